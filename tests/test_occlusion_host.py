"""rptgpu_occluded and rptgpu_bake_ao without a GPU: the four symbols and both structs' layouts against the header, every
refusal that comes before the device — through all four entry points, with its code, its detail and the output arrays
untouched —, no CPU fallback, and what GpuScene.occluded / GpuScene.bake_ao lower their arguments to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_occluded", "rptgpu_occluded_device", "rptgpu_bake_ao", "rptgpu_bake_ao_device")
VIS_FIELDS = ("struct_size", "precision_mode", "flags", "reserved")
AO_FIELDS = ("struct_size", "samples", "seed", "sample_index_base", "max_distance", "precision_mode", "flags")


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES)
    assert set(NAMES) <= {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptVisibilityQuery));' + \
          "".join('printf(" %%zu", offsetof(RptVisibilityQuery, %s));' % f for f in VIS_FIELDS) + \
          'printf(" %zu", sizeof(RptAoQuery));' + \
          "".join('printf(" %%zu", offsetof(RptAoQuery, %s));' % f for f in AO_FIELDS) + 'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    vis, ao = nums[:1 + len(VIS_FIELDS)], nums[1 + len(VIS_FIELDS):]
    assert C.sizeof(_abi.RptVisibilityQuery) == vis[0] == 16
    assert [getattr(_abi.RptVisibilityQuery, f).offset for f in VIS_FIELDS] == vis[1:] == [0, 4, 8, 12]
    assert [f for f, _ in _abi.RptVisibilityQuery._fields_] == list(VIS_FIELDS)
    assert C.sizeof(_abi.RptAoQuery) == ao[0] == 40
    assert [getattr(_abi.RptAoQuery, f).offset for f in AO_FIELDS] == ao[1:] == [0, 4, 8, 16, 24, 32, 36]
    assert [f for f, _ in _abi.RptAoQuery._fields_] == list(AO_FIELDS)


def vis_query(**kw):
    q = _abi.RptVisibilityQuery()
    q.struct_size = C.sizeof(_abi.RptVisibilityQuery)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def ao_query(**kw):
    q = _abi.RptAoQuery()
    q.struct_size, q.samples, q.seed, q.max_distance = C.sizeof(_abi.RptAoQuery), 4, 1, float("inf")
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; visibility queries run the wavefront "
              "pipeline's shadow-ray query only").encode()
MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
VIS_SIZE = b"RptVisibilityQuery: struct_size is not sizeof(RptVisibilityQuery)"
AO_SIZE = b"RptAoQuery: struct_size is not sizeof(RptAoQuery)"
# (what is passed: q, and which arrays are NULL, n) -> the detail
VIS_REFUSALS = [
    ("no query", dict(q=None), b"null RptVisibilityQuery"),
    ("size 0", dict(q=vis_query(struct_size=0)), VIS_SIZE),
    ("size 12", dict(q=vis_query(struct_size=12)), VIS_SIZE),
    ("size 24", dict(q=vis_query(struct_size=24)), VIS_SIZE),
    ("reserved", dict(q=vis_query(reserved=1)), b"RptVisibilityQuery: reserved != 0"),
    ("mode", dict(q=vis_query(precision_mode=1)), MODE),
    ("persistent", dict(q=vis_query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=vis_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("origins", dict(origins=False), b"null argument"),
    ("dirs", dict(dirs=False), b"null argument"),
    ("out", dict(out=False), b"null argument"),
    ("handle", dict(), b"null handle"),
    ("handle, no max_t", dict(max_t=False), b"null handle"),
    ("handle, no rays", dict(n=0, origins=False, dirs=False, max_t=False, out=False), b"null handle"),
]
AO_REFUSALS = [
    ("no query", dict(q=None), b"null RptAoQuery"),
    ("size 0", dict(q=ao_query(struct_size=0)), AO_SIZE),
    ("size 32", dict(q=ao_query(struct_size=32)), AO_SIZE),
    ("size 48", dict(q=ao_query(struct_size=48)), AO_SIZE),
    ("samples", dict(q=ao_query(samples=0)), b"RptAoQuery: samples == 0"),
    ("mode", dict(q=ao_query(precision_mode=1)), MODE),
    ("persistent", dict(q=ao_query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=ao_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("positions", dict(positions=False), b"null argument"),
    ("normals", dict(normals=False), b"null argument"),
    ("out_ao", dict(out_ao=False), b"null argument"),
    ("2^32 + 1 points without ids", dict(n=(1 << 32) + 1, streams=False),
     b"more than 2^32 points without stream ids (a stream id has 32 bits)"),
    ("handle", dict(), b"null handle"),
    ("handle, no ids", dict(streams=False), b"null handle"),
    ("handle, no bent normals", dict(out_bent=False), b"null handle"),
    ("handle, NaN distance", dict(q=ao_query(max_distance=float("nan"))), b"null handle"),
    ("handle, no points", dict(n=0, positions=False, normals=False, streams=False, out_ao=False, out_bent=False), b"null handle"),
]


def _another_detail_first(lib):
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(VIS_REFUSALS)), ids=[r[0] for r in VIS_REFUSALS])
def test_occluded_refuses_before_the_device(row, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    _, kw, detail = VIS_REFUSALS[row]
    lib = _abi.load_library()
    o, d, mt, out = np.full(12, 7.0), np.full(12, 7.0), np.full(4, 7.0), np.full(4, 7, dtype=np.uint8)
    q = kw.get("q", vis_query())
    use = lambda name, a: a if kw.get(name, True) else None
    qp = C.byref(q) if q is not None else None
    _another_detail_first(lib)
    if device:  # (pointers that are never followed: every row is refused before the device is looked at)
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib.rptgpu_occluded_device(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), p(use("max_t", mt)), qp,
                                        p(use("out", out)), None)
    else:
        p = lambda a: a.ctypes.data_as(PD) if a is not None else None
        b = use("out", out)
        rc = lib.rptgpu_occluded(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), p(use("max_t", mt)), qp,
                                 b.ctypes.data_as(C.POINTER(C.c_uint8)) if b is not None else None)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and (mt == 7).all() and (out == 7).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(AO_REFUSALS)), ids=[r[0] for r in AO_REFUSALS])
def test_bake_ao_refuses_before_the_device(row, device):
    _, kw, detail = AO_REFUSALS[row]
    lib = _abi.load_library()
    pos, nrm, ao, bent = np.full(12, 7.0), np.full(12, 7.0), np.full(4, 7.0), np.full(12, 7.0)
    ids = np.full(4, 7, dtype=np.uint32)
    q = kw.get("q", ao_query())
    use = lambda name, a: a if kw.get(name, True) else None
    qp = C.byref(q) if q is not None else None
    _another_detail_first(lib)
    if device:
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib.rptgpu_bake_ao_device(None, kw.get("n", 4), p(use("positions", pos)), p(use("normals", nrm)),
                                       p(use("streams", ids)), qp, p(use("out_ao", ao)), p(use("out_bent", bent)), None)
    else:
        p = lambda a: a.ctypes.data_as(PD) if a is not None else None
        s = use("streams", ids)
        rc = lib.rptgpu_bake_ao(None, kw.get("n", 4), p(use("positions", pos)), p(use("normals", nrm)),
                                s.ctypes.data_as(C.POINTER(C.c_uint32)) if s is not None else None, qp,
                                p(use("out_ao", ao)), p(use("out_bent", bent)))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (pos == 7).all() and (nrm == 7).all() and (ao == 7).all() and (bent == 7).all() and (ids == 7).all()


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never an answer from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    o = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1))
    if gpu_available:
        g = rpt_amd.GpuScene(scene)
        assert g.occluded(o, d).tolist() == [1, 1, 1, 1] and g.occluded(o, -d).tolist() == [0, 0, 0, 0]
        up = np.tile(np.array([0.0, 1.0, 0.0]), (4, 1))
        ao = g.bake_ao(o, up, samples=3, seed=1, max_distance=1.0)  # nothing within 1 above the ground plane
        assert ao.shape == (4,) and (ao == 1.0).all()
        return
    for call in (lambda g: g.occluded(o, d), lambda g: g.bake_ao(o, d, samples=3, seed=1)):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call(rpt_amd.GpuScene(scene))
        assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


class Recorder:
    """stands where the library stands in a GpuScene: keeps what the four entry points are called with"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("rptgpu_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _floats(p, n):
    return np.ctypeslib.as_array(p, shape=(n,)).copy()


def test_what_the_python_calls_lower_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    o = np.arange(12.0).reshape(4, 3)
    d = o[::-1] * 0.5            # not contiguous: the call sees a contiguous copy
    mt = np.array([1.0, np.inf, np.nan, -1.0])
    out = g.occluded(o, d, mt, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, po, pd, pt, q, pout) = g.lib.calls.pop()
    q = q._obj
    assert name == "rptgpu_occluded" and h is g.handle and n == 4
    assert (q.struct_size, q.precision_mode, q.flags, q.reserved) == (16, _abi.RPT_PRECISION_F64_STRICT, _abi.RPT_FLAG_GENERAL_TRAVERSAL, 0)
    assert (_floats(po, 12) == o.ravel()).all() and (_floats(pd, 12) == d.ravel()).all()
    assert _floats(pt, 4).tobytes() == mt.tobytes()
    assert out.dtype == np.uint8 and out.shape == (4,) and C.addressof(pout.contents) == out.ctypes.data
    mine = np.zeros(4, dtype=np.uint8)
    assert g.occluded(o, d, out=mine) is mine
    name, (h, n, po, pd, pt, q, pout) = g.lib.calls.pop()
    assert pt is None and q._obj.flags == 0 and C.addressof(pout.contents) == mine.ctypes.data  # no max_t: NULL

    nrm = np.tile(np.array([0.0, 1.0, 0.0]), (4, 1))
    ao = g.bake_ao(o, nrm, samples=33, seed=(1 << 63) + 5)
    name, (h, n, pp, pn, ps, q, pa, pb) = g.lib.calls.pop()
    q = q._obj
    assert name == "rptgpu_bake_ao" and h is g.handle and n == 4 and ps is None and pb is None
    assert (q.struct_size, q.samples, q.seed, q.sample_index_base, q.precision_mode, q.flags) == (40, 33, (1 << 63) + 5, 0, 0, 0)
    assert q.max_distance == float("inf")
    assert (_floats(pp, 12) == o.ravel()).all() and (_floats(pn, 12) == nrm.ravel()).all()
    assert ao.shape == (4,) and ao.dtype == np.float64 and C.addressof(pa.contents) == ao.ctypes.data
    ao, bent = g.bake_ao(o, nrm, samples=2, seed=3, max_distance=2.5, sample_index_base=1 << 40, streams=[9, 8, 7, 1 << 31],
                         bent_normals=True, flags=_abi.RPT_FLAG_PROFILE_KERNELS)
    name, (h, n, pp, pn, ps, q, pa, pb) = g.lib.calls.pop()
    q = q._obj
    assert (q.samples, q.seed, q.sample_index_base, q.max_distance, q.flags) == (2, 3, 1 << 40, 2.5, _abi.RPT_FLAG_PROFILE_KERNELS)
    assert np.ctypeslib.as_array(ps, shape=(4,)).tolist() == [9, 8, 7, 1 << 31]
    assert bent.shape == (4, 3) and C.addressof(pa.contents) == ao.ctypes.data and C.addressof(pb.contents) == bent.ctypes.data
    a, b = np.zeros(4), np.zeros((4, 3))
    got = g.bake_ao(o, nrm, samples=2, seed=3, bent_normals=True, out=(a, b))
    assert got[0] is a and got[1] is b
    g.lib.calls.pop()
    assert not g.lib.calls
    g.handle = None


def test_the_python_calls_check_their_shapes_and_dtypes():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    z = np.zeros((3, 3))
    with pytest.raises(ValueError, match=r"origins must be an \(n, 3\) float64 array"):
        g.occluded(np.zeros((3, 2)), z)
    with pytest.raises(ValueError, match=r"dirs must be an \(n, 3\) float64 array"):
        g.occluded(z, z.astype(np.float32))
    with pytest.raises(ValueError, match="3 origins for 2 directions"):
        g.occluded(z, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="max_t must be"):
        g.occluded(z, z, np.zeros(4))
    with pytest.raises(ValueError, match="max_t must be"):
        g.occluded(z, z, np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError, match="out must be"):
        g.occluded(z, z, out=np.zeros(3))
    kw = dict(samples=4, seed=1)
    with pytest.raises(ValueError, match=r"positions must be an \(n, 3\) float64 array"):
        g.bake_ao(np.zeros(9), z, **kw)
    with pytest.raises(ValueError, match=r"normals must be an \(n, 3\) float64 array"):
        g.bake_ao(z, z.astype(np.float32), **kw)
    with pytest.raises(ValueError, match="2 normals for 3 positions"):
        g.bake_ao(z, np.zeros((2, 3)), **kw)
    with pytest.raises(ValueError, match="5 stream ids for 3 points"):
        g.bake_ao(z, z, streams=np.arange(5), **kw)
    with pytest.raises(ValueError, match="streams must be"):
        g.bake_ao(z, z, streams=np.arange(3.0), **kw)
    with pytest.raises(ValueError, match="the output for ao must be"):
        g.bake_ao(z, z, out=np.zeros((3, 1)), **kw)
    with pytest.raises(ValueError, match="the output for bent normals must be"):
        g.bake_ao(z, z, bent_normals=True, out=(np.zeros(3), np.zeros(9)), **kw)
    with pytest.raises(ValueError, match="without bent_normals=True"):
        g.bake_ao(z, z, out=(np.zeros(3), np.zeros((3, 3))), **kw)
    with pytest.raises(TypeError):
        g.bake_ao(z, z, 4, 1)  # samples and seed are keyword-only
    for call in (lambda: g.occluded(z, z), lambda: g.bake_ao(z, z, **kw)):  # well-formed arrays: the library speaks
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call()
        assert e.value.code == E and "null handle" in str(e.value)
    g.handle = None
