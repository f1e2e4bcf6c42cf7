"""rptgpu_trace_vertices without a GPU: the two symbols and both structs' layouts against the compiled header, every refusal
that comes before the device — through the host and the device entry points, with its code, its detail and the sentinel-filled
arrays untouched —, no CPU fallback, what GpuScene.trace_vertices lowers its arguments to, and the piece planner
(rpt_amd/csrc/render_plan.h vertices_piece) in a stand-alone program (tests/cpp/vertices_piece_check.cpp), plain and under
AddressSanitizer + UBSan."""
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
NAMES = ("rptgpu_trace_vertices", "rptgpu_trace_vertices_device")
QUERY_FIELDS = ("struct_size", "max_bounces", "iterations", "first_draw", "exposure_value", "seed", "sample_index_base",
                "precision_mode", "flags", "channels", "reserved")
ARRAY_FIELDS = ("struct_size", "reserved", "length", "t", "normal", "object", "position", "direction", "draw", "radiance", "bsdf",
                "inv_pdf", "abs_cos", "rgb")
CHANNELS = ("LENGTH", "T", "NORMAL", "OBJECT", "POSITION", "DIRECTION", "DRAW", "RADIANCE", "BSDF", "INV_PDF", "ABS_COS", "RGB")
B, S, N = 2, 2, 4  # the refusals' call: 4 rays, 2 samples, 3 vertices per path


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES)
    assert set(NAMES) == {s[0] for s in _abi.VERTICES_SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    header = open(ROOT + "/include/rpt_gpu_vertices.h").read()
    assert all("int %s(" % n in header for n in NAMES)
    assert '#include "rpt_gpu_vertices.h"' in open(ROOT + "/include/rpt_gpu.h").read()
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptVertexQuery));' + \
          "".join('printf(" %%zu", offsetof(RptVertexQuery, %s));' % f for f in QUERY_FIELDS) + \
          'printf(" %zu", sizeof(RptVertexArrays));' + \
          "".join('printf(" %%zu", offsetof(RptVertexArrays, %s));' % f for f in ARRAY_FIELDS) + \
          "".join('printf(" %%u", RPT_VERTEX_%s);' % c for c in CHANNELS) + 'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    q, a, bits = nums[:12], nums[12:27], nums[27:]
    assert C.sizeof(_abi.RptVertexQuery) == q[0] == 56
    assert [getattr(_abi.RptVertexQuery, f).offset for f in QUERY_FIELDS] == q[1:] == [0, 4, 8, 12, 16, 24, 32, 40, 44, 48, 52]
    assert [f for f, _ in _abi.RptVertexQuery._fields_] == list(QUERY_FIELDS)
    # (RptRayQuery's fields at RptRayQuery's offsets: a caller's query for trace_rays is the head of this one)
    assert [getattr(_abi.RptRayQuery, f).offset for f, _ in _abi.RptRayQuery._fields_] == q[1:10]
    assert C.sizeof(_abi.RptVertexArrays) == a[0] == 104
    assert [getattr(_abi.RptVertexArrays, f).offset for f in ARRAY_FIELDS] == a[1:] == [0, 4] + [8 * k for k in range(1, 13)]
    assert [f for f, _ in _abi.RptVertexArrays._fields_] == list(ARRAY_FIELDS)
    assert bits == [getattr(_abi, "RPT_VERTEX_" + c) for c in CHANNELS] == [1 << k for k in range(12)] and _abi.RPT_VERTEX_ALL == 4095
    assert all(getattr(rpt_amd, "RPT_VERTEX_" + c) == 1 << k for k, c in enumerate(CHANNELS))


def vertex_query(**kw):
    q = _abi.RptVertexQuery()
    q.struct_size, q.max_bounces, q.iterations, q.channels = C.sizeof(_abi.RptVertexQuery), B, S, _abi.RPT_VERTEX_ALL
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RptVertexQuery: RPT_FLAG_PERSISTENT — the persistent kernel keeps a path in registers and leaves no vertices behind; "
              "path vertices run the wavefront pipeline only").encode()
MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
Q_SIZE = b"RptVertexQuery: struct_size is not sizeof(RptVertexQuery)"
A_SIZE = b"RptVertexArrays: struct_size is not sizeof(RptVertexArrays)"
UNKNOWN = b"RptVertexQuery: channels names an unknown RPT_VERTEX_* bit"
TOO_MANY = b"n * iterations * (max_bounces + 1) does not fit: 2^56 vertices or more would not fit any memory"
# (what is passed: q, the arrays struct's fields, which arrays are NULL, n) -> the detail
REFUSALS = [
    ("no query", dict(q=None), b"null RptVertexQuery"),
    ("no arrays struct", dict(arrays=None), b"null RptVertexArrays"),
    ("query size 0", dict(q=vertex_query(struct_size=0)), Q_SIZE),
    ("query size 48 (an RptRayQuery)", dict(q=vertex_query(struct_size=48)), Q_SIZE),
    ("query size 64", dict(q=vertex_query(struct_size=64)), Q_SIZE),
    ("arrays size 0", dict(a_size=0), A_SIZE),
    ("arrays size 96", dict(a_size=96), A_SIZE),
    ("arrays size 112", dict(a_size=112), A_SIZE),
    ("iterations", dict(q=vertex_query(iterations=0)), b"RptVertexQuery: iterations == 0"),
    ("bounces", dict(q=vertex_query(max_bounces=255)), b"RptVertexQuery: max_bounces > 254"),
    ("mode", dict(q=vertex_query(precision_mode=1)), MODE),
    ("persistent", dict(q=vertex_query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=vertex_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("no channel", dict(q=vertex_query(channels=0)), b"RptVertexQuery: channels == 0 (name at least one RPT_VERTEX_* channel)"),
    ("unknown bit", dict(q=vertex_query(channels=(1 << 12) | _abi.RPT_VERTEX_T)), UNKNOWN),
    ("high bit", dict(q=vertex_query(channels=1 << 31)), UNKNOWN),
    ("query reserved", dict(q=vertex_query(reserved=1)), b"RptVertexQuery: reserved != 0"),
    ("arrays reserved", dict(reserved=1), b"RptVertexArrays: reserved != 0"),
] + [(f, {f: False}, ("RptVertexArrays: RPT_VERTEX_%s is named but %s is NULL" % (f.upper(), f)).encode()) for f in ARRAY_FIELDS[2:]] + [
    ("origins", dict(origins=False), b"null argument"),
    ("dirs", dict(dirs=False), b"null argument"),
    ("2^32 + 1 rays without ids", dict(n=(1 << 32) + 1, streams=False, q=vertex_query(iterations=1, max_bounces=0)),
     b"more than 2^32 rays without stream ids (a stream id has 32 bits)"),
    ("2^56 vertices", dict(n=1 << 48, q=vertex_query(iterations=16, max_bounces=15)), TOO_MANY),
    ("2^64 rays' worth", dict(n=(1 << 64) - 1, q=vertex_query(iterations=0xffffffff, max_bounces=254)), TOO_MANY),
    ("handle", dict(), b"null handle"),
    ("handle, just under 2^56 vertices", dict(n=(1 << 48) - 1, q=vertex_query(iterations=16, max_bounces=15)), b"null handle"),
    ("handle, one channel and only its array",
     dict(q=vertex_query(channels=_abi.RPT_VERTEX_OBJECT), **{f: False for f in ARRAY_FIELDS[2:] if f != "object"}), b"null handle"),
    ("handle, no rays", dict(n=0, origins=False, dirs=False), b"null handle"),
]


def _another_detail_first(lib):
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"


def sentinel_arrays():
    per = {"length": ((N, S), np.uint32), "object": ((N, S, B + 1), np.int32), "draw": ((N, S, B + 1), np.uint32), "rgb": ((N, 3), np.float64)}
    for f in ("t", "inv_pdf", "abs_cos"):
        per[f] = ((N, S, B + 1), np.float64)
    for f in ("normal", "position", "direction", "radiance", "bsdf"):
        per[f] = ((N, S, B + 1, 3), np.float64)
    return {f: np.full(shape, 7, dtype=dtype) for f, (shape, dtype) in per.items()}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_refuses_before_the_device(row, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    o, d, ids = np.full(3 * N, 7.0), np.full(3 * N, 7.0), np.full(N, 7, dtype=np.uint32)
    outs = sentinel_arrays()
    q = kw.get("q", vertex_query())
    a = _abi.RptVertexArrays()
    a.struct_size, a.reserved = kw.get("a_size", C.sizeof(_abi.RptVertexArrays)), kw.get("reserved", 0)
    types = dict(_abi.RptVertexArrays._fields_)
    for name, arr in outs.items():  # (device: pointers that are never followed — every row is refused before the device)
        if kw.get(name, True):
            setattr(a, name, arr.ctypes.data_as(types[name]))
    ap = C.byref(a) if kw.get("arrays", True) is not None else None
    qp = C.byref(q) if q is not None else None
    use = lambda name, arr: arr if kw.get(name, True) else None
    _another_detail_first(lib)
    if device:
        p = lambda arr: C.c_void_p(arr.ctypes.data) if arr is not None else None
        rc = lib.rptgpu_trace_vertices_device(None, kw.get("n", N), p(use("origins", o)), p(use("dirs", d)), p(use("streams", ids)), qp, ap, None)
    else:
        p = lambda arr: arr.ctypes.data_as(PD) if arr is not None else None
        s = ids.ctypes.data_as(C.POINTER(C.c_uint32)) if kw.get("streams", True) else None
        rc = lib.rptgpu_trace_vertices(None, kw.get("n", N), p(use("origins", o)), p(use("dirs", d)), s, qp, ap)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and (ids == 7).all() and all((arr == 7).all() for arr in outs.values())


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never an answer from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    o = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1))
    if gpu_available:
        g = rpt_amd.GpuScene(scene)
        v = g.trace_vertices(o, d, 2, samples=2)
        assert (v.object[:, :, 0] >= 0).all() and (v.length >= 1).all() and np.isfinite(v.rgb).all()
        assert (g.trace_vertices(o, -d, 2, channels=_abi.RPT_VERTEX_LENGTH).length == 1).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).trace_vertices(o, d, 2)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


class Recorder:
    """stands where the library stands in a GpuScene: keeps what the entry points are called with"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("rptgpu_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _address(p):
    return C.cast(p, C.c_void_p).value


def test_what_the_python_call_lowers_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    o = np.arange(12.0).reshape(4, 3)
    d = o[::-1] * 0.5            # not contiguous: the call sees a contiguous copy
    v = g.trace_vertices(o, d, 5, samples=3, seed=(1 << 63) + 5, sample_index_base=1 << 40, first_draw=2, exposure_value=1.5,
                         streams=[9, 8, 7, 6], flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, po, pd, ps, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert name == "rptgpu_trace_vertices" and h is g.handle and n == 4
    assert (q.struct_size, q.max_bounces, q.iterations, q.first_draw, q.exposure_value) == (56, 5, 3, 2, 1.5)
    assert (q.seed, q.sample_index_base, q.precision_mode, q.flags) == ((1 << 63) + 5, 1 << 40, 0, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert (q.channels, q.reserved, a.struct_size, a.reserved) == (4095, 0, 104, 0)
    as_floats = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
    assert (as_floats(po, 12) == o.ravel()).all() and (as_floats(pd, 12) == d.ravel()).all()
    assert list(np.ctypeslib.as_array(ps, shape=(4,))) == [9, 8, 7, 6]
    assert isinstance(v, rpt_amd.PathVertices) and v.channels == 4095 and sorted(v.arrays()) == sorted(ARRAY_FIELDS[2:])
    assert v.length.shape == (4, 3) and v.length.dtype == np.uint32 and v.rgb.shape == (4, 3)
    for k in ("t", "inv_pdf", "abs_cos"):
        assert getattr(v, k).shape == (4, 3, 6) and getattr(v, k).dtype == np.float64
    for k in ("normal", "position", "direction", "radiance", "bsdf"):
        assert getattr(v, k).shape == (4, 3, 6, 3) and getattr(v, k).dtype == np.float64
    assert v.object.shape == (4, 3, 6) and v.object.dtype == np.int32 and v.draw.shape == (4, 3, 6) and v.draw.dtype == np.uint32
    for k, arr in v.arrays().items():
        assert _address(getattr(a, k)) == arr.ctypes.data
    # two channels: the other pointers stay NULL, the other attributes None; no ids: NULL
    v = g.trace_vertices(o, d, 1, channels=_abi.RPT_VERTEX_LENGTH | _abi.RPT_VERTEX_POSITION)
    name, (h, n, po, pd, ps, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert sorted(v.arrays()) == ["length", "position"] and v.t is None and v.rgb is None
    assert (q.channels, q.iterations, q.seed, q.first_draw, q.flags) == (17, 1, 0x52505447, 0, 0) and ps is None
    assert all(not getattr(a, f) for f in ARRAY_FIELDS[2:] if f not in ("length", "position"))
    assert _address(a.position) == v.position.ctypes.data and v.position.shape == (4, 1, 2, 3)
    assert not g.lib.calls
    g.handle = None


def test_the_python_call_checks_its_shapes_and_dtypes():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    z = np.zeros((3, 3))
    with pytest.raises(ValueError, match=r"origins must be an \(n, 3\) float64 array"):
        g.trace_vertices(np.zeros((3, 2)), z, 2)
    with pytest.raises(ValueError, match=r"dirs must be an \(n, 3\) float64 array"):
        g.trace_vertices(z, z.astype(np.float32), 2)
    with pytest.raises(ValueError, match="3 origins for 2 directions"):
        g.trace_vertices(z, np.zeros((2, 3)), 2)
    with pytest.raises(ValueError, match="2 stream ids for 3 rays"):
        g.trace_vertices(z, z, 2, streams=[1, 2])
    for call, word in ((lambda: g.trace_vertices(z, z, 2), "null handle"),  # well-formed arrays: the library speaks
                       (lambda: g.trace_vertices(z, z, 2, channels=0), "channels == 0"),
                       (lambda: g.trace_vertices(z, z, 2, channels=1 << 12), "unknown RPT_VERTEX_"),
                       (lambda: g.trace_vertices(z, z, 255), "max_bounces > 254"),
                       (lambda: g.trace_vertices(z, z, 2, samples=0), "iterations == 0")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call()
        assert e.value.code == E and word in str(e.value)
    g.handle = None


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vertices_piece_" + request.param) / "vertices_piece_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "vertices_piece_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover", "staging"])
def test_vertices_piece(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
