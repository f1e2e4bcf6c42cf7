"""rptgpu_trace_rays without a GPU: the two symbols and RptRayQuery's layout against the header, every refusal that comes
before the device with its code and detail, no CPU fallback, and the piece arithmetic of rpt_amd/csrc/render_plan.h
(rays_piece) compiled with g++ next to a driver that pins it (tests/cpp/rays_piece_check.cpp)."""
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
FIELDS = ("struct_size", "max_bounces", "iterations", "first_draw", "exposure_value", "seed", "sample_index_base",
          "precision_mode", "flags")


def test_symbols_and_struct_size_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert hasattr(lib, "rptgpu_trace_rays") and hasattr(lib, "rptgpu_trace_rays_device")
    names = {s[0] for s in _abi.SYMBOLS}
    assert {"rptgpu_trace_rays", "rptgpu_trace_rays_device"} <= names
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptRayQuery));' + \
          "".join('printf(" %%zu", offsetof(RptRayQuery, %s));' % f for f in FIELDS) + 'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(_abi.RptRayQuery) == nums[0] == 48
    assert [getattr(_abi.RptRayQuery, f).offset for f in FIELDS] == nums[1:]
    assert [f for f, _ in _abi.RptRayQuery._fields_] == list(FIELDS)


def _query(**kw):
    q = _abi.RptRayQuery()
    q.struct_size, q.max_bounces, q.iterations = C.sizeof(_abi.RptRayQuery), 2, 1
    for k, v in kw.items():
        setattr(q, k, v)
    return q


REFUSALS = [
    ("no query", dict(q=None), b"null RptRayQuery"),
    ("size 0", dict(q=_query(struct_size=0)), b"RptRayQuery: struct_size is not sizeof(RptRayQuery)"),
    ("size 40", dict(q=_query(struct_size=40)), b"RptRayQuery: struct_size is not sizeof(RptRayQuery)"),
    ("size 56", dict(q=_query(struct_size=56)), b"RptRayQuery: struct_size is not sizeof(RptRayQuery)"),
    ("iterations", dict(q=_query(iterations=0)), b"RptRayQuery: iterations == 0"),
    ("bounces", dict(q=_query(max_bounces=255)), b"RptRayQuery: max_bounces > 254"),
    ("mode", dict(q=_query(precision_mode=1)),
     b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"),
    ("persistent", dict(q=_query(flags=_abi.RPT_FLAG_PERSISTENT)),
     "RptRayQuery: RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; caller-supplied rays run "
     "the wavefront pipeline only".encode()),
    ("persistent | wavefront", dict(q=_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)),
     "RptRayQuery: RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; caller-supplied rays run "
     "the wavefront pipeline only".encode()),
    ("origins", dict(origins=False), b"null argument"),
    ("dirs", dict(dirs=False), b"null argument"),
    ("out", dict(out=False), b"null argument"),
    ("2^32 + 1 rays without ids", dict(n=(1 << 32) + 1, streams=False),
     b"more than 2^32 rays without stream ids (a stream id has 32 bits)"),
    ("handle", dict(), b"null handle"),
    ("handle, no ids", dict(streams=False), b"null handle"),
    ("handle, no rays", dict(n=0, origins=False, dirs=False, out=False, streams=False), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_every_refusal_comes_before_the_device(row, device):
    """... so each of them is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    o, d, out = np.full(12, 7.0), np.full(12, 7.0), np.full(12, 7.0)
    ids = np.full(4, 7, dtype=np.uint32)
    q = kw.get("q", _query())
    use = lambda name, a: a if kw.get(name, True) else None
    # a call with another detail first: the text below is this call's
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    if device:  # (pointers that are never followed: every row is refused before the device is looked at)
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib.rptgpu_trace_rays_device(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), p(use("streams", ids)),
                                          C.byref(q) if q is not None else None, p(use("out", out)), None)
    else:
        p = lambda a: a.ctypes.data_as(PD) if a is not None else None
        s = use("streams", ids)
        rc = lib.rptgpu_trace_rays(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)),
                                   s.ctypes.data_as(C.POINTER(C.c_uint32)) if s is not None else None,
                                   C.byref(q) if q is not None else None, p(use("out", out)))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and (out == 7).all() and (ids == 7).all()


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never radiance from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    o = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1))
    if gpu_available:
        out = rpt_amd.GpuScene(scene).trace_rays(o, d, 2, samples=2)
        assert out.shape == (4, 3) and np.isfinite(out).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).trace_rays(o, d, 2, samples=2)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


def test_python_wrapper_checks_its_shapes():
    """GpuScene.trace_rays refuses mismatched arrays itself (the C call takes one n for all of them)"""
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    with pytest.raises(ValueError, match="3 origins for 2 directions"):
        g.trace_rays(np.zeros((3, 3)), np.zeros((2, 3)), 1)
    with pytest.raises(ValueError, match="5 stream ids for 3 rays"):
        g.trace_rays(np.zeros((3, 3)), np.zeros((3, 3)), 1, streams=np.arange(5))
    with pytest.raises(ValueError, match="out must be"):
        g.trace_rays(np.zeros((3, 3)), np.zeros((3, 3)), 1, out=np.zeros((3, 3), dtype=np.float32))
    with pytest.raises(rpt_amd.RptGpuError) as e:  # well-formed arrays: the library speaks (no handle)
        g.trace_rays(np.zeros((3, 3)), np.zeros((3, 3)), 1)
    assert e.value.code == E and "null handle" in str(e.value)
    g.handle = None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rays_piece") / "rays_piece_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cpp", "rays_piece_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover", "passes"])
def test_rays_piece(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
