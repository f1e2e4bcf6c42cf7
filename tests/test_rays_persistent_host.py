"""RPT_FLAG_RAYS_PERSISTENT (include/rpt_gpu_rays_persistent.h) without a GPU: the flag's value
against the compiled header, the symbol a binding detects it by, the refusals that come before the device — the flag beside
RPT_FLAG_WAVEFRONT in the four entry points of rptgpu_trace_rays and rptgpu_bake_probes, the flag at all in
rptgpu_trace_vertices[_device], and RPT_FLAG_PERSISTENT with the text it always had — each with its code, its detail and
untouched arrays, no CPU fallback, and the host-only cap of a piece by the kernel's work counter
(rpt_amd/csrc/render_plan.h rays_persistent_piece: tests/cpp/rays_items_check.cpp, built with AddressSanitizer and UBSan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi

import test_first_hits_host as HH
import test_probes_host as PH
import test_trace_rays_host as TH
import test_vertices_host as XH

E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
PU = C.POINTER(C.c_uint32)
ROOT = TH.ROOT
FLAG = getattr(_abi, "RPT_FLAG_RAYS_PERSISTENT", 32)
WF, GEN, PROF, PERS = (_abi.RPT_FLAG_WAVEFRONT, _abi.RPT_FLAG_GENERAL_TRAVERSAL, _abi.RPT_FLAG_PROFILE_KERNELS,
                       _abi.RPT_FLAG_PERSISTENT)
RAYS_BOTH = "RptRayQuery: RPT_FLAG_RAYS_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes".encode()
PROBES_BOTH = "RptProbeQuery: RPT_FLAG_RAYS_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes".encode()
RAYS_PERSISTENT = ("RptRayQuery: RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; caller-supplied rays "
                   "run the wavefront pipeline only").encode()
NOT_VERTICES = ("RptVertexQuery: RPT_FLAG_RAYS_PERSISTENT — only rptgpu_trace_rays, rptgpu_bake_probes and their _device forms "
                "run in the persistent kernel, which leaves no vertices behind").encode()


def test_the_flag_is_the_headers(tmp_path):
    src = '#include <stdio.h>\n#include "rpt_gpu.h"\nint main(void){printf("%u %u %u %u %u %u\\n", RPT_FLAG_RAYS_PERSISTENT, ' \
          '(unsigned)RPT_FLAG_PROFILE_KERNELS, (unsigned)RPT_FLAG_WAVEFRONT, (unsigned)RPT_FLAG_GENERAL_TRAVERSAL, ' \
          '(unsigned)RPT_FLAG_PERSISTENT, (unsigned)RPT_FLAG_VIEWS_PERSISTENT);return 0;}'
    c = tmp_path / "flag.c"
    c.write_text(src)
    exe = tmp_path / "flag"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == FLAG == _abi.RPT_FLAG_RAYS_PERSISTENT == 32
    assert FLAG not in nums[1:] and bin(FLAG).count("1") == 1  # a bit of its own
    assert nums[1:] == [PROF, WF, GEN, PERS, _abi.RPT_FLAG_VIEWS_PERSISTENT]


def test_the_detection_symbol_exists(tmp_path):
    lib = _abi.load_library()
    assert hasattr(lib, "rptgpu_rays_persistent_supported")
    assert lib.rptgpu_rays_persistent_supported() == 1
    assert _abi.rays_persistent_supported() is True
    names = {s[0] for s in _abi.RAYS_PERSISTENT_SYMBOLS}
    assert names == {"rptgpu_rays_persistent_supported"} and not names & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # an addition within ABI 7

    class Older:  # a library without the symbol: still ABI 7, and the binding says no
        pass
    assert _abi.rays_persistent_supported(Older()) is False
    header = open(ROOT + "/include/rpt_gpu_rays_persistent.h").read()
    assert "int rptgpu_rays_persistent_supported(void);" in header
    main = open(ROOT + "/include/rpt_gpu.h").read()
    assert '#include "rpt_gpu_rays_persistent.h"' in main and "RPT_FLAG_RAYS_PERSISTENT = 32u" in main
    assert main.index('#include "rpt_gpu_views_persistent.h"') < main.index('#include "rpt_gpu_rays_persistent.h"')
    c = tmp_path / "sym.c"
    c.write_text('#include "rpt_gpu.h"\nint main(void){return rptgpu_rays_persistent_supported != 0;}')
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wno-address", "-I", ROOT + "/include", str(c)])


# (name, flags, the ray call's detail, the probe call's): what the four entry points refuse of the flags — the new pair by
# name, the old flag with the old text whatever stands beside it — and a well-formed flagged query, which gets as far as the
# handle
ROWS = [
    ("flag | wavefront", FLAG | WF, RAYS_BOTH, PROBES_BOTH),
    ("flag | wavefront | profile | general", FLAG | WF | PROF | GEN, RAYS_BOTH, PROBES_BOTH),
    ("persistent", PERS, RAYS_PERSISTENT, PH.PERSISTENT),
    ("persistent | flag", PERS | FLAG, RAYS_PERSISTENT, PH.PERSISTENT),
    ("persistent | flag | wavefront", PERS | FLAG | WF, RAYS_PERSISTENT, PH.PERSISTENT),
    ("flag: the handle is next", FLAG, b"null handle", b"null handle"),
    ("flag | general | profile: the handle is next", FLAG | GEN | PROF, b"null handle", b"null handle"),
]


def test_the_old_text_is_the_old_tests():
    assert RAYS_PERSISTENT == dict((r[0], r[2]) for r in TH.REFUSALS)["persistent"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_trace_rays_refusals(row, device):
    _, flags, detail, _ = ROWS[row]
    lib = _abi.load_library()
    o, d, out = np.full(12, 7.0), np.full(12, 7.0), np.full(12, 7.0)
    ids = np.full(4, 7, dtype=np.uint32)
    q = TH._query(flags=flags, first_draw=5, iterations=3)
    HH._another_detail_first(lib)
    if device:
        p = lambda a: C.c_void_p(a.ctypes.data)
        rc = lib.rptgpu_trace_rays_device(None, 4, p(o), p(d), p(ids), C.byref(q), p(out), None)
    else:
        rc = lib.rptgpu_trace_rays(None, 4, o.ctypes.data_as(PD), d.ctypes.data_as(PD), ids.ctypes.data_as(PU), C.byref(q),
                                   out.ctypes.data_as(PD))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and (out == 7).all() and (ids == 7).all()


@pytest.mark.parametrize("kind", [_abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE], ids=["sh9", "irradiance"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_bake_probes_refusals(row, device, kind):
    _, flags, _, detail = ROWS[row]
    lib = _abi.load_library()
    pos, nrm, out = np.full(12, 7.0), np.full(12, 7.0), np.full(4 * 27, 7.0)
    ids = np.full(4, 7, dtype=np.uint32)
    q = PH._query(flags=flags, kind=kind)
    HH._another_detail_first(lib)
    if device:
        p = lambda a: C.c_void_p(a.ctypes.data)
        rc = lib.rptgpu_bake_probes_device(None, 4, p(pos), p(nrm), p(ids), C.byref(q), p(out), None)
    else:
        rc = lib.rptgpu_bake_probes(None, 4, pos.ctypes.data_as(PD), nrm.ctypes.data_as(PD), ids.ctypes.data_as(PU), C.byref(q),
                                    out.ctypes.data_as(PD))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (pos == 7).all() and (nrm == 7).all() and (out == 7).all() and (ids == 7).all()


VERTEX_ROWS = [
    ("flag", FLAG, NOT_VERTICES),
    ("flag | wavefront", FLAG | WF, NOT_VERTICES),
    ("flag | general | profile", FLAG | GEN | PROF, NOT_VERTICES),
    ("persistent | flag", PERS | FLAG, XH.PERSISTENT),
    ("persistent", PERS, XH.PERSISTENT),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(VERTEX_ROWS)), ids=[r[0] for r in VERTEX_ROWS])
def test_trace_vertices_refuses_the_flag(row, device):
    _, flags, detail = VERTEX_ROWS[row]
    lib = _abi.load_library()
    o, d, ids = np.full(3 * XH.N, 7.0), np.full(3 * XH.N, 7.0), np.full(XH.N, 7, dtype=np.uint32)
    outs = XH.sentinel_arrays()
    q = XH.vertex_query(flags=flags)
    a = _abi.RptVertexArrays()
    a.struct_size = C.sizeof(_abi.RptVertexArrays)
    types = dict(_abi.RptVertexArrays._fields_)
    for name, arr in outs.items():
        setattr(a, name, arr.ctypes.data_as(types[name]))
    HH._another_detail_first(lib)
    if device:
        p = lambda arr: C.c_void_p(arr.ctypes.data)
        rc = lib.rptgpu_trace_vertices_device(None, XH.N, p(o), p(d), p(ids), C.byref(q), C.byref(a), None)
    else:
        rc = lib.rptgpu_trace_vertices(None, XH.N, o.ctypes.data_as(PD), d.ctypes.data_as(PD), ids.ctypes.data_as(PU), C.byref(q),
                                       C.byref(a))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and (ids == 7).all() and all((arr == 7).all() for arr in outs.values())


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never an answer from the host; and
    GpuScene.trace_rays and GpuScene.bake_probes carry the flag to the library (a recorder in its place)."""
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = HH.Recorder(), C.c_void_p(0x1234), 0
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    o = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1))
    g.trace_rays(o, d, 2, samples=2, first_draw=5, flags=FLAG | PROF)
    name, args = g.lib.calls.pop()
    q = [a for a in args if hasattr(a, "_obj") and isinstance(a._obj, _abi.RptRayQuery)][0]._obj
    assert name == "rptgpu_trace_rays" and q.flags == FLAG | PROF and q.first_draw == 5
    g.bake_probes(o, d, kind=_abi.RPT_PROBE_IRRADIANCE, samples=3, max_bounces=2, seed=1, flags=FLAG)
    name, args = g.lib.calls.pop()
    q = [a for a in args if hasattr(a, "_obj") and isinstance(a._obj, _abi.RptProbeQuery)][0]._obj
    assert name == "rptgpu_bake_probes" and q.flags == FLAG and q.kind == _abi.RPT_PROBE_IRRADIANCE
    g.handle = None
    if gpu_available:
        g2 = rpt_amd.GpuScene(scene)
        out = g2.trace_rays(o, d, 2, samples=2, flags=FLAG)
        assert out.shape == (4, 3) and np.isfinite(out).all()
        sh = g2.bake_probes(o, kind=_abi.RPT_PROBE_SH9, samples=3, max_bounces=2, seed=1, flags=FLAG)
        assert sh.shape == (4, 9, 3) and np.isfinite(sh).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).trace_rays(o, d, 2, samples=2, flags=FLAG)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).bake_probes(o, kind=_abi.RPT_PROBE_SH9, samples=3, max_bounces=2, seed=1, flags=FLAG)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rays_items") / "rays_items_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "rays_items_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "plans", "edge"])
def test_rays_items(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
