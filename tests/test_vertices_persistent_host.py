"""RPT_FLAG_VERTICES_PERSISTENT (include/rpt_gpu_vertices_persistent.h) without a GPU: the flag's value
against the compiled header, the symbol a binding detects it by, the one new refusal that comes before the device — the flag
beside RPT_FLAG_WAVEFRONT in rptgpu_trace_vertices[_device] — and the two old ones with the texts they always had, whatever
stands beside them, each with its code, its detail and untouched arrays; that rptgpu_trace_rays does not read the bit; and the
host-only piece of a flagged call (rpt_amd/csrc/render_plan.h vertices_persistent_piece:
tests/cpp/vertices_persistent_piece_check.cpp, built plain and with AddressSanitizer and UBSan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi

import test_first_hits_host as HH
import test_rays_persistent_host as RH
import test_trace_rays_host as TH
import test_vertices_host as XH

E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
PU = C.POINTER(C.c_uint32)
ROOT = TH.ROOT
FLAG = getattr(_abi, "RPT_FLAG_VERTICES_PERSISTENT", 64)
WF, GEN, PROF, PERS, RAYS = (_abi.RPT_FLAG_WAVEFRONT, _abi.RPT_FLAG_GENERAL_TRAVERSAL, _abi.RPT_FLAG_PROFILE_KERNELS,
                             _abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_RAYS_PERSISTENT)
BOTH = "RptVertexQuery: RPT_FLAG_VERTICES_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes".encode()


def test_the_flag_is_the_headers(tmp_path):
    src = '#include <stdio.h>\n#include "rpt_gpu.h"\nint main(void){printf("%u %u %u %u %u %u %u\\n", RPT_FLAG_VERTICES_PERSISTENT, ' \
          '(unsigned)RPT_FLAG_PROFILE_KERNELS, (unsigned)RPT_FLAG_WAVEFRONT, (unsigned)RPT_FLAG_GENERAL_TRAVERSAL, ' \
          '(unsigned)RPT_FLAG_PERSISTENT, (unsigned)RPT_FLAG_VIEWS_PERSISTENT, (unsigned)RPT_FLAG_RAYS_PERSISTENT);return 0;}'
    c = tmp_path / "flag.c"
    c.write_text(src)
    exe = tmp_path / "flag"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == FLAG == _abi.RPT_FLAG_VERTICES_PERSISTENT == 64
    assert bin(FLAG).count("1") == 1 and not any(FLAG & x for x in nums[1:])  # a bit of its own among the six others
    assert nums[1:] == [PROF, WF, GEN, PERS, _abi.RPT_FLAG_VIEWS_PERSISTENT, RAYS] and len(set(nums)) == 7


def test_the_detection_symbol_exists(tmp_path):
    lib = _abi.load_library()
    assert hasattr(lib, "rptgpu_vertices_persistent_supported")
    assert lib.rptgpu_vertices_persistent_supported() == 1
    assert _abi.vertices_persistent_supported() is True
    names = {s[0] for s in _abi.VERTICES_PERSISTENT_SYMBOLS}
    assert names == {"rptgpu_vertices_persistent_supported"} and not names & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # an addition within ABI 7

    class Older:  # a library without the symbol: still ABI 7, and the binding says no
        pass
    assert _abi.vertices_persistent_supported(Older()) is False
    header = open(ROOT + "/include/rpt_gpu_vertices_persistent.h").read()
    assert "int rptgpu_vertices_persistent_supported(void);" in header
    main = open(ROOT + "/include/rpt_gpu.h").read()
    assert '#include "rpt_gpu_vertices_persistent.h"' in main and "RPT_FLAG_VERTICES_PERSISTENT = 64u" in main
    assert "rptgpu_vertices_persistent_supported(void);" not in main  # (rpt_gpu.h declares no new symbol of its own)
    assert main.index('#include "rpt_gpu_rays_persistent.h"') < main.index('#include "rpt_gpu_vertices_persistent.h"')
    assert main.index('#include "rpt_gpu_vertices.h"') < main.index('#include "rpt_gpu_vertices_persistent.h"')
    # the vertex call's own header points to the new one
    vertices = open(ROOT + "/include/rpt_gpu_vertices.h").read()
    assert vertices.count("rpt_gpu_vertices_persistent.h") >= 2
    c = tmp_path / "sym.c"
    c.write_text('#include "rpt_gpu.h"\nint main(void){return rptgpu_vertices_persistent_supported != 0;}')
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wno-address", "-I", ROOT + "/include", str(c)])
    rust = open(ROOT + "/rust/rpt-gpu-sys/src/lib.rs").read()
    assert "pub const RPT_FLAG_VERTICES_PERSISTENT: u32 = 64;" in rust and "pub fn rptgpu_vertices_persistent_supported() -> c_int;" in rust


# (name, flags, detail): the new pair by name; the two old flags with their old texts whatever stands beside them — bit 64
# too —; and a well-formed flagged query, which gets as far as the handle
ROWS = [
    ("flag | wavefront", FLAG | WF, BOTH),
    ("flag | wavefront | profile | general", FLAG | WF | PROF | GEN, BOTH),
    ("persistent | flag", PERS | FLAG, XH.PERSISTENT),
    ("persistent | flag | wavefront", PERS | FLAG | WF, XH.PERSISTENT),
    ("rays flag | flag", RAYS | FLAG, RH.NOT_VERTICES),
    ("rays flag | flag | wavefront", RAYS | FLAG | WF, RH.NOT_VERTICES),
    ("persistent | rays flag | flag", PERS | RAYS | FLAG, XH.PERSISTENT),
    ("flag: the handle is next", FLAG, b"null handle"),
    ("flag | general | profile: the handle is next", FLAG | GEN | PROF, b"null handle"),
]


def test_the_old_texts_are_the_old_tests():
    assert XH.PERSISTENT == dict((r[0], r[2]) for r in XH.REFUSALS)["persistent"]
    assert RH.NOT_VERTICES == dict((r[0], r[2]) for r in RH.VERTEX_ROWS)["flag"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_trace_vertices_refusals(row, device):
    _, flags, detail = ROWS[row]
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


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("flags,detail", [(FLAG, b"null handle"), (FLAG | WF, b"null handle"), (FLAG | PERS, RH.RAYS_PERSISTENT),
                                          (FLAG | RAYS | WF, RH.RAYS_BOTH)], ids=["flag", "flag | wavefront", "flag | persistent",
                                                                                  "flag | rays flag | wavefront"])
def test_trace_rays_does_not_read_the_bit(flags, detail, device):
    """rptgpu_trace_rays with bit 64 gets as far as it does without it: to the handle, or to the refusal it always made"""
    lib = _abi.load_library()
    got = []
    for fl in (flags, flags & ~FLAG):
        o, d, out = np.full(12, 7.0), np.full(12, 7.0), np.full(12, 7.0)
        ids = np.full(4, 7, dtype=np.uint32)
        q = TH._query(flags=fl, first_draw=5, iterations=3)
        HH._another_detail_first(lib)
        if device:
            p = lambda a: C.c_void_p(a.ctypes.data)
            rc = lib.rptgpu_trace_rays_device(None, 4, p(o), p(d), p(ids), C.byref(q), p(out), None)
        else:
            rc = lib.rptgpu_trace_rays(None, 4, o.ctypes.data_as(PD), d.ctypes.data_as(PD), ids.ctypes.data_as(PU), C.byref(q),
                                       out.ctypes.data_as(PD))
        got.append((rc, lib.rptgpu_last_error_detail(None)))
        assert (o == 7).all() and (d == 7).all() and (out == 7).all() and (ids == 7).all()
    assert got[0] == got[1] == (E, detail)


def test_no_cpu_fallback(gpu_available):
    """GpuScene.trace_vertices carries the flag to the library (a recorder in its place); with valid arguments and no GPU
    there is no handle to be had: RPTGPU_E_NO_DEVICE, never an answer from the host."""
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = HH.Recorder(), C.c_void_p(0x1234), 0
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    o = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1))
    g.trace_vertices(o, d, 2, samples=2, first_draw=5, flags=FLAG | PROF)
    name, args = g.lib.calls.pop()
    q = [a for a in args if hasattr(a, "_obj") and isinstance(a._obj, _abi.RptVertexQuery)][0]._obj
    assert name == "rptgpu_trace_vertices" and q.flags == FLAG | PROF and q.first_draw == 5
    g.handle = None
    if gpu_available:
        v = rpt_amd.GpuScene(scene).trace_vertices(o, d, 2, samples=2, flags=FLAG)
        assert v.rgb.shape == (4, 3) and np.isfinite(v.rgb).all() and (v.length >= 1).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).trace_vertices(o, d, 2, samples=2, flags=FLAG)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vertices_persistent_piece_" + request.param) / "vertices_persistent_piece_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "vertices_persistent_piece_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "subsets", "plans"])
def test_vertices_persistent_piece(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
