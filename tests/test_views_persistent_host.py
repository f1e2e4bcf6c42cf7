"""RPT_FLAG_VIEWS_PERSISTENT (include/rpt_gpu_views_persistent.h) without a GPU: the flag's value against
the compiled header, the symbol a binding detects it by, the refusals that come before the device — the flag beside
RPT_FLAG_WAVEFRONT in the four rptgpu_render_views calls, the flag at all in the aov and denoised calls, and
RPT_FLAG_PERSISTENT with the text it always had — each with its code, its detail and untouched arrays, no CPU fallback, and
the host-only planning of a piece's work items (rpt_amd/csrc/render_plan.h views_items: tests/cpp/views_items_check.cpp,
built with AddressSanitizer and UBSan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import View, _abi

import test_first_hits_host as HH
import test_views_denoised_host as DH
import test_views_host as VH

E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
FLAG = _abi.RPT_FLAG_VIEWS_PERSISTENT
BOTH = "RptViewQuery: RPT_FLAG_VIEWS_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes".encode()
NOT_HERE = ("RptViewQuery: RPT_FLAG_VIEWS_PERSISTENT — only rptgpu_render_views and its _seeded and _device forms run a batch "
            "of views in the persistent kernel").encode()
SEEDS = (5, (1 << 63) + 1)


def test_the_flag_is_the_headers(tmp_path):
    src = '#include <stdio.h>\n#include "rpt_gpu.h"\nint main(void){printf("%u %u %u %u %u\\n", RPT_FLAG_VIEWS_PERSISTENT, ' \
          '(unsigned)RPT_FLAG_PROFILE_KERNELS, (unsigned)RPT_FLAG_WAVEFRONT, (unsigned)RPT_FLAG_GENERAL_TRAVERSAL, ' \
          '(unsigned)RPT_FLAG_PERSISTENT);return 0;}'
    c = tmp_path / "flag.c"
    c.write_text(src)
    exe = tmp_path / "flag"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(VH.ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert nums[0] == FLAG == 16
    assert FLAG not in nums[1:] and bin(FLAG).count("1") == 1  # a bit of its own
    assert nums[1:] == [_abi.RPT_FLAG_PROFILE_KERNELS, _abi.RPT_FLAG_WAVEFRONT, _abi.RPT_FLAG_GENERAL_TRAVERSAL,
                        _abi.RPT_FLAG_PERSISTENT]


def test_the_detection_symbol_exists(tmp_path):
    lib = _abi.load_library()
    assert hasattr(lib, "rptgpu_views_persistent_supported")
    assert lib.rptgpu_views_persistent_supported() == 1
    assert _abi.views_persistent_supported() is True
    names = {s[0] for s in _abi.VIEWS_PERSISTENT_SYMBOLS}
    assert names == {"rptgpu_views_persistent_supported"} and not names & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # an addition within ABI 7

    class Older:  # a library without the symbol: still ABI 7, and the binding says no
        pass
    assert _abi.views_persistent_supported(Older()) is False
    header = open(VH.ROOT + "/include/rpt_gpu_views_persistent.h").read()
    assert "int rptgpu_views_persistent_supported(void);" in header
    main = open(VH.ROOT + "/include/rpt_gpu.h").read()
    assert '#include "rpt_gpu_views_persistent.h"' in main and "RPT_FLAG_VIEWS_PERSISTENT = 16u" in main
    c = tmp_path / "sym.c"
    c.write_text('#include "rpt_gpu.h"\nint main(void){return rptgpu_views_persistent_supported != 0;}')
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wno-address", "-I", VH.ROOT + "/include", str(c)])


# (name, flags, detail): what the four rptgpu_render_views calls refuse of the flags — the new pair by name, the old flag
# with the old text whatever stands beside it — and a well-formed flagged query, which gets as far as the handle
VIEWS_ROWS = [
    ("flag | wavefront", FLAG | _abi.RPT_FLAG_WAVEFRONT, BOTH),
    ("flag | wavefront | profile", FLAG | _abi.RPT_FLAG_WAVEFRONT | _abi.RPT_FLAG_PROFILE_KERNELS, BOTH),
    ("persistent", _abi.RPT_FLAG_PERSISTENT, VH.PERSISTENT),
    ("persistent | flag", _abi.RPT_FLAG_PERSISTENT | FLAG, VH.PERSISTENT),
    ("persistent | flag | wavefront", _abi.RPT_FLAG_PERSISTENT | FLAG | _abi.RPT_FLAG_WAVEFRONT, VH.PERSISTENT),
    ("flag: the handle is next", FLAG, b"null handle"),
    ("flag | general | profile: the handle is next", FLAG | _abi.RPT_FLAG_GENERAL_TRAVERSAL | _abi.RPT_FLAG_PROFILE_KERNELS,
     b"null handle"),
]


@pytest.mark.parametrize("seeded", [False, True], ids=["strided", "seeds"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(VIEWS_ROWS)), ids=[r[0] for r in VIEWS_ROWS])
def test_render_views_refusals(row, device, seeded):
    _, flags, detail = VIEWS_ROWS[row]
    lib = _abi.load_library()
    q = VH._query(flags=flags)
    arr = (_abi.RptView * 2)(VH._view(), VH._view(_abi.RPT_VIEW_PANORAMA))
    keep = bytes(arr)
    out = np.full(2 * 5 * 3 * 3, 7.0)
    seeds = (C.c_uint64 * 2)(*SEEDS)
    HH._another_detail_first(lib)
    head = (None, 2, arr, C.byref(q)) + ((seeds,) if seeded else ())
    if device:
        fn = lib.rptgpu_render_views_seeded_device if seeded else lib.rptgpu_render_views_device
        rc = fn(*head, C.c_void_p(out.ctypes.data), 0, None)
    else:
        fn = lib.rptgpu_render_views_seeded if seeded else lib.rptgpu_render_views
        rc = fn(*head, out.ctypes.data_as(PD))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (out == 7).all() and bytes(arr) == keep and tuple(seeds) == SEEDS


OTHER_ROWS = [
    ("flag", FLAG, NOT_HERE),
    ("flag | wavefront", FLAG | _abi.RPT_FLAG_WAVEFRONT, NOT_HERE),
    ("flag | general", FLAG | _abi.RPT_FLAG_GENERAL_TRAVERSAL, NOT_HERE),
    ("persistent | flag", _abi.RPT_FLAG_PERSISTENT | FLAG, VH.PERSISTENT),
    ("persistent", _abi.RPT_FLAG_PERSISTENT, VH.PERSISTENT),
]


@pytest.mark.parametrize("seeded", [False, True], ids=["strided", "seeds"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(OTHER_ROWS)), ids=[r[0] for r in OTHER_ROWS])
def test_render_views_aov_refuses_the_flag(row, device, seeded):
    _, flags, detail = OTHER_ROWS[row]
    lib = _abi.load_library()
    n_pix = 2 * 4  # two views of 2 x 2
    outs = {"hits": np.full(n_pix, 7, dtype=np.uint32), "depth": np.full(n_pix, 7.0), "normal": np.full(3 * n_pix, 7.0),
            "albedo": np.full(3 * n_pix, 7.0), "position": np.full(3 * n_pix, 7.0), "object": np.full(n_pix, 7, dtype=np.int32)}
    q = HH.view_query(flags=flags)
    b = _abi.RptAovBuffers()
    b.struct_size, b.channels = C.sizeof(_abi.RptAovBuffers), _abi.RPT_AOV_ALL
    types = dict(_abi.RptAovBuffers._fields_)
    for name, a in outs.items():
        setattr(b, name, a.ctypes.data_as(types[name]))
    arr = (_abi.RptView * 2)(HH._view(), HH._view())
    seeds = (C.c_uint64 * 2)(*SEEDS)
    HH._another_detail_first(lib)
    head = (None, 2, arr, C.byref(q)) + ((seeds,) if seeded else ())
    name = "rptgpu_render_views_aov" + ("_seeded" if seeded else "") + ("_device" if device else "")
    rc = getattr(lib, name)(*head, C.byref(b), *((None,) if device else ()))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert all((a == 7).all() for a in outs.values())


@pytest.mark.parametrize("seeded", [False, True], ids=["strided", "seeds"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(OTHER_ROWS)), ids=[r[0] for r in OTHER_ROWS])
def test_render_views_denoised_refuses_the_flag(row, device, seeded):
    _, flags, detail = OTHER_ROWS[row]
    lib = _abi.load_library()
    q = VH._query(flags=flags)
    arr = (_abi.RptView * 2)(VH._view(), VH._view())
    d = DH._denoise()
    outs = {"denoised": np.full(2 * 5 * 3 * 3, 7.0), "rgb8": np.full(2 * 5 * 3 * 3, 7, dtype=np.uint8),
            "mean": np.full(2 * 5 * 3 * 3, 7.0), "variance": np.full(2 * 5 * 3, 7.0)}
    o = _abi.RptViewDenoiseOut()
    o.struct_size = C.sizeof(_abi.RptViewDenoiseOut)
    types = dict(_abi.RptViewDenoiseOut._fields_)
    for name, a in outs.items():
        setattr(o, name, a.ctypes.data_as(types[name]))
    seeds = (C.c_uint64 * 2)(*SEEDS) if seeded else None
    HH._another_detail_first(lib)
    args = (None, 2, arr, C.byref(q), seeds, C.byref(d), C.byref(o))
    rc = lib.rptgpu_render_views_denoised_device(*args, None) if device else lib.rptgpu_render_views_denoised(*args)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert all((a == 7).all() for a in outs.values())


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never frames from the host; and
    GpuScene.render_views carries the flag to the library (a recorder in its place)."""
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = HH.Recorder(), C.c_void_p(0x1234), 0
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    views = [camera, View.orthographic(camera, 2.0), View.panorama((0.0, 0.0, 5.0))]
    g.render_views(views, 9, 5, 2, flags=FLAG | _abi.RPT_FLAG_PROFILE_KERNELS)
    name, args = g.lib.calls.pop()
    assert name == "rptgpu_render_views" and args[3]._obj.flags == FLAG | _abi.RPT_FLAG_PROFILE_KERNELS
    g.render_views(views, 9, 5, 2, flags=FLAG, seeds=[1, 2, 3])
    name, args = g.lib.calls.pop()
    assert name == "rptgpu_render_views_seeded" and args[3]._obj.flags == FLAG
    g.handle = None
    if gpu_available:
        out = rpt_amd.GpuScene(scene).render_views(views, 9, 5, 2, samples=2, flags=FLAG)
        assert out.shape == (3, 5, 9, 3) and np.isfinite(out).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).render_views(views, 9, 5, 2, samples=2, flags=FLAG)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("views_items") / "views_items_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(VH.ROOT, "tests", "cpp", "views_items_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover", "edge"])
def test_views_items(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
