"""rptgpu_render_views_denoised (and its _device form) without a GPU: the two symbols and the layouts of RptViewDenoise /
RptViewDenoiseOut against the header, every refusal that comes before the device — all of rptgpu_render_views', then the
denoise struct's, the outputs' and the batch's own — with its code and detail and untouched outputs, no CPU fallback, what
GpuScene.render_views_denoised lowers to, and the driver's host-only planning (rpt_amd/csrc/render_plan.h
views_denoise_plan, sample_range_fits) as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import Camera, View, _abi

import test_first_hits_host as HH
import test_views_host as VH

E = _abi.RPTGPU_E_INVALID_ARGUMENT
ROOT = VH.ROOT
NAMES = ("rptgpu_render_views_denoised", "rptgpu_render_views_denoised_device")
D_FIELDS = ("struct_size", "batches", "feature_iterations", "_pad", "feature_sample_index_base", "filter")
O_FIELDS = ("struct_size", "_pad", "denoised", "rgb8", "mean", "variance")
SEEDS = (5, (1 << 63) + 1)


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES)
    assert set(NAMES) == {s[0] for s in _abi.DENOISED_SYMBOLS}
    assert not set(NAMES) & {s[0] for s in _abi.SYMBOLS + _abi.SEEDED_SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    header = open(ROOT + "/include/rpt_gpu_views_denoised.h").read()
    assert all("int %s(" % n in header for n in NAMES)
    assert '#include "rpt_gpu_views_denoised.h"' in open(ROOT + "/include/rpt_gpu.h").read()
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){' \
          'printf("%zu %zu", sizeof(RptViewDenoise), sizeof(RptViewDenoiseOut));' + \
          "".join('printf(" %%zu", offsetof(RptViewDenoise, %s));' % f for f in D_FIELDS) + \
          "".join('printf(" %%zu", offsetof(RptViewDenoiseOut, %s));' % f for f in O_FIELDS) + \
          "return 0;}"
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # one #include gives a C caller both declarations
    c.write_text('#include "rpt_gpu.h"\nint main(void){return %s;}' % " && ".join("%s != 0" % n for n in NAMES))
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wno-address", "-I", os.path.join(ROOT, "include"), str(c)])
    assert C.sizeof(_abi.RptViewDenoise) == nums[0] == 64 and C.sizeof(_abi.RptViewDenoiseOut) == nums[1] == 40
    assert [getattr(_abi.RptViewDenoise, f).offset for f in D_FIELDS] == nums[2:2 + len(D_FIELDS)]
    assert [getattr(_abi.RptViewDenoiseOut, f).offset for f in O_FIELDS] == nums[2 + len(D_FIELDS):]
    assert [f for f, _ in _abi.RptViewDenoise._fields_] == list(D_FIELDS)
    assert [f for f, _ in _abi.RptViewDenoiseOut._fields_] == list(O_FIELDS)


def _denoise(**kw):
    d = _abi.RptViewDenoise()
    d.struct_size, d.batches, d.feature_iterations = C.sizeof(_abi.RptViewDenoise), 3, 2
    d.filter = _abi.RptDenoise(C.sizeof(_abi.RptDenoise), 3, 2.0, 0.1, 0.01, 0.1)
    for k, v in kw.items():
        if k in ("levels", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"):
            setattr(d.filter, k, v)
        elif k == "filter_size":
            d.filter.struct_size = v
        else:
            setattr(d, k, v)
    return d


D_SIZE = b"RptViewDenoise: struct_size is not sizeof(RptViewDenoise)"
O_SIZE = b"RptViewDenoiseOut: struct_size is not sizeof(RptViewDenoiseOut)"
F_SIZE = b"RptDenoise: struct_size is not sizeof(RptDenoise)"
LEVELS = b"RptDenoise: levels outside 1..8"
SIGMA = b"RptDenoise: every sigma must be finite and > 0"
BATCHES = b"RptViewDenoise: batches < 2 (there is no variance of one batch)"
BOTH = b"RptViewDenoiseOut: denoised and rgb8 are both NULL"
TOO_MANY = b"n_views * width * height > 2^32 - 1: the batches are accumulated over 32-bit indices"
RANGE = b"sample_index_base + batches * iterations does not fit 64 bits"
F_RANGE = b"feature_sample_index_base + feature_iterations does not fit 64 bits"
M64 = (1 << 64) - 1
# rptgpu_render_views' own rows with a denoise struct attached (tests/test_views_host.py; its `out` is the struct here, and a
# NULL struct is refused whatever n_views is, as rptgpu_render_views_aov refuses a NULL RptAovBuffers) ...
VIEWS_ROWS = [(name, dict(o=None), b"null RptViewDenoiseOut") if name == "out" else
              (name, {k: v for k, v in kw.items() if k != "out"}, detail) for name, kw, detail in VH.REFUSALS]
# ... and this call's: d = the RptViewDenoise (None: NULL), o_size / want = the RptViewDenoiseOut's size and non-NULL arrays
OWN_ROWS = [
    ("no denoise", dict(d=None), b"null RptViewDenoise"),
    ("denoise size 0", dict(d=_denoise(struct_size=0)), D_SIZE),
    ("denoise size 56", dict(d=_denoise(struct_size=56)), D_SIZE),
    ("denoise size 72", dict(d=_denoise(struct_size=72)), D_SIZE),
    ("batches 0", dict(d=_denoise(batches=0)), BATCHES),
    ("batches 1", dict(d=_denoise(batches=1)), BATCHES),
    ("feature_iterations 0", dict(d=_denoise(feature_iterations=0)), b"RptViewDenoise: feature_iterations == 0"),
    ("filter size 0", dict(d=_denoise(filter_size=0)), F_SIZE),
    ("filter size 48", dict(d=_denoise(filter_size=48)), F_SIZE),
    ("levels 0", dict(d=_denoise(levels=0)), LEVELS),
    ("levels 9", dict(d=_denoise(levels=9)), LEVELS),
    ("sigma_color 0", dict(d=_denoise(sigma_color=0.0)), SIGMA),
    ("sigma_normal < 0", dict(d=_denoise(sigma_normal=-0.1)), SIGMA),
    ("sigma_depth inf", dict(d=_denoise(sigma_depth=math.inf)), SIGMA),
    ("sigma_albedo nan", dict(d=_denoise(sigma_albedo=math.nan)), SIGMA),
    ("a bad query before a bad denoise", dict(q=VH._query(iterations=0), d=_denoise(batches=1)), VH.ZERO),
    ("a bad denoise before a bad view", dict(d=_denoise(batches=1), views=[VH._view(), VH._view(3)]), BATCHES),
    ("no outputs struct", dict(o=None), b"null RptViewDenoiseOut"),
    ("no outputs struct, no views", dict(o=None, n=0, views=False), b"null RptViewDenoiseOut"),
    ("outputs size 0", dict(o_size=0), O_SIZE),
    ("outputs size 32", dict(o_size=32), O_SIZE),
    ("outputs size 48", dict(o_size=48), O_SIZE),
    ("no output", dict(want=()), BOTH),
    ("mean and variance alone", dict(want=("mean", "variance")), BOTH),
    ("a bad denoise before the outputs", dict(d=_denoise(levels=9), want=()), LEVELS),
    ("the outputs before a NULL views", dict(want=("mean",), views=False), BOTH),
    ("2^32 indices", dict(q=VH._query(width=1 << 15, height=1 << 15), n=4), TOO_MANY),
    ("2^32 indices in one view", dict(q=VH._query(width=1 << 16, height=1 << 16), n=1), TOO_MANY),
    ("2^32 - 1 indices: the handle is next", dict(q=VH._query(width=65535, height=65537), n=1), b"null handle"),
    ("2^40 views", dict(n=1 << 40), TOO_MANY),
    ("sample range", dict(q=VH._query(sample_index_base=M64 - 10)), RANGE),  # 3 batches of 4: the last index is 2^64
    ("sample range, the last index fits", dict(q=VH._query(sample_index_base=M64 - 11)), b"null handle"),
    ("feature range", dict(d=_denoise(feature_sample_index_base=M64)), F_RANGE),
    ("feature range, the last index fits", dict(d=_denoise(feature_sample_index_base=M64 - 1)), b"null handle"),
    ("ranges before a bad view", dict(d=_denoise(feature_sample_index_base=M64), views=[VH._view(3), VH._view()]), F_RANGE),
    ("mean beside rgb8", dict(want=("rgb8", "mean")), b"null handle"),
    ("handle, no views", dict(n=0, views=False), b"null handle"),
]
ROWS = VIEWS_ROWS + OWN_ROWS


@pytest.mark.parametrize("seeded", [False, True], ids=["strided", "seeds"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_every_refusal_comes_before_the_device(row, device, seeded):
    """... so each of them is there without a handle: code, detail, and nothing written"""
    _, kw, detail = ROWS[row]
    lib = _abi.load_library()
    q = kw.get("q", VH._query())
    views = kw.get("views", [VH._view(), VH._view()])
    arr = (_abi.RptView * 2)(*views) if views else None
    keep = bytes(arr) if arr is not None else None
    d = kw.get("d", _denoise())
    outs = {"denoised": np.full(2 * 5 * 3 * 3, 7.0), "rgb8": np.full(2 * 5 * 3 * 3, 7, dtype=np.uint8),
            "mean": np.full(2 * 5 * 3 * 3, 7.0), "variance": np.full(2 * 5 * 3, 7.0)}
    o = _abi.RptViewDenoiseOut()
    o.struct_size = kw.get("o_size", C.sizeof(_abi.RptViewDenoiseOut))
    types = dict(_abi.RptViewDenoiseOut._fields_)
    for name in kw.get("want", ("denoised", "rgb8", "mean", "variance")):
        setattr(o, name, outs[name].ctypes.data_as(types[name]))
    seeds = (C.c_uint64 * 2)(*SEEDS) if seeded else None
    HH._another_detail_first(lib)
    args = (None, kw.get("n", 2), arr, C.byref(q) if q is not None else None, seeds, C.byref(d) if d is not None else None,
            C.byref(o) if kw.get("o", True) is not None else None)
    rc = lib.rptgpu_render_views_denoised_device(*args, None) if device else lib.rptgpu_render_views_denoised(*args)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert all((a == 7).all() for a in outs.values())
    assert arr is None or bytes(arr) == keep
    assert seeds is None or tuple(seeds) == SEEDS


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never frames from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    views = [camera, View.orthographic(camera, 2.0), View.panorama((0.0, 0.0, 5.0))]
    if gpu_available:
        g = rpt_amd.GpuScene(scene)
        out = g.render_views_denoised(views, 9, 5, 2, samples=2, batches=2, seeds=(5, (1 << 63) + 1, 5), want=("denoised", "rgb8"))
        assert out["denoised"].shape == (3, 5, 9, 3) and np.isfinite(out["denoised"]).all() and out["rgb8"].dtype == np.uint8
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).render_views_denoised(views, 9, 5, 2, samples=2, batches=2)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


def test_what_the_python_call_lowers_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # a recorder in the library's place: nothing here reaches a device
    g.lib, g.handle, g.device = HH.Recorder(), C.c_void_p(0x1234), 0
    cam = Camera((0.0, 1.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.8, 0.0, 0.0)
    views = [cam, View.orthographic(cam, 2.5), View.panorama((1.0, 2.0, 3.0))]
    seeds = [5, (1 << 63) + 1, 5]
    out = g.render_views_denoised(views, 7, 4, 3, 2, 5, seeds=seeds, sample_index_base=9, feature_samples=6,
                                  feature_sample_index_base=1 << 40, levels=4, sigma_color=1.5, sigma_normal=0.2, sigma_depth=0.3,
                                  sigma_albedo=0.4, exposure_value=0.5, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL,
                                  want=("denoised", "rgb8", "mean", "variance"))
    name, (h, n, arr, q, s, d, o) = g.lib.calls.pop()
    q, d, o = q._obj, d._obj, o._obj
    assert name == "rptgpu_render_views_denoised" and h is g.handle and n == 3 and list(s) == seeds
    assert [arr[i].projection for i in range(3)] == [_abi.RPT_VIEW_PERSPECTIVE, _abi.RPT_VIEW_ORTHOGRAPHIC, _abi.RPT_VIEW_PANORAMA]
    assert (q.struct_size, q.width, q.height, q.max_bounces, q.iterations) == (64, 7, 4, 3, 2)
    assert (q.seed_stride, q.sample_index_base, q.exposure_value, q.flags) == (0, 9, 0.5, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert (d.struct_size, d.batches, d.feature_iterations, d.feature_sample_index_base) == (64, 5, 6, 1 << 40)
    f = d.filter
    assert (f.struct_size, f.levels, f.sigma_color, f.sigma_normal, f.sigma_depth, f.sigma_albedo) == (40, 4, 1.5, 0.2, 0.3, 0.4)
    assert o.struct_size == 40 and sorted(out) == ["denoised", "mean", "rgb8", "variance"]
    assert out["denoised"].shape == out["mean"].shape == out["rgb8"].shape == (3, 4, 7, 3) and out["variance"].shape == (3, 4, 7)
    assert out["rgb8"].dtype == np.uint8 and out["variance"].dtype == np.float64
    assert all(HH._address(getattr(o, k)) == out[k].ctypes.data for k in out)
    # the defaults: Buffer.denoise's filter, four feature samples from sample 0, `denoised` alone, the query's seed and stride
    out = g.render_views_denoised(views, 7, 4, 3, samples=2, batches=3, seed=11, seed_stride=5)
    name, (h, n, arr, q, s, d, o) = g.lib.calls.pop()
    d, o, f = d._obj, o._obj, d._obj.filter
    assert s is None and (q._obj.seed, q._obj.seed_stride, q._obj.sample_index_base) == (11, 5, 0)
    assert (d.batches, d.feature_iterations, d.feature_sample_index_base) == (3, 4, 0)
    assert (f.levels, f.sigma_color, f.sigma_normal, f.sigma_depth, f.sigma_albedo) == (3, 2.0, 0.1, 0.01, 0.1)
    assert sorted(out) == ["denoised"] and HH._address(o.denoised) == out["denoised"].ctypes.data
    assert not o.rgb8 and not o.mean and not o.variance
    # the caller's own arrays are written where they lie
    mine = {"rgb8": np.zeros((3, 4, 7, 3), dtype=np.uint8), "variance": np.zeros((3, 4, 7))}
    got = g.render_views_denoised(views, 7, 4, 3, 2, 3, want=("rgb8", "variance"), out=mine)
    o = g.lib.calls.pop()[1][6]._obj
    assert got["rgb8"] is mine["rgb8"] and HH._address(o.rgb8) == mine["rgb8"].ctypes.data and not o.denoised
    # no views: still arrays with an address
    out = g.render_views_denoised([], 7, 4, 3, 2, 3, seeds=[])
    name, (h, n, arr, q, s, d, o) = g.lib.calls.pop()
    assert n == 0 and out["denoised"].shape == (0, 4, 7, 3) and HH._address(o._obj.denoised)
    assert not g.lib.calls

    # the wrapper's own checks: nothing reaches the library
    def call(**kw):
        return g.render_views_denoised(views, 7, 4, 3, 2, 3, **kw)
    with pytest.raises(ValueError, match="render_views_denoised: 2 seeds for 3 views"):
        call(seeds=seeds[:2])
    with pytest.raises(ValueError, match="exclude each other"):
        call(seeds=seeds, seed_stride=1)
    with pytest.raises(ValueError, match="must be uint64"):
        call(seeds=np.array([1, 2, 3], dtype=np.int64))
    with pytest.raises(ValueError, match="64 bits"):
        call(seeds=[1, 2, 1 << 64])
    with pytest.raises(ValueError, match="`denoised` or `rgb8`"):
        call(want=("mean",))
    with pytest.raises(ValueError, match="at most once"):
        call(want=("denoised", "depth"))
    with pytest.raises(ValueError, match="at most once"):
        call(want=("rgb8", "rgb8"))
    with pytest.raises(ValueError, match="exactly the keys"):
        call(want=("rgb8",), out=mine)
    with pytest.raises(ValueError, match="C-contiguous"):
        call(want=("rgb8", "variance"), out={"rgb8": mine["rgb8"], "variance": np.zeros((3, 4, 7), dtype=np.float32)})
    with pytest.raises(TypeError, match="view 1 is a int"):
        g.render_views_denoised([cam, 3], 7, 4, 3, 2, 3)
    assert not g.lib.calls
    g.handle = None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("views_denoise_plan") / "views_denoise_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "views_denoise_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["bound", "bytes", "ranges"])
def test_views_denoise_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
