"""rptgpu_render_views_seeded / rptgpu_render_views_aov_seeded (and their _device forms) without a GPU: the four symbols,
every refusal that comes before the device — all of the unseeded calls', and NULL seeds — with its code and detail and
untouched outputs, no CPU fallback, and what GpuScene.render_views(seeds=...) / render_views_aov(seeds=...) lower to."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import Camera, View, _abi

import test_first_hits_host as HH
import test_views_host as VH

E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_render_views_seeded", "rptgpu_render_views_seeded_device", "rptgpu_render_views_aov_seeded",
         "rptgpu_render_views_aov_seeded_device")
NULL_SEEDS = b"null seeds: the _seeded entry points take one seed per view"
SEEDS = (5, (1 << 63) + 1)


def test_the_four_symbols_exist(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES)
    assert set(NAMES) == {s[0] for s in _abi.SEEDED_SYMBOLS} and not set(NAMES) & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    # declared in the header of the optional additions, which rpt_gpu.h includes: one #include gives a C caller all of them
    header = open(VH.ROOT + "/include/rpt_gpu_views_seeded.h").read()
    assert all("int %s(" % n in header for n in NAMES)
    assert '#include "rpt_gpu_views_seeded.h"' in open(VH.ROOT + "/include/rpt_gpu.h").read()
    src = '#include "rpt_gpu.h"\nint main(void){return %s;}' % " && ".join("%s != 0" % n for n in NAMES)
    c = tmp_path / "seeded.c"
    c.write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wno-address", "-I", VH.ROOT + "/include", str(c)])


# everything rptgpu_render_views refuses (tests/test_views_host.py's rows, seeds given), then the seeds: NULL with views to
# render is refused behind the other NULL arguments and in front of the views' own checks; without views it is not read
VIEWS_ROWS = [r + (True,) for r in VH.REFUSALS] + [
    ("no seeds", dict(), NULL_SEEDS, False),
    ("no seeds, a bad view behind them", dict(views=[VH._view(), VH._view(3)]), NULL_SEEDS, False),
    ("no seeds, persistent", dict(q=VH._query(flags=_abi.RPT_FLAG_PERSISTENT)), VH.PERSISTENT, False),
    ("no seeds, no views pointer", dict(views=False), b"null argument", False),
    ("handle, no views, no seeds", dict(n=0, views=False, out=False), b"null handle", False),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(VIEWS_ROWS)), ids=[r[0] for r in VIEWS_ROWS])
def test_render_views_seeded_refuses_before_the_device(row, device):
    _, kw, detail, with_seeds = VIEWS_ROWS[row]
    lib = _abi.load_library()
    q = kw.get("q", VH._query())
    views = kw.get("views", [VH._view(), VH._view()])
    arr = (_abi.RptView * 2)(*views) if views else None
    keep = bytes(arr) if arr is not None else None
    out = np.full(2 * 5 * 3 * 3, 7.0) if kw.get("out", True) else None
    seeds = (C.c_uint64 * 2)(*SEEDS) if with_seeds else None
    n = kw.get("n", 2)
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    qp = C.byref(q) if q is not None else None
    if device:
        rc = lib.rptgpu_render_views_seeded_device(None, n, arr, qp, seeds, C.c_void_p(out.ctypes.data) if out is not None else None,
                                                   0, None)
    else:
        rc = lib.rptgpu_render_views_seeded(None, n, arr, qp, seeds, out.ctypes.data_as(PD) if out is not None else None)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert out is None or (out == 7).all()
    assert arr is None or bytes(arr) == keep
    assert seeds is None or tuple(seeds) == SEEDS


AOV_ROWS = [r + (True,) for r in HH.VIEWS_REFUSALS] + [
    ("no seeds", dict(), NULL_SEEDS, False),
    ("no seeds, a bad view behind them", dict(views=[HH._view(), HH._view(projection=3)]), NULL_SEEDS, False),
    ("no seeds, persistent", dict(q=HH.view_query(flags=_abi.RPT_FLAG_PERSISTENT)), HH.VIEWS_PERSISTENT, False),
    ("no seeds, no buffers struct", dict(buffers=None), b"null RptAovBuffers", False),
    ("handle, no views, no seeds", dict(n=0, views=None), b"null handle", False),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(AOV_ROWS)), ids=[r[0] for r in AOV_ROWS])
def test_render_views_aov_seeded_refuses_before_the_device(row, device):
    _, kw, detail, with_seeds = AOV_ROWS[row]
    lib = _abi.load_library()
    n_pix = 2 * 4  # two views of 2 x 2
    outs = {"hits": np.full(n_pix, 7, dtype=np.uint32), "depth": np.full(n_pix, 7.0), "normal": np.full(3 * n_pix, 7.0),
            "albedo": np.full(3 * n_pix, 7.0), "position": np.full(3 * n_pix, 7.0), "object": np.full(n_pix, 7, dtype=np.int32)}
    q = kw.get("q", HH.view_query())
    b = _abi.RptAovBuffers()
    b.struct_size, b.channels = kw.get("b_size", C.sizeof(_abi.RptAovBuffers)), kw.get("channels", _abi.RPT_AOV_ALL)
    types = dict(_abi.RptAovBuffers._fields_)
    for name, a in outs.items():
        if kw.get(name, True):
            setattr(b, name, a.ctypes.data_as(types[name]))
    views = kw.get("views", [HH._view(), HH._view()])
    arr = (_abi.RptView * 2)(*views) if views is not None else None
    bp = C.byref(b) if kw.get("buffers", True) is not None else None
    qp = C.byref(q) if q is not None else None
    seeds = (C.c_uint64 * 2)(*SEEDS) if with_seeds else None
    HH._another_detail_first(lib)
    if device:
        rc = lib.rptgpu_render_views_aov_seeded_device(None, kw.get("n", 2), arr, qp, seeds, bp, None)
    else:
        rc = lib.rptgpu_render_views_aov_seeded(None, kw.get("n", 2), arr, qp, seeds, bp)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert all((a == 7).all() for a in outs.values())


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never frames from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    views = [camera, View.orthographic(camera, 2.0), View.panorama((0.0, 0.0, 5.0))]
    seeds = (5, (1 << 63) + 1, 5)
    if gpu_available:
        g = rpt_amd.GpuScene(scene)
        out = g.render_views(views, 9, 5, 2, samples=2, seeds=seeds)
        assert out.shape == (3, 5, 9, 3) and np.isfinite(out).all()
        assert g.render_views_aov(views, 9, 5, samples=2, seeds=seeds)["hits"].shape == (3, 5, 9)
        return
    for call in (lambda g: g.render_views(views, 9, 5, 2, samples=2, seeds=seeds),
                 lambda g: g.render_views_aov(views, 9, 5, samples=2, seeds=seeds)):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call(rpt_amd.GpuScene(scene))
        assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


def test_what_the_python_calls_lower_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # a recorder in the library's place: nothing here reaches a device
    g.lib, g.handle, g.device = HH.Recorder(), C.c_void_p(0x1234), 0
    cam = Camera((0.0, 1.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.8, 0.0, 0.0)
    views = [cam, View.orthographic(cam, 2.5), View.panorama((1.0, 2.0, 3.0))]
    seeds = [5, (1 << 63) + 1, 5]
    for given in (seeds, tuple(seeds), np.array(seeds, dtype=np.uint64), iter(seeds)):
        out = g.render_views(views, 7, 4, 3, samples=2, seed=11, sample_index_base=9, exposure_value=0.5, seeds=given,
                             flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
        name, (h, n, arr, q, s, po) = g.lib.calls.pop()
        q = q._obj
        assert name == "rptgpu_render_views_seeded" and h is g.handle and n == 3
        assert isinstance(s, C.Array) and s._type_ is C.c_uint64 and list(s) == seeds
        assert [arr[i].projection for i in range(3)] == [_abi.RPT_VIEW_PERSPECTIVE, _abi.RPT_VIEW_ORTHOGRAPHIC, _abi.RPT_VIEW_PANORAMA]
        assert (q.struct_size, q.width, q.height, q.max_bounces, q.iterations) == (64, 7, 4, 3, 2)
        assert (q.seed_stride, q.sample_index_base, q.exposure_value, q.flags) == (0, 9, 0.5, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
        assert out.shape == (3, 4, 7, 3) and HH._address(po) == out.ctypes.data
    # without seeds the call is the one it was
    g.render_views(views, 7, 4, 3, seed=11, seed_stride=5)
    name, args = g.lib.calls.pop()
    assert name == "rptgpu_render_views" and len(args) == 5 and (args[3]._obj.seed, args[3]._obj.seed_stride) == (11, 5)
    # no views: no seeds either, and still an array with an address
    assert g.render_views([], 7, 4, 3, seeds=[]).shape == (0, 4, 7, 3)
    name, (h, n, arr, q, s, po) = g.lib.calls.pop()
    assert name == "rptgpu_render_views_seeded" and n == 0 and len(s) == 1

    aov = g.render_views_aov(views, 5, 4, samples=3, sample_index_base=1 << 40, channels=_abi.RPT_AOV_DEPTH, seeds=seeds)
    name, (h, n, arr, q, s, b) = g.lib.calls.pop()
    assert name == "rptgpu_render_views_aov_seeded" and h is g.handle and n == 3 and list(s) == seeds
    assert (q._obj.iterations, q._obj.seed_stride, q._obj.sample_index_base) == (3, 0, 1 << 40)
    assert b._obj.channels == _abi.RPT_AOV_DEPTH and HH._address(b._obj.depth) == aov["depth"].ctypes.data
    g.render_views_aov(views, 5, 4, seed=3, seed_stride=2)
    name, args = g.lib.calls.pop()
    assert name == "rptgpu_render_views_aov" and len(args) == 5
    assert not g.lib.calls

    # the wrapper's own checks: nothing reaches the library
    for call, who in ((lambda **kw: g.render_views(views, 7, 4, 3, **kw), "render_views"),
                      (lambda **kw: g.render_views_aov(views, 7, 4, **kw), "render_views_aov")):
        with pytest.raises(ValueError, match="%s: 2 seeds for 3 views" % who):
            call(seeds=seeds[:2])
        with pytest.raises(ValueError, match="%s: 4 seeds for 3 views" % who):
            call(seeds=seeds + [1])
        with pytest.raises(ValueError, match="exclude each other"):
            call(seeds=seeds, seed_stride=1)
        with pytest.raises(ValueError, match="must be uint64"):
            call(seeds=np.array([1, 2, 3], dtype=np.int64))
        with pytest.raises(ValueError, match="64 bits"):
            call(seeds=[1, 2, 1 << 64])
        with pytest.raises(ValueError, match="64 bits"):
            call(seeds=[1, -2, 3])
        call(seeds=seeds, seed_stride=0)  # a stride of zero says nothing
        g.lib.calls.pop()
    assert not g.lib.calls
    g.handle = None
