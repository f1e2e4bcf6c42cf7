"""rptgpu_render_views_aov on the GPU: rptgpu_render_aov's sums for every view of a batch.  Every comparison is on bits
(aov_model.mismatches: f64 as uint64, hits and object as they are).

A perspective view has a reference inside the library: rptgpu_render_aov of its camera over the full frame with the view's
seed.  The two other projections have none, but the contract gives one: the rays of tests/views_model.py (the header's
formulas in numpy, their sines and cosines evaluated on the device) through GpuScene.closest_hit, folded per pixel by
aov_model.fold in ascending sample order.  The rest is the contract's last sentence: a view's buffers are its own.  Scenes,
sizes and views are test_gpu_views': cornell and wine_glass at 37 x 21, glass at 33 x 23, three samples from sample 5 on."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import _abi, make_params

import aov_model
import small_scenes
import test_gpu_views as views_test
import views_model as M

pytestmark = pytest.mark.gpu

SCENES = ["cornell", "glass", "wine_glass"]
SIZES, SPP, BASE = views_test.SIZES, views_test.SPP, views_test.BASE
gpu, cameras, other_views = views_test.gpu, views_test.cameras, views_test.other_views
NAMES = ("hits", "object") + aov_model.CHANNELS


def render(g, name, views, **kw):
    w, h = SIZES[name]
    kw.setdefault("samples", SPP)
    kw.setdefault("seed", small_scenes.small(name)[2].seed)
    kw.setdefault("sample_index_base", BASE)
    return g.render_views_aov(views, w, h, **kw)


def view_of(aov, v):
    return {k: a[v] for k, a in aov.items()}


@functools.lru_cache(maxsize=None)
def mixed(name, stride):
    """(views, their buffers): every projection, the lens, and a second perspective view — computed once, never written to"""
    plain, beside, lens, L = cameras(name)
    views = (lens,) + other_views(name) + (beside,)
    out = render(gpu(name), name, views, seed_stride=stride)
    for a in out.values():
        a.setflags(write=False)
    return views, out


# ---- 1. a perspective view is render_aov
@pytest.mark.parametrize("stride", [0, 7])
@pytest.mark.parametrize("name", SCENES)
def test_a_perspective_view_is_render_aov(name, stride):
    """three cameras, one under a lens: view v == rptgpu_render_aov of its camera with seed + v * seed_stride, in every
    channel including hits and object"""
    w, h = SIZES[name]
    p0 = small_scenes.small(name)[2]
    g = gpu(name)
    views = cameras(name)[:3]
    got = render(g, name, views, seed_stride=stride)
    assert sorted(got) == sorted(NAMES)
    assert got["hits"].shape == (3, h, w) and got["hits"].dtype == np.uint32 and got["object"].dtype == np.int32
    assert got["depth"].shape == (3, h, w) and got["position"].shape == (3, h, w, 3)
    for v, cam in enumerate(views):
        p = make_params(w, h, p0.max_bounces, SPP, seed=p0.seed + v * stride, sample_index_base=BASE)
        want = g.render_aov(cam, p)
        assert aov_model.mismatches(view_of(got, v), want) == [], v
    assert got["hits"].max() == SPP and (got["hits"] < SPP).any()  # hits and misses
    assert aov_model.mismatches(view_of(got, 0), view_of(got, 2)) != []  # (the lens does something)


# ---- 2. the two other projections are the header's rays through closest_hit, folded
@pytest.mark.parametrize("name", SCENES)
def test_orthographic_and_panorama_are_the_headers_rays_folded(name, oracle):
    w, h = SIZES[name]
    scene, _, p0 = small_scenes.small(name)
    g = gpu(name)
    ortho, pano = other_views(name)
    seed, stride = p0.seed, 7
    got = render(g, name, (ortho, pano), seed_stride=stride)
    col = aov_model.colors(scene)
    n = w * h
    for v, view in enumerate((ortho, pano)):
        o, d = np.empty((n, SPP, 3)), np.empty((n, SPP, 3))
        for k, s in enumerate(range(BASE, BASE + SPP)):
            if view is ortho:
                o[:, k], d[:, k] = M.orthographic_rays(oracle, view.camera, view.ortho_scale, seed + v * stride, w, h, s)
            else:
                o[:, k], d[:, k] = M.panorama_rays(oracle, view.camera.eye, seed + v * stride, w, h, s, M.device_sincos(g))[:2]
        t, nrm, obj = g.closest_hit(o.reshape(-1, 3), d.reshape(-1, 3))
        t, nrm, obj = t.reshape(n, SPP), nrm.reshape(n, SPP, 3), obj.reshape(n, SPP)
        want = {"hits": np.zeros(n, dtype=np.uint32), "depth": np.zeros(n), "normal": np.zeros((n, 3)), "albedo": np.zeros((n, 3)),
                "position": np.zeros((n, 3)), "object": np.zeros(n, dtype=np.int32)}
        with np.errstate(all="ignore"):
            for j in range(n):
                (want["hits"][j], want["depth"][j], want["normal"][j], want["albedo"][j], want["position"][j],
                 want["object"][j]) = aov_model.fold(o[j], d[j], t[j], nrm[j], obj[j], col)
        mine = {k: a[v].reshape(want[k].shape) for k, a in got.items()}
        assert aov_model.mismatches(mine, want) == [], ("orthographic", "panorama")[v]
        assert 0 < want["hits"].sum() and (want["object"] >= 0).any()  # (they do see something)


# ---- 3. a view's buffers are its own
@pytest.mark.parametrize("stride", [0, 7])
@pytest.mark.parametrize("name", SCENES)
def test_a_views_buffers_are_its_own(name, stride, monkeypatch):
    g = gpu(name)
    views, base = mixed(name, stride)
    # pieces of 500 indices: they end inside a view and — the views' seeds being one — straddle view boundaries
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "500")
    assert aov_model.mismatches(render(g, name, views, seed_stride=stride), base) == []
    seed = small_scenes.small(name)[2].seed
    for v, view in enumerate(views):  # every view alone, with the seed it had in the batch
        alone = render(g, name, [view], seed=seed + v * stride)
        assert aov_model.mismatches(view_of(alone, 0), view_of(base, v)) == [], v
    if not stride:  # reordered (with a stride the seeds would move with the places: the views alone cover that)
        back = render(g, name, views[::-1])
        assert aov_model.mismatches({k: a[::-1] for k, a in back.items()}, base) == []
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    for v, view in enumerate(views):
        alone = render(g, name, [view], seed=seed + v * stride)
        assert aov_model.mismatches(view_of(alone, 0), view_of(base, v)) == [], v


# ---- 4. device arrays; 5. the flag
@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_device_arrays_channels_and_flags(name, monkeypatch):
    g = gpu(name)
    views, base = mixed(name, 7)
    dev = torch.device("cuda", 0)
    got = render(g, name, views, seed_stride=7, out="torch")
    assert all(isinstance(t, torch.Tensor) and t.device == dev for t in got.values())
    host = {k: t.cpu().numpy().view(base[k].dtype) for k, t in got.items()}
    assert aov_model.mismatches(host, base) == []
    # a channel that is not named is not written: through the ABI with EVERY pointer set and a sentinel in every array
    shape = base["hits"].shape
    full = {"hits": torch.full(shape, 7, dtype=torch.int32, device=dev), "object": torch.full(shape, 7, dtype=torch.int32, device=dev),
            "depth": torch.full(shape, 7.0, dtype=torch.float64, device=dev)}
    for k in ("normal", "albedo", "position"):
        full[k] = torch.full(shape + (3,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    w, h = SIZES[name]
    q = _abi.RptViewQuery()
    q.struct_size, q.width, q.height, q.iterations = _abi.C.sizeof(q), w, h, SPP
    q.seed, q.seed_stride, q.sample_index_base = small_scenes.small(name)[2].seed, 7, BASE
    b = _abi.RptAovBuffers()
    b.struct_size, b.channels = _abi.C.sizeof(b), _abi.RPT_AOV_DEPTH | _abi.RPT_AOV_ALBEDO
    types = dict(_abi.RptAovBuffers._fields_)
    for k, t in full.items():
        setattr(b, k, _abi.C.cast(_abi.C.c_void_p(t.data_ptr()), types[k]))
    arr = g._lower_views(list(views), "test")
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "500")
    _abi.check(g.lib.rptgpu_render_views_aov_device(g.handle, len(views), arr, _abi.C.byref(q), _abi.C.byref(b), None), g.handle)
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    back = {k: t.cpu().numpy() for k, t in full.items()}
    assert aov_model.mismatches({"hits": back["hits"].view(np.uint32), "depth": back["depth"], "albedo": back["albedo"]},
                                {k: base[k] for k in ("hits", "depth", "albedo")}) == []
    assert (back["object"] == 7).all() and (back["normal"] == 7.0).all() and (back["position"] == 7.0).all()
    # the Python method with two channels, into tensors of the caller's own, on a stream of the caller's own
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        mine = {"hits": torch.zeros(shape, dtype=torch.int32, device=dev), "object": torch.zeros(shape, dtype=torch.int32, device=dev)}
        ret = render(g, name, views, seed_stride=7, channels=_abi.RPT_AOV_OBJECT, out=mine)
        assert ret["object"] is mine["object"] and np.array_equal(mine["object"].cpu().numpy(), base["object"])
    # RPT_FLAG_GENERAL_TRAVERSAL changes no bit
    assert aov_model.mismatches(render(g, name, views, seed_stride=7, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL), base) == []
    hits_only = render(g, name, views, seed_stride=7, channels=0)
    assert sorted(hits_only) == ["hits"] and np.array_equal(hits_only["hits"], base["hits"])


def test_one_channel_of_a_host_caller_in_pieces_of_three(monkeypatch):
    """a view of 7 x 1 pixels in pieces of 3 — the last holds one —, NORMAL alone (not the first channel, three components),
    against the same view in one piece with every channel: a wrong staging offset, component count or row of the channel
    table shows"""
    name = "cornell"
    g = gpu(name)
    view = cameras(name)[0]
    kw = dict(samples=SPP, seed=small_scenes.small(name)[2].seed, sample_index_base=BASE)
    whole = g.render_views_aov([view], 7, 1, **kw)
    assert whole["hits"].max() > 0
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "3")
    got = g.render_views_aov([view], 7, 1, channels=_abi.RPT_AOV_NORMAL, **kw)
    assert aov_model.mismatches({k: got[k] for k in ("hits", "normal")}, {k: whole[k] for k in ("hits", "normal")}) == []


def test_nothing_to_do_and_refusals_on_a_live_handle():
    name = "cornell"
    w, h = SIZES[name]
    g = gpu(name)
    plain, beside, lens, L = cameras(name)
    assert render(g, name, [])["hits"].shape == (0, h, w)
    assert render(g, name, [], out="torch")["depth"].shape == (0, h, w)
    for views, kw, word in (((plain, beside), dict(flags=_abi.RPT_FLAG_PERSISTENT), "RPT_FLAG_PERSISTENT"),
                            ((plain, beside), dict(samples=0), "must be non-zero"),
                            ((plain, beside), dict(channels=32), "unknown RPT_AOV_"),
                            ((plain, rpt_amd.View.orthographic(lens, 1.0)), {}, "only RPT_VIEW_PERSPECTIVE has a lens"),
                            ((rpt_amd.View(plain, 9), plain), {}, "unknown projection")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            render(g, name, views, **kw)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
    views, base = mixed(name, 0)
    assert aov_model.mismatches(render(g, name, views), base) == []  # the handle is as good as before
