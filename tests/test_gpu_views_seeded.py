"""Batches of views with a seed per view on the GPU: rptgpu_render_views_seeded / rptgpu_render_views_aov_seeded, and
rptgpu_render_views with a seed stride, which takes the same route.  Tolerance 0 (== on the f64 arrays, aov_model.mismatches
on the feature buffers) everywhere.

The seed travels with the path (rpt_raygen_views_seeded, rpt_shade_seeded), so a piece of consecutive (view, pixel) indices
spans views whatever their seeds.  What is checked: view v is what the unseeded call gives with seed = seeds[v] — a
perspective view against rptgpu_render_batch / rptgpu_render_aov (and the oracle), the two other projections against the
header's rays (tests/views_model.py) through trace_rays / closest_hit —, a view's result is its own whatever the pieces,
the order and the other views, and the launches of a depth are shared by views with different seeds.

Scenes, sizes and cameras are tests/test_gpu_views.py's: cornell and wine_glass at 37 x 21, glass at 33 x 23 (more than one
256-thread block per frame, an odd number of them); three samples from sample 5 on; three bounces."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

from rpt_amd import Camera, _abi, make_params

import aov_model
import small_scenes
import test_gpu_views as VT
import views_model as M

pytestmark = pytest.mark.gpu

SCENES = ["cornell", "glass", "wine_glass"]
SIZES, SPP, BASE = VT.SIZES, VT.SPP, VT.BASE
BOUNCES = 3
SEEDS = (5, 2 ** 63 + 1, 5)  # not an arithmetic sequence, one above 2^32 (and 2^63), one duplicate
gpu, cameras, other_views = VT.gpu, VT.cameras, VT.other_views


def three_views(name):
    """a perspective view under a lens, an orthographic view, a panorama"""
    return (cameras(name)[2],) + other_views(name)


def render(g, name, views, **kw):
    w, h = SIZES[name]
    kw.setdefault("samples", SPP)
    kw.setdefault("sample_index_base", BASE)
    return g.render_views(views, w, h, BOUNCES, **kw)


def render_aov(g, name, views, **kw):
    w, h = SIZES[name]
    kw.setdefault("samples", SPP)
    kw.setdefault("sample_index_base", BASE)
    return g.render_views_aov(views, w, h, **kw)


def params(name, seed, spp=SPP):
    w, h = SIZES[name]
    return make_params(w, h, BOUNCES, spp, seed=seed, sample_index_base=BASE)


@functools.lru_cache(maxsize=None)
def base(name):
    """the three views' frames under SEEDS, one piece — computed once, never written to"""
    out = render(gpu(name), name, three_views(name), seeds=SEEDS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def base_aov(name):
    out = render_aov(gpu(name), name, three_views(name), seeds=SEEDS)
    for a in out.values():
        a.setflags(write=False)
    return out


def view_of(aov, v):
    return {k: a[v] for k, a in aov.items()}


def pieces_that_span_two_seeds(name, piece):
    """pieces of `piece` consecutive indices j = v * npix + pixel of the three views that hold indices of two views whose
    seeds differ"""
    w, h = SIZES[name]
    npix = w * h
    spans = 0
    for first in range(0, 3 * npix, piece):
        last = min(first + piece, 3 * npix) - 1
        if SEEDS[first // npix] != SEEDS[last // npix]:
            spans += 1
    return spans


# ---- 1. a perspective view is render_batch with the view's seed
@pytest.mark.parametrize("name", SCENES)
def test_a_perspective_view_is_render_batch_with_its_seed(name, oracle):
    w, h = SIZES[name]
    scene = small_scenes.small(name)[0]
    g = gpu(name)
    views = cameras(name)[:3]  # the scene's camera, one from beside it, one under a lens
    g.reset_stats()
    got = render(g, name, views, seeds=SEEDS)
    st = g.stats()
    assert got.shape == (3, h, w, 3) and got.dtype == np.float64 and np.isfinite(got).all()
    assert st.samples == 3 * w * h * SPP and st.kernel_launches[_abi.RPT_K_PATHS] == 0  # wavefront only
    for v, cam in enumerate(views):
        p = params(name, SEEDS[v])
        want = g.render_batch(cam, p)
        assert (got[v].reshape(-1, 3) == want).all(), "view %d: %d pixels differ" % (v, (got[v].reshape(-1, 3) != want).any(axis=1).sum())
        if name == "cornell":
            assert (want == oracle.OracleScene(scene).render(cam, p)).all(), v
    # the lens among the other projections
    lens = cameras(name)[2]
    assert (base(name)[0].reshape(-1, 3) == g.render_batch(lens, params(name, SEEDS[0]))).all()
    assert not (got[0] == got[1]).all()


# ---- 2. the two other projections are the header's rays under the view's seed
@pytest.mark.parametrize("name", SCENES)
def test_orthographic_and_panorama_are_the_headers_rays_with_their_seeds(name, oracle):
    """per sample index the model's rays through trace_rays (streams = pixel, first_draw = 2, seed = seeds[v], one sample),
    folded in sample order from +0.0, / iterations"""
    w, h = SIZES[name]
    g = gpu(name)
    lens, ortho, pano = three_views(name)
    pixels = np.arange(w * h, dtype=np.uint32)
    got = base(name)
    for v, view in ((1, ortho), (2, pano)):
        seed = SEEDS[v]
        acc = np.zeros((w * h, 3))
        for s in range(BASE, BASE + SPP):
            if view is ortho:
                o, d = M.orthographic_rays(oracle, view.camera, view.ortho_scale, seed, w, h, s)
            else:
                o, d, _, _ = M.panorama_rays(oracle, view.camera.eye, seed, w, h, s, M.device_sincos(g))
            acc = acc + g.trace_rays(o, d, BOUNCES, samples=1, seed=seed, sample_index_base=s, streams=pixels, first_draw=2,
                                     exposure_value=0.0)
        want = acc / float(SPP)
        assert (got[v].reshape(-1, 3) == want).all(), "view %d: %d pixels differ" % (v, (got[v].reshape(-1, 3) != want).any(axis=1).sum())
        assert not (acc == acc[0]).all()  # (it does see something)


# ---- 3. a view's pixels are its own: pieces that span views with different seeds, the order, the other views
@pytest.mark.parametrize("name", SCENES)
def test_pieces_span_views_with_different_seeds(name, monkeypatch):
    w, h = SIZES[name]
    npix = w * h
    g = gpu(name)
    views = three_views(name)
    want = base(name)
    # a view is 777 or 759 indices: pieces of 100 begin and end inside views, and the two that hold a view's last and the
    # next view's first indices run paths of two seeds through one rpt_shade_seeded launch
    assert npix % 100 != 0 and (2 * npix) % 100 != 0 and npix // 100 != (2 * npix) // 100
    assert pieces_that_span_two_seeds(name, 100) == 2
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "100")
    g.reset_stats()
    assert (render(g, name, views, seeds=SEEDS) == want).all()
    st = g.stats()
    assert st.samples == 3 * npix * SPP
    assert st.kernel_launches[_abi.RPT_K_RAYGEN] >= (3 * npix + 99) // 100
    # the views and their seeds in reverse order
    assert (render(g, name, views[::-1], seeds=SEEDS[::-1]) == want[::-1]).all()
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    assert (render(g, name, views[::-1], seeds=SEEDS[::-1]) == want[::-1]).all()
    # every view alone: through the seeded call, and through the unseeded one with its seed
    for v, view in enumerate(views):
        assert (render(g, name, [view], seeds=[SEEDS[v]])[0] == want[v]).all(), v
        assert (render(g, name, [view], seed=SEEDS[v])[0] == want[v]).all(), v


@pytest.mark.parametrize("name", SCENES)
def test_equal_seeds_and_equal_cameras_give_equal_frames(name):
    lens, ortho, pano = three_views(name)
    got = render(gpu(name), name, (lens, ortho, lens), seeds=SEEDS)  # views 0 and 2: seed 5
    assert (got[0] == got[2]).all() and (got[0] == base(name)[0]).all() and (got[1] == base(name)[1]).all()
    other = render(gpu(name), name, (lens, lens), seeds=SEEDS[:2])
    assert (other[0] == got[0]).all() and not (other[1] == other[0]).all()  # (the seed does something)


# ---- 4. a seed stride is the seeded call with seed + v * stride, in wrapping u64 arithmetic
@pytest.mark.parametrize("name", SCENES)
def test_a_seed_stride_is_the_seeded_call(name, monkeypatch):
    g = gpu(name)
    views = three_views(name)
    strided = render(g, name, views, seed=11, seed_stride=7)
    assert (strided == render(g, name, views, seeds=(11, 18, 25))).all()
    for v, view in enumerate(views):
        assert (render(g, name, [view], seed=11 + 7 * v)[0] == strided[v]).all(), v
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "100")
    assert (render(g, name, views, seed=11, seed_stride=7) == strided).all()
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    # 2^64 - 3, 2^64 - 1, then past the wrap: 1
    wrapped = render(g, name, views, seed=2 ** 64 - 3, seed_stride=2)
    assert (wrapped == render(g, name, views, seeds=(2 ** 64 - 3, 2 ** 64 - 1, 1))).all()
    assert (wrapped[2] == render(g, name, [views[2]], seed=1)[0]).all()
    assert not (wrapped[2] == strided[2]).all()


# ---- 5. device memory; the flag
def test_device_tensors_and_general_traversal():
    name = "wine_glass"
    g = gpu(name)
    views = three_views(name)
    want = base(name)
    dev = torch.device("cuda", 0)
    out = torch.full(want.shape, -1.0, dtype=torch.float64, device=dev)
    assert render(g, name, views, seeds=SEEDS, out=out) is out
    assert (out.cpu().numpy() == want).all()
    out32 = torch.full(want.shape, -1.0, dtype=torch.float32, device=dev)
    render(g, name, views, seeds=SEEDS, out=out32)
    assert (out32.cpu().numpy() == want.astype(np.float32)).all()
    with torch.cuda.stream(torch.cuda.Stream(dev)):  # on a stream of the caller's own
        out2 = torch.zeros(want.shape, dtype=torch.float64, device=dev)
        render(g, name, views, seeds=SEEDS, out=out2)
        assert (out2.cpu().numpy() == want).all()
    host = np.full(want.shape, -1.0)
    assert render(g, name, views, seeds=SEEDS, out=host) is host and (host == want).all()
    assert (render(g, name, views, seeds=SEEDS, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL) == want).all()
    assert (render(gpu("cornell"), "cornell", three_views("cornell"), seeds=SEEDS, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
            == base("cornell")).all()


# ---- 6. the feature buffers
@pytest.mark.parametrize("name", SCENES)
def test_aov_views_with_their_seeds(name, oracle, monkeypatch):
    """a perspective view == rptgpu_render_aov of its camera and seed in every channel; the two other projections == the
    model's rays through closest_hit, folded as tests/test_gpu_views_aov.py folds them; the same bits in pieces of 100"""
    w, h = SIZES[name]
    n = w * h
    scene = small_scenes.small(name)[0]
    g = gpu(name)
    persp = cameras(name)[:3]
    got = render_aov(g, name, persp, seeds=SEEDS)
    for v, cam in enumerate(persp):
        assert aov_model.mismatches(view_of(got, v), g.render_aov(cam, params(name, SEEDS[v]))) == [], v
    lens, ortho, pano = three_views(name)
    mixed = base_aov(name)
    assert aov_model.mismatches(view_of(mixed, 0), g.render_aov(lens, params(name, SEEDS[0]))) == []
    col = aov_model.colors(scene)
    for v, view in ((1, ortho), (2, pano)):
        seed = SEEDS[v]
        o, d = np.empty((n, SPP, 3)), np.empty((n, SPP, 3))
        for k, s in enumerate(range(BASE, BASE + SPP)):
            if view is ortho:
                o[:, k], d[:, k] = M.orthographic_rays(oracle, view.camera, view.ortho_scale, seed, w, h, s)
            else:
                o[:, k], d[:, k] = M.panorama_rays(oracle, view.camera.eye, seed, w, h, s, M.device_sincos(g))[:2]
        t, nrm, obj = g.closest_hit(o.reshape(-1, 3), d.reshape(-1, 3))
        t, nrm, obj = t.reshape(n, SPP), nrm.reshape(n, SPP, 3), obj.reshape(n, SPP)
        want = {"hits": np.zeros(n, dtype=np.uint32), "depth": np.zeros(n), "normal": np.zeros((n, 3)), "albedo": np.zeros((n, 3)),
                "position": np.zeros((n, 3)), "object": np.zeros(n, dtype=np.int32)}
        with np.errstate(all="ignore"):
            for j in range(n):
                (want["hits"][j], want["depth"][j], want["normal"][j], want["albedo"][j], want["position"][j],
                 want["object"][j]) = aov_model.fold(o[j], d[j], t[j], nrm[j], obj[j], col)
        mine = {k: a[v].reshape(want[k].shape) for k, a in mixed.items()}
        assert aov_model.mismatches(mine, want) == [], ("orthographic", "panorama")[v - 1]
        assert 0 < want["hits"].sum()  # (it does see something)
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "100")
    assert aov_model.mismatches(render_aov(g, name, three_views(name), seeds=SEEDS), mixed) == []
    assert aov_model.mismatches(render_aov(g, name, three_views(name), seed=11, seed_stride=7),
                                render_aov(g, name, three_views(name), seeds=(11, 18, 25))) == []
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    dev = render_aov(g, name, three_views(name), seeds=SEEDS, out="torch")
    assert aov_model.mismatches({k: t.cpu().numpy().view(mixed[k].dtype) for k, t in dev.items()}, mixed) == []


# ---- 7. sharing: views with seeds of their own share the launches of a depth
def test_views_with_a_seed_stride_share_their_launches():
    """8 perspective views of the Cornell box at 37 x 21, 2 spp, 3 bounces, the default piece — one piece holds them all.
    A per-view depth loop (what seed_stride != 0 ran before the seed travelled with the path) launches about eight times
    what the stride-0 call launches; twice is a cap that such a loop cannot meet, not a measurement."""
    name = "cornell"
    w, h = SIZES[name]
    g = gpu(name)
    plain, beside, lens, L = cameras(name)
    eye, right = VT._v(plain.eye), np.cross(VT._v(plain.direction), VT._v(plain.up))
    views = [Camera(tuple(eye + (k - 3.5) * 0.02 * L * right), plain.direction, plain.up, plain.fov, 0.0, 0.0) for k in range(8)]
    launches = {}
    frames = {}
    for stride in (0, 1):
        g.reset_stats()
        frames[stride] = g.render_views(views, w, h, BOUNCES, samples=2, seed=21, seed_stride=stride)
        st = g.stats()
        launches[stride] = sum(int(c) for c in st.kernel_launches)
        assert st.kernel_launches[_abi.RPT_K_PATHS] == 0 and st.samples == 8 * w * h * 2
    print("kernel launches, 8 views: seed_stride 0: %d, seed_stride 1: %d" % (launches[0], launches[1]))
    assert launches[0] > 0 and launches[1] <= 2 * launches[0], launches
    assert (frames[0][0] == frames[1][0]).all() and not (frames[0][1] == frames[1][1]).all()
    p = make_params(w, h, BOUNCES, 2, seed=21 + 5)
    assert (frames[1][5].reshape(-1, 3) == g.render_batch(views[5], p)).all()
