"""rptgpu_render_views_denoised on the GPU: a denoised frame per view of a batch, in one call.  Tolerance 0 (== on the bits
of the f64 arrays) everywhere.

The call has two references.  Inside the library, for a perspective view: a DeviceBuffer on the same handle, sampled
`batches` times, with features, denoised.  Outside it, for every projection: tests/denoise_model.py (the filter's contract
in numpy) on inputs built here from three render_views calls — the Welford state in the header's order — and one
render_views_aov call with the same seeds.  The rest is the contract's sentence that a view's outputs are its own: the same
bits whatever the pieces, the order, the other views, the seed's form, the outputs asked for and the memory they lie in.

Scenes, sizes and cameras are tests/test_gpu_views.py's: cornell and wine_glass at 37 x 21, glass at 33 x 23 (sky and
surface).  Three views — a perspective view under a lens, an orthographic view, a panorama —, three bounces, three batches
of two samples from sample 5, features from two samples at sample 0, seeds (5, 2^63 + 1, 5).  At 21 rows the taps of level
index 4 (16 and 32 pixels out) leave the view and land, in memory, inside the next view's rows."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

from rpt_amd import DeviceBuffer, _abi, make_params
from rpt_amd.color import color_bytes

import denoise_model as M
import test_gpu_views as VT

pytestmark = pytest.mark.gpu

SCENES = ["cornell", "glass", "wine_glass"]
SIZES = VT.SIZES
BOUNCES, SPP, BATCHES, BASE, FSPP, FBASE = 3, 2, 3, 5, 2, 0
SEEDS = (5, 2 ** 63 + 1, 5)
ALL = ("denoised", "rgb8", "mean", "variance")
gpu, cameras, other_views = VT.gpu, VT.cameras, VT.other_views


def three_views(name):
    """a perspective view under a lens, an orthographic view, a panorama"""
    return (cameras(name)[2],) + other_views(name)


def call(g, views, w, h, **kw):
    kw.setdefault("samples", SPP)
    kw.setdefault("batches", BATCHES)
    kw.setdefault("sample_index_base", BASE)
    kw.setdefault("feature_samples", FSPP)
    kw.setdefault("feature_sample_index_base", FBASE)
    return g.render_views_denoised(views, w, h, BOUNCES, **kw)


def same(got, want):
    return got.shape == want.shape and np.array_equal(M.bits(got), M.bits(want))


def same_all(got, want):
    return sorted(got) == sorted(want) and all(
        np.array_equal(got[k], want[k]) if got[k].dtype == np.uint8 else same(got[k], want[k]) for k in want)


def model(g, views, w, h, seeds, **filt):
    """the header's definition in numpy: per view the batches by render_views, their Welford state, the features by
    render_views_aov, the filter by denoise_model -> denoised, mean, variance, hits"""
    frames = [g.render_views(views, w, h, BOUNCES, samples=SPP, sample_index_base=BASE + b * SPP, seeds=seeds)
              for b in range(BATCHES)]
    ch = _abi.RPT_AOV_DEPTH | _abi.RPT_AOV_NORMAL | _abi.RPT_AOV_ALBEDO | _abi.RPT_AOV_POSITION
    aov = g.render_views_aov(views, w, h, samples=FSPP, sample_index_base=FBASE, channels=ch, seeds=seeds)
    out = {"denoised": [], "mean": [], "variance": [], "hits": aov["hits"]}
    for v in range(len(views)):
        total, counts, M2 = M.welford([f[v] for f in frames])
        feats = {k: a[v] for k, a in aov.items()}
        out["denoised"].append(M.denoise(total, counts, M2, feats, **filt))
        n = counts.astype(np.float64)
        with np.errstate(all="ignore"):
            out["mean"].append(total / n[..., None])
            out["variance"].append((M2 / (n - 1.0)) / n)
    return {k: np.stack(a) if isinstance(a, list) else a for k, a in out.items()}


@functools.lru_cache(maxsize=None)
def base(name):
    """the three views under SEEDS, every output, three levels, one piece — computed once, never written to"""
    w, h = SIZES[name]
    out = call(gpu(name), three_views(name), w, h, seeds=SEEDS, want=ALL)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def base_model(name):
    w, h = SIZES[name]
    out = model(gpu(name), three_views(name), w, h, SEEDS)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- 1. a perspective view is the Buffer a caller fills and denoises per view
@pytest.mark.parametrize("name", SCENES)
def test_a_perspective_view_is_the_buffer(name):
    w, h = SIZES[name]
    g = gpu(name)
    plain, beside, lens, _ = cameras(name)
    views = (lens, beside, plain)
    got = call(g, views, w, h, seeds=SEEDS, want=("denoised", "rgb8"))
    assert got["denoised"].shape == (3, h, w, 3) and np.isfinite(got["denoised"]).all()
    for v, cam in enumerate(views):
        buf = DeviceBuffer(g, w, h)
        for b in range(BATCHES):
            buf.sample(cam, make_params(w, h, BOUNCES, SPP, seed=SEEDS[v], sample_index_base=BASE + b * SPP))
        buf.features(cam, make_params(w, h, BOUNCES, FSPP, seed=SEEDS[v], sample_index_base=FBASE))
        want = buf.denoise()
        assert same(got["denoised"][v], want), "view %d: %d values differ" % (v, (M.bits(got["denoised"][v]) != M.bits(want)).sum())
        assert np.array_equal(got["rgb8"][v], buf.denoised_image())
        raw = buf.totals() / float(BATCHES)
        assert not same(want, raw)  # it did filter
        buf.close()
    assert same(got["denoised"][0], base(name)["denoised"][0])  # the lens among the other projections


# ---- 2. (and 7.) every projection is the model on inputs made by render_views and render_views_aov
@pytest.mark.parametrize("name", SCENES)
def test_every_projection_is_the_model(name):
    got, want = base(name), base_model(name)
    for k in ("mean", "variance", "denoised"):
        for v in range(3):
            assert same(got[k][v], want[k][v]), "%s of view %d: %d values differ" % (k, v, (M.bits(got[k][v]) != M.bits(want[k][v])).sum())
    assert not same(got["denoised"], got["mean"]) and (got["variance"] >= 0).all()
    if name == "glass":  # sky and surface in one frame: the model never mixes them, so neither does the device
        hits = want["hits"]
        assert all((hits[v] == 0).any() and (hits[v] > 0).any() for v in range(3))


# ---- 3. levels, frames smaller than the taps' reach, other sigmas
@pytest.mark.parametrize("levels", [1, 5])
@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_levels_whose_taps_leave_the_view(name, levels):
    w, h = SIZES[name]
    g = gpu(name)
    got = call(g, three_views(name), w, h, seeds=SEEDS, levels=levels)["denoised"]
    want = model(g, three_views(name), w, h, SEEDS, levels=levels)["denoised"]
    assert same(got, want), "%d values differ" % (M.bits(got) != M.bits(want)).sum()
    assert not same(got, base(name)["denoised"])  # (three levels)


@pytest.mark.parametrize("w,h", [(1, 37), (7, 5)])
def test_frames_smaller_than_a_block(w, h):
    """no panorama: that projection needs width and height >= 2"""
    g = gpu("cornell")
    views = three_views("cornell")[:2] + (cameras("cornell")[1],)
    got = call(g, views, w, h, seeds=SEEDS, levels=5, want=ALL)
    want = model(g, views, w, h, SEEDS, levels=5)
    assert all(same(got[k], want[k]) for k in ("denoised", "mean", "variance"))
    assert np.array_equal(got["rgb8"], color_bytes(got["denoised"]))


def test_other_sigmas():
    w, h = SIZES["glass"]
    g = gpu("glass")
    filt = dict(levels=2, sigma_color=0.7, sigma_normal=0.35, sigma_depth=0.2, sigma_albedo=0.03)
    got = call(g, three_views("glass"), w, h, seeds=SEEDS, **filt)["denoised"]
    assert same(got, model(g, three_views("glass"), w, h, SEEDS, **filt)["denoised"])
    assert not same(got, call(g, three_views("glass"), w, h, seeds=SEEDS, levels=2)["denoised"])


# ---- 4. a view's outputs are its own
@pytest.mark.parametrize("name", SCENES)
def test_pieces_order_and_neighbours_change_nothing(name, monkeypatch):
    w, h = SIZES[name]
    g = gpu(name)
    views = three_views(name)
    want = base(name)
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "100")
    assert same_all(call(g, views, w, h, seeds=SEEDS, want=ALL), want)
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    back = call(g, views[::-1], w, h, seeds=SEEDS[::-1], want=ALL)
    assert same_all({k: a[::-1] for k, a in back.items()}, want)
    for v in range(3):
        alone = call(g, views[v:v + 1], w, h, seeds=SEEDS[v:v + 1], want=ALL)
        assert same_all({k: a[0] for k, a in alone.items()}, {k: a[v] for k, a in want.items()}), v
    # views 0 and 2 have one seed: given one camera they give one frame, and view 1 between them another
    twice = call(g, (views[0], views[1], views[0]), w, h, seeds=SEEDS, want=ALL)
    assert same_all({k: a[0] for k, a in twice.items()}, {k: a[2] for k, a in twice.items()})
    assert same_all({k: a[:2] for k, a in twice.items()}, {k: a[:2] for k, a in want.items()})


# ---- 5. the seed's forms
def test_seed_forms():
    name = "wine_glass"
    w, h = SIZES[name]
    g = gpu(name)
    views = three_views(name)
    strided = call(g, views, w, h, seed=11, seed_stride=7, want=ALL)
    assert same_all(strided, call(g, views, w, h, seeds=(11, 18, 25), want=ALL))
    one = call(g, views, w, h, seed=11, want=ALL)
    assert same_all(one, call(g, views, w, h, seeds=(11, 11, 11), want=ALL))
    assert same(one["denoised"][0], strided["denoised"][0]) and not same(one["denoised"][1], strided["denoised"][1])


# ---- 6. the outputs
@pytest.mark.parametrize("name", SCENES)
def test_outputs(name):
    w, h = SIZES[name]
    g = gpu(name)
    views = three_views(name)
    want = base(name)
    assert want["rgb8"].dtype == np.uint8 and np.array_equal(want["rgb8"], color_bytes(want["denoised"]))
    for k in ("denoised", "rgb8"):  # each alone: the others NULL
        assert same_all(call(g, views, w, h, seeds=SEEDS, want=(k,)), {k: want[k]})
    for k in ("mean", "variance"):  # ... beside the one output the call must have
        assert same_all(call(g, views, w, h, seeds=SEEDS, want=("rgb8", k)), {"rgb8": want["rgb8"], k: want[k]})
    on_device = call(g, views, w, h, seeds=SEEDS, want=ALL, out="torch")
    assert all(t.is_cuda for t in on_device.values())
    assert same_all({k: t.cpu().numpy() for k, t in on_device.items()}, want)
    mine = {"denoised": torch.full((3, h, w, 3), 7.0, dtype=torch.float64, device="cuda:0")}
    assert call(g, views, w, h, seeds=SEEDS, out=mine)["denoised"] is mine["denoised"]
    assert same(mine["denoised"].cpu().numpy(), want["denoised"])
    assert same_all(call(g, views, w, h, seeds=SEEDS, want=ALL, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL), want)


# ---- 8. the views share the launches
def test_eight_views_share_their_launches():
    """RptStats counts the render kernels, not the filter's, so what it can show is the total: the one call against the loop
    a caller writes, per view a Buffer, on the same handle and through the same pipeline (RPT_FLAG_WAVEFRONT: a batch of
    views always runs the wavefront kernels; the default loop on this flat scene takes the persistent kernel, one counted
    launch per batch whatever its work, which says nothing about sharing — its count is printed beside the others)."""
    name = "cornell"
    w, h = SIZES[name]
    g = gpu(name)
    plain, beside, lens, _ = cameras(name)
    views = [plain, beside, lens, plain, beside, lens, plain, beside]
    seeds = list(range(40, 48))

    def launches():
        return int(sum(g.stats().kernel_launches))

    g.reset_stats()
    got = call(g, views, w, h, seeds=seeds)["denoised"]
    one_call = launches()
    st = g.stats()
    assert st.samples == 8 * w * h * SPP * BATCHES  # as `batches` view renders
    counts = {}
    for flags in (_abi.RPT_FLAG_WAVEFRONT, 0):
        g.reset_stats()
        for v, cam in enumerate(views):
            buf = DeviceBuffer(g, w, h)
            for b in range(BATCHES):
                buf.sample(cam, make_params(w, h, BOUNCES, SPP, seed=seeds[v], sample_index_base=BASE + b * SPP, flags=flags))
            buf.features(cam, make_params(w, h, BOUNCES, FSPP, seed=seeds[v], sample_index_base=FBASE, flags=flags))
            assert same(got[v], buf.denoise()), (flags, v)
            buf.close()
        counts[flags] = launches()
    print("launches counted by RptStats: one call %d, the 8-Buffer loop %d (wavefront), %d (default route)"
          % (one_call, counts[_abi.RPT_FLAG_WAVEFRONT], counts[0]))
    assert one_call < counts[_abi.RPT_FLAG_WAVEFRONT]
