"""rptgpu_render_views on the GPU: batches of perspective, orthographic and panoramic views.  Tolerance 0 (== on the f64
arrays) everywhere.

A perspective view has a reference inside the library — rptgpu_render_batch of its camera and seed — and, on the Cornell
box, outside it: the oracle's frame.  The two other projections have none, but the stream contract of rptgpu_trace_rays
gives one for any ray generator: the rays of tests/views_model.py (the header's formulas in numpy, their sines and
cosines evaluated on the device) handed to trace_rays with the pixel as stream id and first_draw = 2 must fold to the
views' frame, bit for bit.  The rest is the contract's last sentence: a view's pixels are its own."""
import functools
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import Camera, GpuScene, View, _abi, make_params

import small_scenes
import views_model as M

pytestmark = pytest.mark.gpu

# tests/test_gpu_trace_rays.py's scenes and sizes: the smallest frames that still span more than one 256-thread block and
# an odd number of them; flat with an object light, HDRI misses, deep trees at 8 bounces
SIZES = {"cornell": (37, 21), "glass": (33, 23), "wine_glass": (37, 21)}
SPP, BASE = 3, 5


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(small_scenes.small(name)[0], 0)


def _v(x):
    return np.array([float(c) for c in x])


@functools.lru_cache(maxsize=None)
def cameras(name):
    """the scene's camera without its lens, a second one from beside and above it with a narrower lens-less view, and
    the first under a lens focused half-way into the scene; and the length all of them are scaled by"""
    c = small_scenes.small(name)[1]
    eye, direction, up = _v(c.eye), _v(c.direction), _v(c.up)
    L = float(np.linalg.norm(eye))
    right = np.cross(direction, up)
    plain = Camera(c.eye, c.direction, c.up, c.fov, 0.0, 0.0)
    target = eye + direction * L
    beside = Camera.look_at(tuple(eye + 0.15 * L * right + 0.1 * L * up), tuple(target), tuple(up), 0.8 * c.fov)
    lens = Camera(c.eye, c.direction, c.up, c.fov, 0.0, 0.0).focus(tuple(eye + 0.5 * L * direction), 0.02 * L)
    assert lens.aperture > 0.0
    return plain, beside, lens, L


def other_views(name):
    """an orthographic view along the scene's camera and a panorama from a point 0.6 of the way into the scene"""
    plain, beside, lens, L = cameras(name)
    eye = _v(plain.eye) + 0.6 * L * _v(plain.direction)
    return View.orthographic(plain, L * math.tan(plain.fov / 2.0)), View.panorama(tuple(eye))


def render(g, name, views, **kw):
    w, h = SIZES[name]
    p0 = small_scenes.small(name)[2]
    kw.setdefault("samples", SPP)
    kw.setdefault("seed", p0.seed)
    kw.setdefault("sample_index_base", BASE)
    return g.render_views(views, w, h, p0.max_bounces, **kw)


@functools.lru_cache(maxsize=None)
def mixed(name, stride):
    """(views, their frames): every projection, the lens, and a second perspective view — computed once, never written to"""
    plain, beside, lens, L = cameras(name)
    views = (lens,) + other_views(name) + (beside,)
    out = render(gpu(name), name, views, seed_stride=stride)
    out.setflags(write=False)
    return views, out


@pytest.mark.parametrize("stride", [0, 7])
@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"])
def test_a_perspective_view_is_render_batch(name, stride, oracle):
    """three cameras, one under a lens: view v == rptgpu_render_batch of its camera with seed + v * seed_stride — and,
    on the Cornell box, == the oracle's frame"""
    w, h = SIZES[name]
    scene, _, p0 = small_scenes.small(name)
    g = gpu(name)
    views = cameras(name)[:3]
    g.reset_stats()
    got = render(g, name, views, seed_stride=stride)
    st = g.stats()
    assert got.shape == (3, h, w, 3) and got.dtype == np.float64 and np.isfinite(got).all()
    assert st.samples == 3 * w * h * SPP and st.kernel_launches[_abi.RPT_K_PATHS] == 0  # wavefront only
    assert st.kernel_launches[_abi.RPT_K_RAYGEN] >= (3 if stride else 1)
    for v, cam in enumerate(views):
        p = make_params(w, h, p0.max_bounces, SPP, seed=p0.seed + v * stride, sample_index_base=BASE)
        want = g.render_batch(cam, p)
        assert (got[v].reshape(-1, 3) == want).all(), "view %d: %d pixels differ" % (v, (got[v].reshape(-1, 3) != want).any(axis=1).sum())
        if name == "cornell":
            assert (want == oracle.OracleScene(scene).render(cam, p)).all(), v
    assert not (got[0] == got[2]).all() and not (got[0] == got[1]).all()


@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"])
def test_orthographic_and_panorama_are_the_headers_rays(name, oracle):
    """per sample index the model's rays through trace_rays (streams = pixel, first_draw = 2, one sample, exposure 0),
    folded in sample order from +0.0, / iterations * 2^EV: the views' frame, with exposure_value 0 and 1"""
    w, h = SIZES[name]
    scene, _, p0 = small_scenes.small(name)
    g = gpu(name)
    ortho, pano = other_views(name)
    seed, stride = p0.seed, 3
    pixels = np.arange(w * h, dtype=np.uint32)
    sums = []
    for v, view in enumerate((ortho, pano)):
        acc = np.zeros((w * h, 3))
        for s in range(BASE, BASE + SPP):
            if view is ortho:
                o, d = M.orthographic_rays(oracle, view.camera, view.ortho_scale, seed + v * stride, w, h, s)
            else:
                o, d, _, _ = M.panorama_rays(oracle, view.camera.eye, seed + v * stride, w, h, s, M.device_sincos(g))
            acc = acc + g.trace_rays(o, d, p0.max_bounces, samples=1, seed=seed + v * stride, sample_index_base=s,
                                     streams=pixels, first_draw=2, exposure_value=0.0)
        sums.append(acc)
    for ev in (0.0, 1.0):
        got = render(g, name, (ortho, pano), seed_stride=stride, exposure_value=ev)
        for v in range(2):
            want = sums[v] / float(SPP) * 2.0 ** ev
            assert (got[v].reshape(-1, 3) == want).all(), \
                "%s, EV %g: %d pixels differ" % (("orthographic", "panorama")[v], ev, (got[v].reshape(-1, 3) != want).any(axis=1).sum())
    assert not (sums[0] == sums[0][0]).all() and not (sums[1] == sums[1][0]).all()  # (they do see something)


@pytest.mark.parametrize("stride", [0, 7])
@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"])
def test_a_views_pixels_are_its_own(name, stride, monkeypatch):
    w, h = SIZES[name]
    g = gpu(name)
    views, base = mixed(name, stride)
    n = len(views) * w * h
    # pieces of 100 indices: they end inside a view and — the views' seeds being one — span two
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "100")
    g.reset_stats()
    assert (render(g, name, views, seed_stride=stride) == base).all()
    pieces = len(views) * ((w * h + 99) // 100) if stride else (n + 99) // 100
    assert g.stats().kernel_launches[_abi.RPT_K_RAYGEN] >= pieces and g.stats().samples == n * SPP
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    # every view alone, with the seed it had in the batch
    seed = small_scenes.small(name)[2].seed
    for v, view in enumerate(views):
        assert (render(g, name, [view], seed=seed + v * stride)[0] == base[v]).all(), v
    # in reverse order (with a stride the seeds would move with the places: the views alone cover that)
    if not stride:
        assert (render(g, name, views[::-1]) == base[::-1]).all()
        monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "100")
        assert (render(g, name, views[::-1]) == base[::-1]).all()


def test_outputs_and_flags():
    name = "wine_glass"
    w, h = SIZES[name]
    g = gpu(name)
    views, base = mixed(name, 7)
    dev = torch.device("cuda", 0)
    out = torch.full(base.shape, -1.0, dtype=torch.float64, device=dev)
    assert render(g, name, views, seed_stride=7, out=out) is out
    assert (out.cpu().numpy() == base).all()
    out32 = torch.full(base.shape, -1.0, dtype=torch.float32, device=dev)
    render(g, name, views, seed_stride=7, out=out32)
    assert (out32.cpu().numpy() == base.astype(np.float32)).all()
    with torch.cuda.stream(torch.cuda.Stream(dev)):  # on a stream of the caller's own
        out2 = torch.zeros(base.shape, dtype=torch.float64, device=dev)
        render(g, name, views, seed_stride=7, out=out2)
        assert (out2.cpu().numpy() == base).all()
    host = np.full(base.shape, -1.0)
    assert render(g, name, views, seed_stride=7, out=host) is host and (host == base).all()
    g.reset_stats()
    assert (render(g, name, views, seed_stride=7, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL) == base).all()
    assert (render(g, name, views, seed_stride=7, flags=_abi.RPT_FLAG_PROFILE_KERNELS | _abi.RPT_FLAG_WAVEFRONT) == base).all()
    st = g.stats()
    assert st.samples == 2 * len(views) * w * h * SPP and st.kernel_launches[_abi.RPT_K_PATHS] == 0
    assert st.kernel_ms[_abi.RPT_K_RAYGEN] > 0.0
    with pytest.raises(ValueError):
        render(g, name, views, out=torch.zeros(base.shape, dtype=torch.float64))  # a host tensor


def test_a_panorama_is_an_environment():
    """A sky whose red is the column and whose green is the row of its texel grid, captured as a panorama of the same
    size: Hdri::get_color interpolates such a ramp exactly, so a sample that points at (cx, cy) returns (cx, cy) — and
    the mean over a pixel's samples, all within half a texel of (x, y), stays within half a texel of it: the panorama
    is laid out as the Hdri it came from.  Rounding is around 1e-14 texel; 1e-9 is allowed.  Columns 0 and width-1
    (one meridian: samples wrap between them) and the pole rows (the one object, a speck straight below the eye, is
    only seen from the last) are left out."""
    from rpt_amd import Environment, Hdri, Material, Object, Scene, sphere
    w, h = 16, 9
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    sky = Hdri(w, h, np.stack([x, y, np.full_like(x, 0.25)], axis=-1))
    scene = Scene()
    scene.environment = Environment.Hdri(sky)
    scene.add(Object(sphere().scale((0.01, 0.01, 0.01)).translate((0.0, -50.0, 0.0))).material(Material.diffuse((0.5, 0.5, 0.5))))
    g = GpuScene(scene, 0)
    pano = g.render_views([View.panorama((0.0, 0.0, 0.0))], w, h, 0, samples=16, seed=9)[0]
    g.close()
    inner = (slice(1, h - 1), slice(1, w - 1))
    assert np.abs(pano[..., 0] - x)[inner].max() <= 0.5 + 1e-9
    assert np.abs(pano[..., 1] - y)[inner].max() <= 0.5 + 1e-9
    assert (pano[..., 2][inner] == 0.25).all() or np.abs(pano[..., 2][inner] - 0.25).max() <= 1e-15
    assert np.abs(pano[..., 0] - x)[inner].max() > 0.0  # (the samples are jittered)


# (The abandoned handle's refusal, RPTGPU_E_COMM, is REFUSE_IF_ABANDONED, the macro every entry point that enqueues work
# shares; tests/test_gpu_trace_rays.py says why no test brings such a handle about.)
def test_refusals_on_a_live_handle():
    name = "cornell"
    w, h = SIZES[name]
    g = gpu(name)
    plain, beside, lens, L = cameras(name)
    out = np.full((2, h, w, 3), 7.0)
    for views, kw, word in (((plain, beside), dict(flags=_abi.RPT_FLAG_PERSISTENT), "RPT_FLAG_PERSISTENT"),
                            ((plain, beside), dict(samples=0), "must be non-zero"),
                            ((plain, View.orthographic(lens, 1.0)), {}, "only RPT_VIEW_PERSPECTIVE has a lens"),
                            ((plain, View.orthographic(plain, 0.0)), {}, "ortho_scale"),
                            ((View(plain, 9), plain), {}, "unknown projection")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            render(g, name, views, out=out, **kw)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
        assert (out == 7.0).all()
    assert render(g, name, []).shape == (0, h, w, 3)  # n_views == 0: nothing to do
    p0 = small_scenes.small(name)[2]
    p = make_params(w, h, p0.max_bounces, SPP, seed=p0.seed, sample_index_base=BASE)
    assert (render(g, name, [plain])[0].reshape(-1, 3) == g.render_batch(plain, p)).all()  # the handle is as it was
