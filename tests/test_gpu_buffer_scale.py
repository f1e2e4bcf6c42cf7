"""The device Buffer where its kernels change behaviour: a 1920x1080 adaptive render (hundreds of blocks
of the list compaction), list lengths at the compaction's tile size, tiny and one-pixel-wide frames, sparse lists split
over passes and launches, the u8 conversion at every byte threshold, filter radii past the frame and variance edges.

As in test_gpu_adaptive.py, random numbers are keyed by (pixel, sample index): a pixel rendered in an adaptive round at
sample_index_base B gets bit for bit what a plain full-frame rptgpu_render_batch at B gives it, so every expectation is
the numpy model (adaptive_model.py) run over plain frames.  Bits are compared, not tolerances."""
import math
import os
import re

import numpy as np
import pytest

import rpt_amd
from rpt_amd import Camera, Filter, GpuScene, Light, Material, Object, Scene, _abi, make_params, polygon, scenes
from rpt_amd.color import color_bytes

import adaptive_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def retire_tile():
    """RPT_RETIRE_TILE of kernels.h: list entries per 256-thread block of rpt_retire_count / rpt_retire_scatter"""
    with open(os.path.join(ROOT, "rpt_amd", "csrc", "kernels.h")) as f:
        items = int(re.search(r"#define RPT_RETIRE_ITEMS (\d+)u", f.read()).group(1))
    return items * 256


def wall_scene():
    """A diffuse wall filling the view, lit by a point light, no bounces: a pixel's value depends smoothly on where its
    jittered camera ray lands, so every pixel has noise of its own and no two pixels' statistics tie."""
    scene = Scene()
    s = 1000.0
    scene.add(Object(polygon([(-s, -s, 0.0), (s, -s, 0.0), (s, s, 0.0), (-s, s, 0.0)]))
              .material(Material.diffuse((0.8, 0.7, 0.6))))
    scene.add(Light.Point((60.0, 50.0, 40.0), (1.5, 2.0, 4.0)))
    return scene, Camera()  # the default camera: eye (0, 0, 10) looking down -z


def emitter_scene(c):
    """One emissive polygon filling the view, nothing else: a sample's value is emittance * colour = c exactly"""
    scene = Scene()
    scene.add(emitter(c))
    return scene, Camera()


def emitter(c):
    s = 1000.0
    return Object(polygon([(-s, -s, 0.0), (s, -s, 0.0), (s, s, 0.0), (-s, s, 0.0)])).material(Material.light(c, 1.0))


@pytest.fixture(scope="module")
def handles():
    cache = {}

    def get(name):
        if name not in cache:
            if name == "sphere":
                scene, cam, _ = scenes.sphere_scene()  # default environment: constant black sky
            elif name == "wall":
                scene, cam = wall_scene()
            else:
                scene, cam = emitter_scene((0.5, 0.5, 0.5))
            cache[name] = (scene, cam, GpuScene(scene, 0))
        return cache[name]

    yield get
    for v in cache.values():
        v[2].close()


def adaptive(g, cam, w, h, rounds, params, mb, abs_tol, rel_tol, radius=0):
    dev = rpt_amd.DeviceBuffer(g, w, h, Filter.Box(radius))
    left = [dev.sample_adaptive(cam, params(k), mb, abs_tol, rel_tol) for k in range(rounds)]
    return dev, left


def longdouble_variance(frames, counts):
    """Buffer::variance's value computed another way: per pixel a two-pass sample variance in extended precision, then
    the mean over the pixels by math.fsum (exactly rounded)"""
    n = counts.astype(np.longdouble)
    total = np.zeros(frames[0].shape, dtype=np.longdouble)
    for k, F in enumerate(frames):
        total += np.where((counts > k)[:, None], F.astype(np.longdouble), 0.0)
    mean = total / n[:, None]
    ss = np.zeros(len(counts), dtype=np.longdouble)
    for k, F in enumerate(frames):
        d = F.astype(np.longdouble) - mean
        ss += np.where(counts > k, (d * d).sum(axis=1), 0.0)
    return math.fsum((ss / (n - 1)).astype(np.float64).tolist()) / len(counts)


# ------------------------------------------------------------------ 1. adaptive rounds at 1920x1080
W1, H1, K1, MB1 = 1920, 1080, 5, 2


@pytest.mark.parametrize("flags", [0, _abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT])
def test_adaptive_rounds_at_1080p(handles, flags):
    """507 blocks in the first compaction (more than 256: the strided block-offset loop takes a second step), a partly
    full tail block, the last block writing the new length; every round from min_batches on retires some pixels."""
    tile = retire_tile()
    P = W1 * H1
    assert P > 256 * tile and P % tile != 0
    scene, cam, g = handles("sphere")

    def params(k):
        return make_params(W1, H1, 1, 1, seed=33, sample_index_base=k, exposure_value=0.5, flags=flags)

    frames = [g.render_batch(cam, params(k)) for k in range(K1)]
    for rel in (0.3, 0.1, 0.5, 0.05, 1.0, 0.02):  # every round from min_batches on retires some pixels, never all
        r = M.run(frames, MB1, 0.0, rel)
        a = r["active"]
        if a[MB1 - 2] == P and all(a[k] < a[k - 1] for k in range(MB1 - 1, K1)) and a[-1] > 0:
            break
    else:
        raise AssertionError("no tolerance retires pixels in every round: %s" % r["active"])
    assert any(x % 256 for x in r["active"]), r["active"]
    for radius in (0, 2):
        dev, left = adaptive(g, cam, W1, H1, K1, params, MB1, 0.0, rel, radius)
        counts = M.check_against(dev, left, frames, r)
        totals = M.masked_totals(frames, counts)
        assert np.array_equal(dev.image(), M.filtered_image(totals, counts, W1, H1, radius)), radius
        v = dev.variance()
        want = M.variance(frames, counts)
        assert M.bits(v) == M.bits(want), (v, want)
        indep = longdouble_variance(frames, counts)
        assert abs(v - indep) <= 1e-12 * abs(indep), (v, indep)
        dev.close()


# ------------------------------------------------------------------ 2. list lengths at the tile size, tiny frames
@pytest.mark.parametrize("w,h", [(63, 65), (64, 64), (17, 241), (1, 37), (37, 1), (7, 5), (33, 9)])
def test_list_lengths_and_tiny_frames(handles, w, h):
    """4095, 4096 and 4097 list entries (one block exactly full, one entry either side), frames smaller than an 8x8
    block or a 32x8 tile and one pixel wide or high; tolerances the model picks so that nothing retires, everything
    retires, exactly one pixel survives, and all but one survive."""
    scene, cam, g = handles("wall")
    K, mb, P = 4, 2, w * h

    def params(k):
        return make_params(w, h, 0, 1, seed=5, sample_index_base=k, flags=0)

    frames = [g.render_batch(cam, params(k)) for k in range(K)]
    r2 = M.run(frames[:mb], mb, 0.0, 0.0)  # e of every pixel at n = mb
    n2 = np.full(P, float(mb))
    e = np.sort((r2["M2"] / (n2 - 1.0)) / n2)
    assert e[0] > 0.0 and (P < 2 or (e[1] > e[0] and e[-1] > e[-2])), e[:3]
    cases = [(0.0, P), (1e300, 0)]
    if P > 1:
        cases += [(float(np.sqrt(0.5 * (e[-1] + e[-2]))), 1), (float(np.sqrt(0.5 * (e[0] + e[1]))), P - 1)]
    for abs_tol, survivors in cases:
        r = M.run(frames, mb, abs_tol, 0.0)
        assert r["active"][:mb] == [P] * (mb - 1) + [survivors], (abs_tol, r["active"])
        dev, left = adaptive(g, cam, w, h, K, params, mb, abs_tol, 0.0, radius=1)
        counts = M.check_against(dev, left, frames, r)
        totals = M.masked_totals(frames, counts)
        want = M.filtered_image(totals, counts, w, h, 1)
        assert np.array_equal(dev.image(), want)
        if P <= 64:  # the per-pixel Python reference too
            ref = M.ref_filtered(M.pixel_lists(frames, counts), w, h, 1)
            assert np.array_equal(want, color_bytes(ref))
        assert M.bits(dev.variance()) == M.bits(M.variance(frames, counts))
        dev.close()


# ------------------------------------------------------------------ 3. sparse lists split over passes and launches
W3, H3, S3, K3 = 192, 108, 3, 4


def test_sparse_lists_split_over_passes_and_launches(handles, monkeypatch):
    """Rounds after the sky has retired render a sparse list; forced tiny wavefront passes, one or five samples per
    work item of the persistent kernel and a radiance buffer that holds one or two samples of that list must not
    change a bit of the counts or totals."""
    scene, cam, g = handles("sphere")

    def params(flags):
        return lambda k: make_params(W3, H3, 1, S3, seed=8, sample_index_base=k * S3, exposure_value=0.5, flags=flags)

    P = W3 * H3
    frames = [g.render_batch(cam, params(0)(k)) for k in range(K3)]
    # round 1 retires most of the frame (the sky at least), and the list left still needs several 4096-path passes
    runs = [M.run(frames, 2, 0.0, rel) for rel in (0.3, 0.5, 1.0, 0.1, 0.03)]
    ok = [(rel, r) for rel, r in zip((0.3, 0.5, 1.0, 0.1, 0.03), runs)
          if r["active"][1] * S3 > 2 * 4096 and r["active"][-1] > 0]
    assert ok, [r["active"] for r in runs]
    rel, r = min(ok, key=lambda t: t[1]["active"][1])
    sparse = r["active"][1]  # the list of round 2
    assert sparse < P // 2, r["active"]
    ref = {}
    for flags in (_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT):
        dev, left = adaptive(g, cam, W3, H3, K3, params(flags), 2, 0.0, rel)
        ref[flags] = (M.check_against(dev, left, frames, r), M.bits(dev.totals()))
        dev.close()
    settings = [({"RPTGPU_TARGET_PATHS": "4096"}, _abi.RPT_FLAG_WAVEFRONT, None)]
    for chunk in (1, 5):
        for cap in (1, 2):
            settings.append(({"RPTGPU_PATHS_CHUNK": str(chunk), "RPTGPU_LBUF_BYTES": str(sparse * 24 * cap)},
                             _abi.RPT_FLAG_PERSISTENT, cap))
    for env, flags, cap in settings:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g2 = GpuScene(scene, 0)
        for k in env:
            monkeypatch.delenv(k)
        dev = rpt_amd.DeviceBuffer(g2, W3, H3)
        pp = params(flags | _abi.RPT_FLAG_PROFILE_KERNELS)
        left = []
        for k in range(K3):
            g2.reset_stats()
            left.append(dev.sample_adaptive(cam, pp(k), 2, 0.0, rel))
            if k == 2 and cap is not None:  # the sparse list's batch, split into launches of `cap` samples
                launches = g2.stats().kernel_launches[_abi.RPT_K_PATHS]
                assert launches == -(-S3 // cap), (env, launches)
        assert left == r["active"], env
        assert np.array_equal(dev.sample_counts().ravel(), ref[flags][0]), env
        assert np.array_equal(M.bits(dev.totals()), ref[flags][1]), env
        dev.close()
        g2.close()


# ------------------------------------------------------------------ 4. the byte staircase
def host_thresholds():
    """thr[k] (k = 1..255): the smallest double in [0, 1] that rpt_amd.color.color_bytes maps to k or more, by
    bisection over the bit patterns, all 255 at once"""
    k = np.arange(1, 256)
    lo = np.zeros(255, dtype=np.uint64)
    hi = np.full(255, np.float64(1.0).view(np.uint64))
    while (lo < hi).any():
        mid = lo + (hi - lo) // np.uint64(2)
        ge = color_bytes(mid.view(np.float64)) >= k
        hi = np.where(ge, mid, hi)
        lo = np.where(ge, lo, mid + np.uint64(1))
    return lo.view(np.float64)


def test_u8_conversion_at_every_byte_threshold(handles):
    """Every value from 2 ulps below to 2 ulps above each of the 255 byte thresholds, plus 0, 1, a value above 1 and
    +inf, as the colour of an emitter filling a 2x2 frame: image() must be color_bytes of the read-back mean."""
    scene, cam, g = handles("emitter")
    thr = host_thresholds()
    assert thr[0] > 0.0 and thr[-1] <= 1.0 and (np.diff(thr) > 0).all()
    u = thr.view(np.int64)
    vals = np.concatenate([(u + d).view(np.float64) for d in range(-2, 3)] + [[0.0, 1.0, 1.75]])
    vals = np.concatenate([vals, np.full((-len(vals)) % 3, 0.5)])
    p = make_params(2, 2, 0, 1, seed=3, exposure_value=0.0)
    seen = []
    for c in vals.reshape(-1, 3):
        g.set_objects([0], [emitter(tuple(float(x) for x in c))])
        dev = rpt_amd.DeviceBuffer(g, 2, 2)
        dev.sample(cam, p)
        mean = dev.totals() / dev.sample_counts()[:, :, None]
        assert np.array_equal(dev.image(), color_bytes(mean)), c
        seen.append(mean.reshape(-1, 3))
        dev.close()
    # +inf: an exposure scale of 2^2000 overflows
    g.set_objects([0], [emitter((1.0, 1.0, 1.0))])
    dev = rpt_amd.DeviceBuffer(g, 2, 2)
    dev.sample(cam, make_params(2, 2, 0, 1, seed=3, exposure_value=2000.0))
    mean = dev.totals() / dev.sample_counts()[:, :, None]
    assert np.isposinf(mean).all()
    assert (dev.image() == 255).all() and (color_bytes(mean) == 255).all()
    dev.close()
    g.set_objects([0], [emitter((0.5, 0.5, 0.5))])
    # the read-back values really are the colours asked for: both sides of every threshold were rendered
    landed = set(np.concatenate(seen).ravel().tolist())
    for t in thr:
        assert float(t) in landed and float(np.nextafter(t, 0.0)) in landed, t
    assert 0.0 in landed and 1.0 in landed and 1.75 in landed


# ------------------------------------------------------------------ 5. Buffer edges
def test_filter_radius_at_and_past_the_frame(handles):
    w, h, K = 13, 7, 5
    scene, cam, g = handles("wall")

    def params(k):
        return make_params(w, h, 0, 1, seed=12, sample_index_base=k)

    frames = [g.render_batch(cam, params(k)) for k in range(K)]
    r2 = M.run(frames[:2], 2, 0.0, 0.0)
    e = np.sort((r2["M2"] / 1.0) / 2.0)
    tol = float(np.sqrt(e[len(e) // 2]))  # about half the pixels retire at n = 2, the rest later or never
    r = M.run(frames, 2, tol, 0.0)
    assert 0 < r["active"][1] < w * h
    for radius in sorted({w - 1, w, max(w, h), w + h}):
        dev, left = adaptive(g, cam, w, h, K, params, 2, tol, 0.0, radius)
        counts = M.check_against(dev, left, frames, r)
        assert len(set(counts.tolist())) > 1
        ref = M.ref_filtered(M.pixel_lists(frames, counts), w, h, radius)
        assert np.array_equal(dev.image(), color_bytes(ref)), radius
        assert np.array_equal(dev.image(), M.filtered_image(M.masked_totals(frames, counts), counts, w, h, radius))
        dev.close()


def test_variance_after_one_batch_is_nan_and_identical_samples_give_zero(handles):
    w, h = 13, 7
    scene, cam, g = handles("wall")
    p = make_params(w, h, 0, 1, seed=12)
    dev = rpt_amd.DeviceBuffer(g, w, h)
    dev.sample(cam, p)
    host = rpt_amd.Buffer(w, h)
    host.add_samples(g.render_batch(cam, p))
    assert math.isnan(dev.variance()) and math.isnan(host.variance())
    dev.close()
    # identical samples: the mean is exact, every deviation is 0 (dyadic values); 0.1 is not exact, and its tiny
    # variance must still be the reference's bits
    scene, cam, g = handles("emitter")
    for c, zero in (((0.375, 0.5, 0.0625), True), ((0.1, 0.7, 0.3), False)):
        g.set_objects([0], [emitter(c)])
        dev = rpt_amd.DeviceBuffer(g, 4, 3)
        host = rpt_amd.Buffer(4, 3)
        frames = []
        for k in range(3):
            pk = make_params(4, 3, 0, 1, seed=1, sample_index_base=k)
            dev.sample(cam, pk)
            frames.append(g.render_batch(cam, pk))
            host.add_samples(frames[-1])
        assert all((F == np.array(c)).all() for F in frames)
        v = dev.variance()
        assert M.bits(v) == M.bits(host.variance()) == M.bits(M.variance(frames, np.full(12, 3)))
        assert (v == 0.0) == zero, v
        dev.close()
    g.set_objects([0], [emitter((0.5, 0.5, 0.5))])
