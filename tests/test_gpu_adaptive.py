"""Adaptive sampling on the device-resident Buffer (rptgpu_buffer_sample_adaptive), on a real MI355X.

Random numbers are keyed by (pixel, sample index), so a pixel rendered in an adaptive round at sample_index_base B gets
bit for bit what a full-frame render at B gives it: every check below compares the adaptive buffer with plain
rptgpu_render_batch frames F_k (base k * s) and with the numpy model of the rule run over the same frames."""
import numpy as np
import pytest

import rpt_amd
from rpt_amd import GpuScene, _abi, make_params, scenes

import adaptive_model as M

pytestmark = pytest.mark.gpu

W, H = 80, 45
S = 2  # samples per round
K = 6  # rounds


@pytest.fixture(scope="module")
def gpus():
    cache = {}

    def get(name):
        if name not in cache:
            if name == "cornell":
                scene, cam, _ = scenes.cornell()
            elif name == "sphere":
                scene, cam, _ = scenes.sphere_scene()
            else:  # a deep mesh under an HDRI: the wavefront pipeline's scene
                scene, cam, _ = scenes.wine_glass(hdri_size=(256, 128), segments=24)
            cache[name] = (scene, cam, GpuScene(scene, 0))
        return cache[name]

    yield get
    for v in cache.values():
        v[2].close()


def params(k, bounces=3, flags=0, seed=21, s=S):
    return make_params(W, H, bounces, s, seed=seed, sample_index_base=k * s, exposure_value=0.5, flags=flags)


def frames_of(g, cam, n, **kw):
    return [g.render_batch(cam, params(k, **kw)) for k in range(n)]


bits = M.bits
check_against = M.check_against


def mixed_tolerance(frames, min_batches):
    """a relative tolerance under which the model retires some pixels, but not all, within the rounds"""
    for rel in (0.3, 0.2, 0.1, 0.05, 0.5, 1.0, 0.02):
        r = M.run(frames, min_batches, 0.0, rel)
        if 0 < r["active"][-1] < len(frames[0]):
            return rel, r
    raise AssertionError("no tolerance gives a mix of retired and active pixels")


def adaptive(g, cam, n, min_batches, abs_tol, rel_tol, radius=0, **kw):
    dev = rpt_amd.DeviceBuffer(g, W, H, rpt_amd.Filter.Box(radius))
    left = [dev.sample_adaptive(cam, params(k, **kw), min_batches, abs_tol, rel_tol) for k in range(n)]
    return dev, left


@pytest.mark.parametrize("flags", [_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT, _abi.RPT_FLAG_GENERAL_TRAVERSAL])
def test_prefix_exactness_image_and_variance(gpus, flags):
    scene, cam, g = gpus("cornell")
    frames = frames_of(g, cam, K, flags=flags)
    rel, r = mixed_tolerance(frames, 3)
    for radius in (0, 1, 2):
        dev, left = adaptive(g, cam, K, 3, 0.0, rel, radius, flags=flags)
        counts = check_against(dev, left, frames, r)
        host = rpt_amd.Buffer(W, H, rpt_amd.Filter.Box(radius))
        for k in range(K):
            for p in np.nonzero(counts > k)[0]:
                host.add_sample(p % W, p // W, frames[k][p])
        assert (dev.image() == host.image()).all()
        want = M.ref_variance(M.pixel_lists(frames, counts))
        v = dev.variance()
        assert abs(v - want) <= 1e-15 * abs(want) and abs(host.variance() - want) <= 1e-15 * abs(want)
        with pytest.raises(rpt_amd.RptGpuError) as e:  # a full-frame batch after a retirement
            dev.sample(cam, params(K, flags=flags))
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT
        dev.close()


def test_wavefront_scene_and_a_list_of_one_pixel(gpus):
    """The deep-mesh scene (wavefront pipeline by default) and both forced pipelines, down to a list of ONE pixel: the
    absolute tolerance is chosen from the model so that exactly one pixel survives round min_batches."""
    for name, flags in (("wine_glass", 0), ("cornell", _abi.RPT_FLAG_PERSISTENT), ("cornell", _abi.RPT_FLAG_WAVEFRONT)):
        scene, cam, g = gpus(name)
        frames = frames_of(g, cam, 5, flags=flags)
        mb = 2
        r2 = M.run(frames[:mb], mb, 0.0, 0.0)  # nothing but exact constants retires: e of every pixel at n = 2
        n2 = np.full(len(r2["counts"]), 2.0)
        e = np.sort((r2["M2"] / (n2 - 1.0)) / n2)
        assert e[-1] > e[-2] >= 0.0
        tol = float(np.sqrt(0.5 * (e[-1] + e[-2])))
        r = M.run(frames, mb, tol, 0.0)
        assert r["active"][mb - 1] == 1, r["active"]
        dev, left = adaptive(g, cam, 5, mb, tol, 0.0, flags=flags)
        check_against(dev, left, frames, r)
        dev.close()


def test_sky_pixels_retire_at_min_batches_and_zero_tolerance(gpus):
    scene, cam, g = gpus("sphere")  # default environment: constant black
    frames = frames_of(g, cam, K)
    sky = np.all([np.all(F == 0.0, axis=1) for F in frames], axis=0)
    assert 0 < sky.sum() < W * H
    for mb in (2, 4):
        r = M.run(frames, mb, 0.0, 0.0)
        dev, left = adaptive(g, cam, K, mb, 0.0, 0.0)
        counts = check_against(dev, left, frames, r)
        assert (counts[sky] == mb).all()
        # every pixel that did not retire has what the same number of plain batches gives it
        plain = rpt_amd.DeviceBuffer(g, W, H)
        for k in range(K):
            plain.sample(cam, params(k))
        full = counts == K
        assert full.sum() > 0
        assert np.array_equal(bits(dev.totals().reshape(-1, 3)[full]), bits(plain.totals().reshape(-1, 3)[full]))
        assert (plain.sample_counts() == K).all()
        dev.close()
        plain.close()


def test_everything_retires_then_nothing_is_recorded(gpus):
    scene, cam, g = gpus("cornell")
    dev = rpt_amd.DeviceBuffer(g, W, H)
    dev.sample(cam, params(0))  # plain batches mix in while every pixel is active
    assert dev.sample_adaptive(cam, params(1), 2, 1e300, 0.0) == 0
    assert dev.num_batches() == 2 and (dev.sample_counts() == 2).all()
    assert dev.sample_adaptive(cam, params(2), 2, 1e300, 0.0) == 0
    assert dev.num_batches() == 2 and (dev.sample_counts() == 2).all()
    F = frames_of(g, cam, 2)
    assert np.array_equal(bits(dev.totals().reshape(-1, 3)), bits(M.masked_totals(F, np.full(W * H, 2))))
    with pytest.raises(rpt_amd.RptGpuError):
        dev.sample(cam, params(3))
    with pytest.raises(rpt_amd.RptGpuError):  # multi-GPU parts are out of scope
        dev.sample_adaptive(cam, make_params(W, H, 3, S, part=(0, 2)), 2, 0.0, 0.0)
    with pytest.raises(rpt_amd.RptGpuError):
        dev.sample_adaptive(cam, make_params(W + 1, H, 3, S), 2, 0.0, 0.0)
    dev.close()


def test_plain_render_after_adaptive_rounds_uses_the_full_partition(gpus):
    """The adaptive rounds render a list of their own; the handle's cached partition stays what plain renders use."""
    scene, cam, g = gpus("cornell")
    before = g.render_batch(cam, params(0))
    dev, left = adaptive(g, cam, 4, 2, 0.0, 0.3)
    assert left[-1] < W * H
    assert np.array_equal(bits(g.render_batch(cam, params(0))), bits(before))
    dev.close()


def test_adaptive_totals_equal_the_oracle(gpus, oracle):
    scene, cam, g = gpus("cornell")
    frames = frames_of(g, cam, 4)
    rel, r = mixed_tolerance(frames, 2)
    dev, left = adaptive(g, cam, 4, 2, 0.0, rel)
    counts = dev.sample_counts().ravel()
    osc = oracle.OracleScene(scene)
    ref = [osc.render(cam, params(k), threads=0) for k in range(4)]
    assert 0 < left[-1] < W * H
    assert (dev.totals().reshape(-1, 3) == M.masked_totals(ref, counts)).all()
    dev.close()


def test_renderer_adaptive_render(gpus):
    scene, cam, g = gpus("cornell")
    seen = []
    r = rpt_amd.Renderer(scene, cam).width(W).height(H).max_bounces(3).num_samples(12).seed(4).with_gpu_scene(g)
    img = r.adaptive_render(2, lambda it, buf, active: seen.append((it, active, buf.sample_counts().copy())),
                            min_batches=2, rel_tol=0.3)
    assert img.shape == (H, W, 3) and img.dtype == np.uint8
    its = [s[0] for s in seen]
    assert its == list(range(2, 2 * len(seen) + 1, 2)) and its[-1] <= 12
    assert all(a >= b for a, b in zip([s[1] for s in seen], [s[1] for s in seen][1:]))
    assert seen[-1][1] == 0 or its[-1] == 12
    # the same rounds by hand: same image
    dev = rpt_amd.DeviceBuffer(g, W, H)
    for k in range(len(seen)):
        dev.sample_adaptive(cam, make_params(W, H, 3, 2, seed=4, sample_index_base=2 * k), 2, 0.0, 0.3)
    assert (dev.image() == img).all()
    dev.close()
