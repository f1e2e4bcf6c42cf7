"""rptgpu_buffer_features / _feature_sums / _denoise on a real MI355X against the numpy model of
tests/denoise_model.py.  Every comparison of the filter is on the raw bits (f64 viewed as uint64), tolerance 0, over every
pixel.  The model's inputs are the buffer's own batches (re-rendered by rptgpu_render_batch: a pixel's batch is keyed by
(pixel, sample index) alone) folded by the model's Welford, and the held feature sums, which are first shown to be
rptgpu_render_aov's."""
import ctypes as C

import numpy as np
import pytest

import rpt_amd
from rpt_amd import DeviceBuffer, Filter, GpuScene, Renderer, _abi, make_params, scenes
from rpt_amd.color import color_bytes

import adaptive_model
import aov_model
import denoise_model as M
import small_scenes

pytestmark = pytest.mark.gpu

E = _abi.RPTGPU_E_INVALID_ARGUMENT
CH = _abi.RPT_AOV_DEPTH | _abi.RPT_AOV_NORMAL | _abi.RPT_AOV_ALBEDO | _abi.RPT_AOV_POSITION


def filled(scene, camera, w, h, bounces, batches, spp, seed, fspp=4, flags=0, radius=0):
    """a GpuScene, a DeviceBuffer with `batches` batches of spp samples and features from fspp samples, and the batches
    as frames (H, W, 3)"""
    g = GpuScene(scene, 0)
    buf = DeviceBuffer(g, w, h, Filter.Box(radius) if radius else None)
    frames = []
    for b in range(batches):
        p = make_params(w, h, bounces, spp, seed=seed, sample_index_base=b * spp)
        buf.sample(camera, p)
        frames.append(g.render_batch(camera, p).reshape(h, w, 3))
    if fspp:
        buf.features(camera, make_params(w, h, bounces, fspp, seed=seed, flags=flags))
    return g, buf, frames


def same_bits(got, want, what):
    diff = M.bits(got) != M.bits(want)
    if diff.any():
        print("%s: %d of %d values differ, max |delta| = %r" % (what, int(diff.sum()), diff.size,
                                                                  float(np.nanmax(np.abs(got - want)))))
    return not diff.any()


def model_of(buf, frames, counts=None, **kw):
    total, counts, M2 = M.welford(frames, counts)
    assert np.array_equal(M.bits(total), M.bits(buf.totals()))  # the model starts from what the buffer holds
    return M.denoise(total, counts, M2, buf.feature_sums(), **kw)


@pytest.mark.parametrize("name,flags", [("cornell", 0), ("cornell", _abi.RPT_FLAG_WAVEFRONT), ("wine_glass", 0),
                                        ("wine_glass", _abi.RPT_FLAG_WAVEFRONT), ("glass", 0)])
def test_held_features_are_render_aovs(name, flags):
    scene, camera, p0 = small_scenes.small(name)
    w, h = p0.width, p0.height
    g = GpuScene(scene, 0)
    buf = DeviceBuffer(g, w, h)
    first = make_params(w, h, 1, 3, seed=p0.seed, sample_index_base=2, flags=flags)
    buf.features(camera, first)
    got = buf.feature_sums()
    want = g.render_aov(camera, first, CH)
    assert sorted(got) == sorted(want) and want["hits"].sum() > 0
    assert aov_model.mismatches(got, want) == []
    # a second call replaces, it does not accumulate
    second = make_params(w, h, 1, 2, seed=p0.seed + 1, flags=flags)
    buf.features(camera, second)
    got2 = buf.feature_sums()
    assert aov_model.mismatches(got2, g.render_aov(camera, second, CH)) == []
    assert aov_model.mismatches(got2, want) != []
    buf.close()
    g.close()


CASES = [("cornell", 96, 72, 3), ("cornell", 96, 72, 1), ("cornell", 96, 72, 5), ("cornell", 96, 72, 8),
         ("spheres", 96, 72, 3), ("glass", 96, 72, 3), ("wine_glass", 96, 72, 3), ("dragon", 63, 65, 5),
         ("cornell", 63, 65, 3), ("glass", 1, 37, 3), ("cornell", 37, 1, 3), ("spheres", 7, 5, 8), ("glass", 7, 5, 3)]


@pytest.mark.parametrize("name,w,h,levels", CASES)
def test_denoise_equals_the_model_bit_for_bit(name, w, h, levels):
    scene, camera, p0 = small_scenes.small(name)
    g, buf, frames = filled(scene, camera, w, h, 4, 4, 2, p0.seed)
    feats = buf.feature_sums()
    if name == "glass" and w * h > 100:
        assert (feats["hits"] == 0).any() and (feats["hits"] > 0).any()  # sky and surface
    want = model_of(buf, frames, levels=levels)
    got = buf.denoise(levels=levels)
    assert got.shape == (h, w, 3)
    assert same_bits(got, want, "%s %dx%d levels %d" % (name, w, h, levels))
    if w * h > 100:
        raw = buf.totals() / 4.0
        assert not np.array_equal(M.bits(got), M.bits(raw))  # it did filter
    # the bytes are color_bytes of the linear frame; either output alone gives the same
    assert np.array_equal(buf.denoised_image(levels=levels), color_bytes(got))
    d = _abi.RptDenoise(C.sizeof(_abi.RptDenoise), levels, 2.0, 0.1, 0.01, 0.1)
    lin, rgb = np.empty((h, w, 3)), np.empty((h, w, 3), dtype=np.uint8)
    _abi.check(g.lib.rptgpu_buffer_denoise(buf.handle, C.byref(d), lin.ctypes.data_as(C.POINTER(C.c_double)),
                                           rgb.ctypes.data_as(C.POINTER(C.c_uint8))), g.handle)
    assert np.array_equal(M.bits(lin), M.bits(got)) and np.array_equal(rgb, color_bytes(got))
    buf.close()
    g.close()


def test_other_sigmas_and_the_wavefront_features():
    scene, camera, p0 = small_scenes.small("wine_glass")
    g, buf, frames = filled(scene, camera, 64, 36, 4, 3, 2, p0.seed, fspp=2, flags=_abi.RPT_FLAG_WAVEFRONT)
    kw = dict(levels=2, sigma_color=0.7, sigma_normal=0.33, sigma_depth=0.05, sigma_albedo=1.5)
    assert same_bits(buf.denoise(**kw), model_of(buf, frames, **kw), "wine_glass, other sigmas")
    buf.close()
    g.close()


def test_a_buffer_with_retired_pixels():
    scene, camera, p0 = small_scenes.small("cornell")
    w, h, spp = 96, 72, 2
    g = GpuScene(scene, 0)
    buf = DeviceBuffer(g, w, h)
    frames, left = [], []
    for b in range(6):
        p = make_params(w, h, 4, spp, seed=p0.seed, sample_index_base=b * spp)
        left.append(buf.sample_adaptive(camera, p, min_batches=2, abs_tol=0.005, rel_tol=0.02))
        frames.append(g.render_batch(camera, p).reshape(h, w, 3))
    counts = buf.sample_counts()
    print("active after each round:", left, "counts", counts.min(), counts.max())
    assert 2 <= counts.min() < counts.max() <= 6  # uneven n_p: some pixels retired early, others went on
    buf.features(camera, make_params(w, h, 4, 4, seed=p0.seed))
    for levels in (1, 3):
        assert same_bits(buf.denoise(levels=levels), model_of(buf, frames, counts, levels=levels), "retired, levels %d" % levels)
    buf.close()
    g.close()


def test_the_buffer_is_untouched():
    scene, camera, p0 = small_scenes.small("spheres")
    g, buf, frames = filled(scene, camera, 64, 48, 4, 3, 2, p0.seed, radius=1)

    def state():
        f = buf.feature_sums()
        return [buf.image(), np.float64(buf.variance()), buf.totals(), buf.sample_counts(), buf.num_batches()] + \
               [f[k] for k in sorted(f)]

    before = state()
    a = buf.denoise()
    buf.denoised_image(levels=5)
    b = buf.denoise()
    after = state()
    for x, y in zip(before, after):
        same = np.array_equal(M.bits(x), M.bits(y)) if np.asarray(x).dtype == np.float64 else np.array_equal(x, y)
        assert same
    assert np.array_equal(M.bits(a), M.bits(b))
    # and sampling goes on afterwards, the filter following it
    p = make_params(64, 48, 4, 2, seed=p0.seed, sample_index_base=6)
    buf.sample(camera, p)
    frames.append(g.render_batch(camera, p).reshape(48, 64, 3))
    assert same_bits(buf.denoise(), model_of(buf, frames), "after one more batch")
    buf.close()
    g.close()


def test_device_side_refusals():
    scene, camera, p0 = small_scenes.small("sphere")
    w, h = 32, 20
    g = GpuScene(scene, 0)
    buf = DeviceBuffer(g, w, h)

    def refused(fn, word):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            fn()
        assert e.value.code == E and word in str(e.value), str(e.value)

    good = make_params(w, h, 1, 2, seed=3)
    refused(buf.denoise, "features")
    refused(buf.feature_sums, "features")
    refused(lambda: buf.features(camera, make_params(w + 1, h, 1, 2)), "dimension")
    refused(lambda: buf.features(camera, make_params(w, h - 1, 1, 2)), "dimension")
    refused(lambda: buf.features(camera, make_params(w, h, 1, 2, part=(0, 2))), "part_count")
    refused(lambda: buf.features(camera, make_params(w, h, 1, 0)), "iterations")
    refused(lambda: buf.features(camera, make_params(w, h, 1, 2, precision=1)), "precision_mode")
    refused(buf.denoise, "features")  # a refused call left none behind
    buf.features(camera, good)
    refused(buf.denoise, "two batches")  # no batch at all
    buf.sample(camera, good)
    refused(buf.denoise, "two batches")  # one batch: no variance
    refused(lambda: buf.denoise(levels=9), "levels")
    refused(lambda: buf.denoise(sigma_depth=0.0), "sigma")
    d = _abi.RptDenoise(C.sizeof(_abi.RptDenoise), 3, 2.0, 0.1, 0.01, 0.1)
    assert g.lib.rptgpu_buffer_denoise(buf.handle, C.byref(d), None, None) == E
    assert b"both NULL" in g.lib.rptgpu_last_error_detail(g.handle)
    buf.sample(camera, make_params(w, h, 1, 2, seed=3, sample_index_base=2))
    assert buf.denoise().shape == (h, w, 3)
    buf.close()
    g.close()


def rmse(a, ref):
    return float(np.sqrt(np.mean((np.minimum(a, 4.0) - np.minimum(ref, 4.0)) ** 2)))


@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_it_denoises(name, oracle):
    """The issue's two configurations: 96x72, 4 bounces, 8 batches of 2 spp, seed 11, features from 4 spp, the default
    filter; reference = the oracle at 1024 spp with another seed; values clamped at 4.0.  The denoised frame must beat
    the Box(1) frame of the same buffer and 0.75 x the raw frame's RMSE."""
    scene, camera = getattr(scenes, name)()[:2]
    w, h = 96, 72
    g, buf, frames = filled(scene, camera, w, h, 4, 8, 2, 11)
    den = buf.denoise()
    totals, counts = buf.totals(), buf.sample_counts()
    buf.close()
    g.close()
    ref = oracle.OracleScene(scene).render(camera, make_params(w, h, 4, 1024, seed=9999)).reshape(h, w, 3)
    raw = totals / counts[..., None]
    box = adaptive_model.filtered_color(totals.reshape(-1, 3), counts.reshape(-1), w, h, 1)
    r_raw, r_box, r_den = rmse(raw, ref), rmse(box, ref), rmse(den, ref)
    print("%s: RMSE raw %.5f  Box(1) %.5f (%.3fx)  denoised %.5f (%.3fx)" % (name, r_raw, r_box, r_box / r_raw, r_den, r_den / r_raw))
    assert r_den < r_box
    assert r_den < 0.75 * r_raw


def test_renderer_denoised_render():
    scene, camera, p0 = small_scenes.small("cornell")
    r = Renderer(scene, camera).width(64).height(36).max_bounces(4).num_samples(8).seed(p0.seed)
    img = r.denoised_render(2, feature_samples=4, levels=2)
    g, buf, _ = filled(scene, camera, 64, 36, 4, 4, 2, p0.seed)
    assert img.dtype == np.uint8 and np.array_equal(img, buf.denoised_image(levels=2))
    buf.close()
    g.close()
    with pytest.raises(ValueError):
        r.denoised_render(8)


def test_full_hd_against_the_model():
    """1920x1080, 3 levels, every pixel (the model is vectorised over the frame and walks the taps in a Python loop)."""
    scene, camera, _ = scenes.cornell()
    w, h = 1920, 1080
    g, buf, frames = filled(scene, camera, w, h, 2, 3, 1, 0xC2, fspp=2)
    want = model_of(buf, frames, levels=3)
    got = buf.denoise(levels=3)
    assert same_bits(got, want, "1920x1080")
    assert np.array_equal(buf.denoised_image(levels=3), color_bytes(got))
    buf.close()
    g.close()
