"""Adaptive sampling without a GPU: the numpy model of the per-pixel statistics and the stopping rule, the host Buffer
with uneven per-pixel sample counts (Buffer::add_sample, buffer.rs:25-30) against a direct restatement of
buffer.rs:59-93, and the C ABI's argument checks of rptgpu_buffer_sample_adaptive."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi

import adaptive_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_welford_model_matches_the_two_pass_statistics():
    rng = np.random.default_rng(5)
    frames = [rng.random((50, 3)) * 2.0 for _ in range(7)]
    r = M.run(frames, min_batches=100, abs_tol=0.0, rel_tol=0.0)  # nothing retires
    assert (r["counts"] == 7).all() and r["active"] == [50] * 7
    stack = np.stack(frames)
    assert np.allclose(r["mean"], stack.mean(axis=0), rtol=1e-14, atol=0)
    ss = ((stack - stack.mean(axis=0)) ** 2).sum(axis=(0, 2))
    assert np.allclose(r["M2"], ss, rtol=1e-12, atol=1e-15)
    assert np.array_equal(r["totals"], M.masked_totals(frames, r["counts"]))


def test_stopping_rule_model():
    rng = np.random.default_rng(6)
    P = 400
    noise = np.where(np.arange(P) < 100, 0.0, np.where(np.arange(P) < 200, 1e-3, 0.5))
    frames = [np.full((P, 3), 0.25) + noise[:, None] * rng.standard_normal((P, 3)) for _ in range(8)]
    r = M.run(frames, min_batches=3, abs_tol=0.0, rel_tol=0.01)
    c = r["counts"]
    assert (c[:100] == 3).all()  # constant values: M2 == 0, they retire at exactly min_batches
    assert (c[100:200] == 3).all()  # tiny noise: well inside 1 %
    assert (c[200:] == 8).all()  # never
    assert r["active"][:2] == [P, P] and r["active"][2] == 200 and r["active"][-1] == 200
    # a NaN never retires; abs = rel = 0 retires only the zero-variance pixels
    frames[0][5] = np.nan
    r = M.run(frames, 2, 1e300, 0.0)
    assert r["counts"][5] == 8 and (np.delete(r["counts"], 5) == 2).all()
    r = M.run(frames, 2, 0.0, 0.0)
    assert (r["counts"][:5] == 2).all() and (r["counts"][100:] == 8).all()


def _uneven(seed, w, h, kmax):
    rng = np.random.default_rng(seed)
    frames = [rng.random((w * h, 3)) * 1.3 for _ in range(kmax)]
    frames[0][3] = [0.0, -0.0, 2.0]
    counts = rng.integers(1, kmax + 1, size=w * h)
    counts[0], counts[-1] = kmax, 1
    return frames, counts


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_add_sample_with_uneven_counts_is_the_reference_buffer(radius):
    w, h, kmax = 9, 7, 5
    frames, counts = _uneven(11 + radius, w, h, kmax)
    buf = rpt_amd.Buffer(w, h, rpt_amd.Filter.Box(radius))
    for k in range(kmax):  # round by round, as the adaptive device buffer adds them
        for p in np.nonzero(counts > k)[0]:
            buf.add_sample(p % w, p // w, frames[k][p])
    assert np.array_equal(buf.counts, counts)
    pix = M.pixel_lists(frames, counts)
    want = M.ref_filtered(pix, w, h, radius)
    assert np.array_equal(buf._filtered(), want)
    assert (buf.image() == rpt_amd.color.color_bytes(want)).all()
    v, rv = buf.variance(), M.ref_variance(pix)
    assert (np.isnan(v) and np.isnan(rv)) if np.isnan(rv) else v == rv


@pytest.mark.parametrize("w,h", [(9, 7), (1, 11), (11, 1), (2, 2), (3, 2)])
def test_vectorised_references_equal_the_per_pixel_ones(w, h):
    """filtered_image / variance (numpy, what the full-frame GPU tests use) against ref_filtered / ref_variance (Python
    floats, pixel by pixel): bit for bit, with uneven counts, all-zero pixels, every radius up to past the frame."""
    kmax = 5
    frames, counts = _uneven(40 + w * 13 + h, w, h, kmax)
    for F in frames:  # pixels whose samples are all zeros, of both signs
        F[(w * h) // 2] = [0.0, -0.0, 0.0]
    pix = M.pixel_lists(frames, counts)
    totals = M.masked_totals(frames, counts)
    for radius in sorted({0, 1, 2, 3, 4, max(w, h), w + h + 3}):
        want = M.ref_filtered(pix, w, h, radius)
        got = M.filtered_color(totals, counts, w, h, radius)
        assert np.array_equal(M.bits(got), M.bits(want)), radius
        assert np.array_equal(M.filtered_image(totals, counts, w, h, radius), rpt_amd.color.color_bytes(want))
    v, rv = M.variance(frames, counts), M.ref_variance(pix)  # some pixel has one sample: NaN
    assert np.isnan(v) and np.isnan(rv)
    counts2 = np.maximum(counts, 2)
    pix2 = M.pixel_lists(frames, counts2)
    v, rv = M.variance(frames, counts2), M.ref_variance(pix2)
    assert M.bits(v) == M.bits(rv)
    buf = rpt_amd.Buffer(w, h)
    for k in range(kmax):
        for p in np.nonzero(counts2 > k)[0]:
            buf.add_sample(p % w, p // w, frames[k][p])
    assert M.bits(buf.variance()) == M.bits(v)


def test_vectorised_variance_sums_the_pixels_in_order():
    """The pixel sum is sequential, as buffer.rs's loop: values whose pairwise sum rounds differently tell it apart."""
    P = 4096
    rng = np.random.default_rng(9)
    frames = [rng.random((P, 3)) * np.where(np.arange(P) % 3 == 0, 1e6, 1e-6)[:, None] for _ in range(3)]
    counts = rng.integers(2, 4, size=P)
    want = M.ref_variance(M.pixel_lists(frames, counts))
    assert M.bits(M.variance(frames, counts)) == M.bits(want)


def test_add_sample_order_and_add_samples_after_uneven_counts():
    """A pixel's samples keep their insertion order whatever the call: add_samples after add_sample appends each
    pixel's value at its own next position."""
    w, h = 4, 3
    rng = np.random.default_rng(3)
    a, b = rng.random((w * h, 3)), rng.random((w * h, 3))
    buf = rpt_amd.Buffer(w, h)
    buf.add_sample(1, 2, a[9])
    buf.add_samples(b)
    counts = np.ones(w * h, dtype=np.int64)
    counts[9] = 2
    assert np.array_equal(buf.counts, counts)
    pix = [[tuple(b[p])] for p in range(w * h)]
    pix[9] = [tuple(a[9]), tuple(b[9])]
    assert np.array_equal(buf._filtered(), M.ref_filtered(pix, w, h, 0))
    assert buf.variance() == M.ref_variance(pix) or np.isnan(buf.variance())


def test_add_samples_only_gives_the_same_bits_as_per_pixel_lists():
    w, h = 8, 5
    rng = np.random.default_rng(8)
    frames = [rng.random((w * h, 3)) for _ in range(4)]
    for radius in (0, 2):
        buf = rpt_amd.Buffer(w, h, rpt_amd.Filter.Box(radius))
        for f in frames:
            buf.add_samples(f)
        assert len(buf.samples) == 4
        pix = M.pixel_lists(frames, np.full(w * h, 4))
        assert np.array_equal(buf._filtered(), M.ref_filtered(pix, w, h, radius))
        assert buf.variance() == M.ref_variance(pix)


def test_invalid_pixel_location():
    buf = rpt_amd.Buffer(4, 3)
    for x, y in ((4, 0), (0, 3), (-1, 0)):
        with pytest.raises(AssertionError, match="Invalid pixel location"):
            buf.add_sample(x, y, (1.0, 1.0, 1.0))
    buf.add_sample(0, 0, (1.0, 1.0, 1.0))
    with pytest.raises(AssertionError, match="Pixel found with no samples"):
        buf.image()  # radius 0: the other pixels have none


def test_rpt_adaptive_size_matches_the_header(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu %zu %zu\\n", ' \
          'sizeof(RptAdaptive), offsetof(RptAdaptive, abs_tol), offsetof(RptAdaptive, rel_tol));return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    size, o1, o2 = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(_abi.RptAdaptive) == size == 24
    assert (_abi.RptAdaptive.abs_tol.offset, _abi.RptAdaptive.rel_tol.offset) == (o1, o2)


def test_adaptive_entry_points_refuse_bad_arguments_without_a_device():
    lib = _abi.load_library()
    E = _abi.RPTGPU_E_INVALID_ARGUMENT
    assert lib.rptgpu_buffer_sample_adaptive(None, None, None, None, None) == E
    assert b"RptAdaptive" in lib.rptgpu_last_error_detail(None)
    cam, params, n = _abi.RptCamera(), rpt_amd.make_params(8, 8, 1, 1), C.c_uint32(7)

    def call(a):
        return lib.rptgpu_buffer_sample_adaptive(None, C.byref(cam), C.byref(params), C.byref(a), C.byref(n))

    good = _abi.RptAdaptive(C.sizeof(_abi.RptAdaptive), 4, 0.0, 0.01)
    assert call(good) == E and b"null" in lib.rptgpu_last_error_detail(None)
    for field, value in (("struct_size", 16), ("struct_size", 32), ("min_batches", 1), ("min_batches", 0),
                         ("abs_tol", -1e-9), ("rel_tol", float("nan")), ("abs_tol", float("inf")), ("rel_tol", -0.5)):
        bad = _abi.RptAdaptive(good.struct_size, good.min_batches, good.abs_tol, good.rel_tol)
        setattr(bad, field, value)
        assert call(bad) == E, field
        assert field.encode() in lib.rptgpu_last_error_detail(None), field
    assert n.value == 7  # nothing written
    assert lib.rptgpu_buffer_sample_counts(None, None) == E
    assert lib.rptgpu_buffer_totals(None, None) == E
