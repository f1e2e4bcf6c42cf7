"""The two host-side halves of rptgpu_render_views that need no GPU: the piece planner of rpt_amd/csrc/render_plan.h,
compiled with g++ under AddressSanitizer and UBSan next to a driver that pins it (tests/cpp/views_piece_check.cpp), and
tests/views_model.py — the numpy restatement of the header's rays that tests/test_gpu_views.py holds the device to —
checked against what it is meant to say: a panorama's rays point where Hdri::get_color looks their texel up, and the
film coordinates are the oracle's camera's."""
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import Camera, make_params

import views_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 21  # odd, and no multiple of anything


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("views_piece") / "views_piece_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "views_piece_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover", "passes"])
def test_views_piece(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr


def test_a_panoramas_rays_point_at_their_texels(oracle):
    """Every sample of rows 1 .. height-2 of a 37x21 panorama: the direction pushed through Hdri::get_color's own mapping
    (environment.rs:27-30: atan2(z, x) + pi over width-1, acos(y) over height-1) gives back the (cx, cy) it was made
    from within 1e-6 texel, modulo the column wrap (columns 0 and width-1 are one meridian).  Rounding is around 1e-12
    texel at this size and a wrong quadrant or sign is off by at least a quarter of the width, so 1e-6 separates the two.
    The two pole rows are left out: there cos(elevation) -> 0 and atan2 of the direction is ill-conditioned."""
    seed, worst = 20261, 0.0
    for sample in range(3):
        o, d, cx, cy = M.panorama_rays(oracle, (1.0, -2.0, 0.5), seed, W, H, sample, M.host_sincos(oracle))
        assert (o == np.array([1.0, -2.0, 0.5])).all() and np.isfinite(d).all()
        assert cx.min() >= 0.0 and cx.max() <= W - 1 and cy.min() >= 0.0 and cy.max() <= H - 1
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 4e-16 * 4
        rows = np.arange(W * H) // W
        keep = (rows >= 1) & (rows <= H - 2)
        assert keep.sum() == W * (H - 2)  # exactly 2 rows left out
        n = d / np.linalg.norm(d, axis=1, keepdims=True)  # get_color normalises
        tx = (np.arctan2(n[:, 2], n[:, 0]) + np.pi) / (2.0 * np.pi) * (W - 1)
        ty = np.arccos(n[:, 1]) / np.pi * (H - 1)
        ex = np.abs(tx - cx)
        ex = np.minimum(ex, np.abs(ex - (W - 1)))  # the column wrap
        ey = np.abs(ty - cy)
        worst = max(worst, ex[keep].max(), ey[keep].max())
        assert ex[keep].max() <= 1e-6 and ey[keep].max() <= 1e-6, (sample, ex[keep].max(), ey[keep].max())
        # the samples do spread over their texel, on both sides of the wrap and over every quadrant
        assert (cx - np.arange(W * H) % W != 0).any() and (np.abs(cx / (W - 1) - 0.5) > 0.25).any()
    print("panorama: largest texel error %.3e" % worst)


def test_the_models_film_is_the_oracles_camera(oracle):
    """the perspective formula of the model (no lens) against oracle_camera_ray, bit for bit: the draws, the film
    coordinates and the vector arithmetic the two other projections share with it are then the reference's"""
    camera = Camera.look_at((0.5, 2.2, 7.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 0.7)
    for w, h, sample in ((W, H, 0), (23, 33, 5)):
        p = make_params(w, h, 1, 1, seed=99, sample_index_base=sample)
        o, d = M.perspective_rays(oracle, camera, 99, w, h, sample)
        for i in range(w * h):
            wo, wd = oracle.camera_ray(camera, p, i % w, i // w, sample)
            assert (o[i] == wo).all() and (d[i] == wd).all(), i


def test_an_orthographic_views_rays_are_parallel_and_span_the_scale(oracle):
    camera = Camera.look_at((0.5, 2.2, 7.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 0.7)
    o, d = M.orthographic_rays(oracle, camera, 2.5, 7, W, H, 0)
    eye, direction, up, right = M.camera_frame(camera)
    assert (d == d[0]).all() and abs(np.linalg.norm(d[0]) - 1.0) <= 4e-16
    rel = o - eye
    u, v = rel @ right, rel @ up
    assert np.abs(rel @ direction).max() <= 1e-12  # the origins lie in the plane through the eye
    # the longer side (37 pixels) spans [-2.5, 2.5]: pixel centres at +-(1 - 1/37) * 2.5, jitter at most half a pixel
    assert u.min() >= -2.5 - 1e-12 and u.max() <= 2.5 + 1e-12 and u.max() - u.min() >= 2.0 * 2.5 * (1.0 - 2.0 / W)
    assert v.max() <= 2.5 * H / W + 1e-12 and v.min() >= -2.5 * H / W - 1e-12
    assert u[0] < u[W - 1] and v[0] > v[-1]  # x to the right, the top row first
