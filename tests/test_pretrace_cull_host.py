"""The pre-trace cull's screen rectangles (rpt_amd/csrc/host_scene.cpp pinhole_screen_rect), checked without a GPU: the
PRODUCT's flattener and rectangle function, compiled with g++ next to a small C++ driver
(tests/cpp/pretrace_cull_host.cpp), give the rectangles of the Cornell box's cubes for a camera; then for random pixels
and samples the ORACLE's pinhole camera ray goes to the ORACLE's exact cube test: whenever the pixel is outside a cube's
rectangle — the conservative test says "miss", the kernel may skip the cube — the exact test must reject.  Also: the
rectangles are not vacuous (most outside pixels, many hits inside), and a lens gets none."""
import os
import subprocess

import numpy as np
import pytest

from rpt_amd import Camera, _abi, make_params, scenes
from oracle import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAMERAS = {
    "shipped": (lambda: scenes.cornell()[1], (1920, 1080)),
    "odd": (lambda: scenes.cornell()[1], (97, 55)),
    "close": (lambda: Camera.look_at((278.0, 273.0, -800.0), (368.0, 165.0, 351.0), (0.0, 1.0, 0.0), 0.08), (128, 72)),
    "walls": (lambda: Camera.look_at((278.0, 273.0, -800.0), (545.0, 480.0, 300.0), (0.0, 1.0, 0.0), 0.12), (128, 72)),
    "oblique": (lambda: Camera.look_at((900.0, 700.0, -300.0), (250.0, 150.0, 250.0), (0.1, 1.0, 0.05), 0.9), (333, 211)),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cull") / "pretrace_cull_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "pretrace_cull_host.cpp"),
                           os.path.join(ROOT, "rpt_amd", "csrc", "host_scene.cpp"), "-o", exe, "-lpthread"])
    return exe


def rectangles(exe, cam, w, h):
    args = [repr(float(v)) for v in list(cam.eye) + list(cam.direction) + list(cam.up)] + [repr(cam.fov), str(w), str(h)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    head = out[0].split()
    assert head[:2] == ["rc", "0"] and head[3] == "1" and head[5] == "7" and int(head[7], 16) == 0, out[0]
    assert out[-1].split() == ["lens", "got", "0"]
    rects = {}
    for line in out[1:8]:
        f = line.split()
        rects[int(f[1])] = (int(f[5]), int(f[7]), int(f[8]), int(f[10]), int(f[11]))
    return rects


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_a_pixel_outside_a_cubes_rectangle_cannot_hit_the_cube(driver, name):
    make, (w, h) = CAMERAS[name]
    cam = make()
    rects = rectangles(driver, cam, w, h)
    scene = scenes.cornell()[0]
    p = make_params(w, h, 8, 64, seed=0xC0FFEE, flags=_abi.RPT_FLAG_PERSISTENT)
    rng = np.random.default_rng(5)
    n = 6000
    xs, ys, ss = rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, 64, n)
    for k in (5, 6):
        got, x0, x1, y0, y1 = rects[k]
        assert got == 1  # every camera here has the cubes in front of it
        # half of the pixels from a band around the rectangle, where a wrong edge would show
        if x0 <= x1:
            bx = np.clip(rng.integers(x0 - 6, x1 + 7, n // 2), 0, w - 1)
            by = np.clip(rng.integers(y0 - 6, y1 + 7, n // 2), 0, h - 1)
            edge = rng.integers(0, 4, n // 2)
            bx = np.where(edge == 0, np.clip(x0 - 1 - rng.integers(0, 3, n // 2), 0, w - 1), np.where(edge == 1, np.clip(x1 + 1 + rng.integers(0, 3, n // 2), 0, w - 1), bx))
            by = np.where(edge == 2, np.clip(y0 - 1 - rng.integers(0, 3, n // 2), 0, h - 1), np.where(edge == 3, np.clip(y1 + 1 + rng.integers(0, 3, n // 2), 0, h - 1), by))
            px, py = np.concatenate([xs[: n // 2], bx]), np.concatenate([ys[: n // 2], by])
        else:
            px, py = xs, ys
        shape = scene.objects[k].shape
        outside = hits_inside = 0
        for x, y, s in zip(px, py, ss):
            o, d = O.camera_ray(cam, p, int(x), int(y), int(s))[:2]
            hit = O.shape_intersect(shape, o, d, t_min=1e-12)[0]
            inside = x0 <= x <= x1 and y0 <= y <= y1
            if not inside:
                outside += 1
                assert not hit, (name, k, int(x), int(y), int(s), rects[k])
            elif hit:
                hits_inside += 1
        covers = x0 <= x1 and (x1 - x0 + 1) * (y1 - y0 + 1) > 0.9 * w * h  # ("close": the tall cube fills the frame)
        assert covers or outside > n // 20
        if name in ("shipped", "odd"):
            assert hits_inside > n // 20  # (both cubes well in view: the rectangle is about the cube, not the whole frame)
        if name == "walls":
            assert x0 > x1 and y0 > y1  # off screen


def test_no_rectangle_when_a_corner_is_not_in_front_of_the_eye(driver):
    cam = Camera(eye=(278.0, 300.0, 100.0), direction=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0), fov=0.686)
    rects = rectangles(driver, cam, 128, 72)
    assert rects[5][0] == 0 and rects[6][0] == 0
    assert rects[1] == (1, 0, 127, 0, 71)  # the ceiling fills the frame
