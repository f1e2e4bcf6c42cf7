"""The pre-trace pass of rpt_paths<KdFlat, false, true> (kernels/paths_flat.inc cull_skip_mask, RPT_PRETRACE_CULL) on a real
MI355X: under a pinhole camera a wave none of whose pending pixels lies in a cube's screen rectangle (host_scene.cpp
pinhole_screen_rect) leaves that cube's exact test out of the pass.  A skipped test is one that would have rejected, so
every frame must equal the oracle's BIT for bit, with the oracle's closest-hit and shadow ray counts (a skipped object
test is not a ray), through the fused kernel: Cornell with the camera as shipped, looking at walls only (both cubes off
screen: every wave skips them; and from between the cubes' top and bottom, where they have no rectangle), close on a
cube (no wave skips), at odd frame sizes where the cubes' silhouettes cross the 32x8 tiles, with a lens (no rectangles),
and after a cube moved on a live handle (the rectangles follow)."""
import math
import os

import numpy as np
import pytest

from rpt_amd import Camera, GpuScene, Material, Object, _abi, cube, hex_color, make_params, scenes

pytestmark = pytest.mark.gpu

PERSISTENT = _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_PROFILE_KERNELS
FUSED = "shadow and bounce rays in one query"


def params(w, h, b, spp, **kw):
    return make_params(w, h, b, spp, seed=kw.pop("seed", 29), flags=PERSISTENT, **kw)


def check(g, osc, cam, p):
    g.reset_stats()
    img = g.render_batch(cam, p)
    st = g.stats()
    ref, cnt = osc.render(cam, p, threads=0, counters=True)
    assert st.kernel_launches[_abi.RPT_K_PATHS] >= 1  # the persistent kernel ran
    assert (img.view(np.int64) == ref.view(np.int64)).all(), (p.width, p.height, p.max_bounces, np.abs(img - ref).max())
    assert st.extend_rays == cnt["closest_rays"], (st.extend_rays, cnt["closest_rays"])
    assert st.shadow_rays == cnt["shadow_rays"], (st.shadow_rays, cnt["shadow_rays"])
    return img


def assert_fused(g, cam, capfd):
    """the launch diagnostics (RPTGPU_PRINT_LAUNCH) of one small render name the fused kernel"""
    capfd.readouterr()
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    try:
        g.render_batch(cam, params(16, 9, 2, 1))
    finally:
        del os.environ["RPTGPU_PRINT_LAUNCH"]
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]
    assert lines and all(FUSED in ln for ln in lines), lines


@pytest.fixture(scope="module")
def c2(oracle):
    scene, cam, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    yield scene, cam, g, oracle.OracleScene(scene)
    g.close()


def test_camera_as_shipped(c2, capfd):
    _, cam, g, osc = c2
    assert_fused(g, cam, capfd)
    check(g, osc, cam, params(128, 72, 8, 8))
    check(g, osc, cam, params(192, 108, 3, 5, seed=4))


def test_walls_only_every_wave_skips_the_cubes(c2, capfd):
    """towards the upper corner of the back and left walls, narrow: both cubes' rectangles are off screen"""
    _, _, g, osc = c2
    cam = Camera.look_at((278.0, 273.0, -800.0), (545.0, 480.0, 300.0), (0.0, 1.0, 0.0), 0.12)
    assert_fused(g, cam, capfd)
    check(g, osc, cam, params(128, 72, 8, 8))
    check(g, osc, cam, params(64, 40, 0, 6))
    # straight up from between the tall cube's top and bottom: the cubes straddle the eye's plane (no rectangle: always
    # tested), no camera ray comes near them, later bounces do
    cam = Camera(eye=(278.0, 300.0, 100.0), direction=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0), fov=0.686)
    check(g, osc, cam, params(128, 72, 8, 8))


def test_close_on_the_tall_cube_no_wave_skips(c2, capfd):
    _, _, g, osc = c2
    cam = Camera.look_at((278.0, 273.0, -800.0), (368.0, 165.0, 351.0), (0.0, 1.0, 0.0), 0.08)
    assert_fused(g, cam, capfd)
    img = check(g, osc, cam, params(128, 72, 8, 8))
    assert np.isfinite(img).all()
    # inside the small cube's box region too: the camera in the room, a metre from the small cube
    cam = Camera.look_at((185.0, 300.0, -50.0), (185.0, 82.5, 169.0), (0.0, 1.0, 0.0), 0.5)
    check(g, osc, cam, params(96, 54, 8, 6))


@pytest.mark.parametrize("size", [(97, 55), (161, 91), (33, 17)])
def test_silhouettes_cross_tile_edges_at_odd_sizes(c2, size):
    _, cam, g, osc = c2
    check(g, osc, cam, params(size[0], size[1], 8, 7))
    # a tile partition: the lanes of a wave hold pixels of this part's tiles only
    acc = None
    for i in range(3):
        img = check(g, osc, cam, params(size[0], size[1], 4, 3, tile=(32, 8), part=(i, 3)))
        acc = img if acc is None else acc + img
    assert (acc == check(g, osc, cam, params(size[0], size[1], 4, 3))).all()


def test_lens_camera_takes_the_stashed_origins(c2, capfd):
    """aperture > 0: every lane has its own origin on the lens"""
    _, _, g, osc = c2
    cam = Camera(eye=(278.0, 273.0, -800.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=0.686)
    cam.focus((278.0, 273.0, 280.0), 25.0)
    assert cam.aperture > 0.0
    assert_fused(g, cam, capfd)
    check(g, osc, cam, params(128, 72, 8, 8))
    check(g, osc, cam, params(97, 55, 2, 5, seed=8))


def test_cube_moved_on_a_live_handle(oracle, capfd):
    """set_objects moves the tall cube out of the creation's rectangle, and back: the rectangles are the render's"""
    scene, cam, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    try:
        first = check(g, oracle.OracleScene(scene), cam, params(128, 72, 8, 6))
        two_pi = 2.0 * math.pi
        white = Material.diffuse(hex_color(0xAAAAAA))
        was = scene.objects[5]
        for at, angle in (((150.0, 165.0, 420.0), -300.0), ((278.0, 165.0, 125.0), -253.0)):
            scene.objects[5] = Object(cube().scale((165.0, 330.0, 165.0)).rotate_y(two_pi * (angle / 360.0))
                                      .translate(at)).material(white)
            g.set_objects([5], [scene.objects[5]])
            assert_fused(g, cam, capfd)
            img = check(g, oracle.OracleScene(scene), cam, params(128, 72, 8, 6))
            assert not (img == first).all()  # (the moved cube is in view)
        scene.objects[5] = was
        g.update(scene)
        assert (check(g, oracle.OracleScene(scene), cam, params(128, 72, 8, 6)) == first).all()
    finally:
        g.close()
