"""rpt_paths<KdFlat, false, true> (kernels/paths.inc FUSE, paths_flat.inc flat_query2) on a real MI355X: a hit's shadow ray and bounce
ray are traced in one two-ray query, after illuminate, sample_f and both bsdf evaluations.  Every frame is compared BIT
for bit with the oracle through the persistent kernel, with the closest-hit and shadow ray counts equal to the oracle's:
C2 at small odd sizes and bounces 0-8, sample counts that are not a multiple of the work item's chunk, later sample
batches and a tile partition, a point light (a finite distance through illuminate's other branch), a glass cube (sample_f
returns None: the bounce slot is off while the shadow ray runs), and scenes with two lights or an ambient one, which
keep the one-ray kernel and must match all the same."""
import math
import os

import numpy as np
import pytest

from rpt_amd import Camera, GpuScene, Light, Material, Object, Scene, _abi, cube, hex_color, make_params, polygon, scenes

pytestmark = pytest.mark.gpu

PERSISTENT = _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_PROFILE_KERNELS
FUSED = "shadow and bounce rays in one query"


def cornell_variant(light="quad", glass=False, extra_light=None):
    """examples/cornell.rs with the light swapped or joined by another, or the small box made of glass."""
    scene = Scene()
    white = Material.diffuse(hex_color(0xAAAAAA))
    red = Material.diffuse(hex_color(0xBC0000))
    green = Material.diffuse(hex_color(0x00BC00))
    walls = [
        [(0.0, 0.0, 0.0), (0.0, 0.0, 559.2), (556.0, 0.0, 559.2), (556.0, 0.0, 0.0)],
        [(0.0, 548.9, 0.0), (556.0, 548.9, 0.0), (556.0, 548.9, 559.2), (0.0, 548.9, 559.2)],
        [(0.0, 0.0, 559.2), (0.0, 548.9, 559.2), (556.0, 548.9, 559.2), (556.0, 0.0, 559.2)],
        [(556.0, 0.0, 0.0), (556.0, 0.0, 559.2), (556.0, 548.9, 559.2), (556.0, 548.9, 0.0)],
        [(0.0, 0.0, 0.0), (0.0, 548.9, 0.0), (0.0, 548.9, 559.2), (0.0, 0.0, 559.2)],
    ]
    for pts, m in zip(walls, (white, white, white, red, green)):
        scene.add(Object(polygon(pts)).material(m))
    two_pi = 2.0 * math.pi
    scene.add(Object(cube().scale((165.0, 330.0, 165.0)).rotate_y(two_pi * (-253.0 / 360.0))
                     .translate((368.0, 165.0, 351.0))).material(white))
    small = Material.clear(1.5, 0.0) if glass else white
    scene.add(Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(two_pi * (-197.0 / 360.0))
                     .translate((185.0, 82.5, 169.0))).material(small))
    if light == "quad":
        rect = polygon([(343.0, 548.8, 227.0), (343.0, 548.8, 332.0), (213.0, 548.8, 332.0), (213.0, 548.8, 227.0)])
        scene.add(Light.Object(Object(rect).material(Material.light(hex_color(0xFFFEFA), 100.0))))
    else:
        scene.add(Light.Point((40000.0, 40000.0, 38000.0), (278.0, 540.0, 279.5)))
    if extra_light is not None:
        scene.add(extra_light)
    camera = Camera(eye=(278.0, 273.0, -800.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=0.686)
    return scene, camera


def params(w, h, b, spp, flags=PERSISTENT, **kw):
    return make_params(w, h, b, spp, seed=kw.pop("seed", 13), flags=flags, **kw)


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


def launch_line(g, cam, capfd):
    """The persistent kernel's launch diagnostics (RPTGPU_PRINT_LAUNCH) of one small render."""
    capfd.readouterr()
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    try:
        g.render_batch(cam, params(16, 9, 2, 1))
    finally:
        del os.environ["RPTGPU_PRINT_LAUNCH"]
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]


@pytest.fixture(scope="module")
def c2(oracle):
    scene, cam, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    g3 = GpuScene(scene, 0, paths_chunk=3)
    yield cam, g, g3, oracle.OracleScene(scene)
    g.close()
    g3.close()


def test_c2_takes_the_fused_kernel(c2, capfd):
    cam, g, _, _ = c2
    lines = launch_line(g, cam, capfd)
    assert lines and all(FUSED in ln for ln in lines), lines


@pytest.mark.parametrize("bounces", [0, 1, 2, 3, 8])
def test_c2_small_odd_sizes(c2, bounces):
    cam, g, _, osc = c2
    check(g, osc, cam, params(97, 55, bounces, 5))
    check(g, osc, cam, params(33, 17, bounces, 9, seed=3))


def test_spp_not_a_multiple_of_the_chunk(c2):
    cam, _, g3, osc = c2
    check(g3, osc, cam, params(161, 91, 8, 7))
    check(g3, osc, cam, params(95, 53, 5, 11, seed=5))


def test_later_sample_batch_and_tiles(c2):
    cam, g, _, osc = c2
    check(g, osc, cam, params(96, 54, 8, 6, sample_index_base=6))
    acc = None
    for i in range(4):
        img = check(g, osc, cam, params(128, 72, 8, 4, tile=(32, 8), part=(i, 4)))
        acc = img if acc is None else acc + img
    assert (acc == check(g, osc, cam, params(128, 72, 8, 4))).all()


@pytest.mark.parametrize("kind", ["point", "glass"])
def test_fused_variants(oracle, capfd, kind):
    scene, cam = cornell_variant(light="point" if kind == "point" else "quad", glass=kind == "glass")
    g = GpuScene(scene, 0)
    try:
        lines = launch_line(g, cam, capfd)
        assert lines and all(FUSED in ln for ln in lines), lines
        osc = oracle.OracleScene(scene)
        for b in (0, 1, 8):
            check(g, osc, cam, params(77, 43, b, 6))
    finally:
        g.close()


@pytest.mark.parametrize("extra", ["point", "ambient"])
def test_two_lights_keep_the_one_ray_kernel(oracle, capfd, extra):
    light = (Light.Point((20000.0, 20000.0, 20000.0), (100.0, 500.0, 100.0)) if extra == "point"
             else Light.Ambient((0.05, 0.05, 0.05)))
    scene, cam = cornell_variant(extra_light=light)
    g = GpuScene(scene, 0)
    try:
        lines = launch_line(g, cam, capfd)
        assert lines and not any(FUSED in ln for ln in lines), lines
        osc = oracle.OracleScene(scene)
        for b in (0, 8):
            check(g, osc, cam, params(77, 43, b, 6))
    finally:
        g.close()
