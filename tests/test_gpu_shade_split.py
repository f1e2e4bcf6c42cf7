"""rpt_paths<KdFlat, false, true>'s fast shading form (kernels/paths_shade.inc hit_draws, RPT_SHADE_SPLIT) on a real MI355X:
a wave whose light is an untransformed mesh and whose hits are opaque takes every draw of its hits first (the light
triangle's index and (u, v) pairs, gen_bool, u_theta and the +-1 pairs) and shades them in one straight-line block.
Every frame is compared BIT for bit with the oracle, with the closest-hit and shadow ray counts equal to the oracle's:
C2 at bounces 0-8 and odd sizes (paths that stop at max_bounces draw no sample_f values), later sample batches, a point
light (the sequence of illuminate / sample_f), and a glass cube, whose waves mix the two forms from one iteration to the
next: a wave with a lane on the glass takes the sequence, the others the straight-line block."""
import math

import numpy as np
import pytest

from rpt_amd import Camera, GpuScene, Light, Material, Object, Scene, _abi, cube, hex_color, make_params, polygon, scenes

pytestmark = pytest.mark.gpu

PERSISTENT = _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_PROFILE_KERNELS


def cornell(light="quad", glass=False, metal=False):
    """examples/cornell.rs with the light swapped for a point light, the small box made of glass, or the tall box of a
    rough metal (a specular-lobe probability near 1 against the walls' 0.232)."""
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
    tall = Material.metallic_(hex_color(0xD4AF37), 0.2) if metal else white
    scene.add(Object(cube().scale((165.0, 330.0, 165.0)).rotate_y(two_pi * (-253.0 / 360.0))
                     .translate((368.0, 165.0, 351.0))).material(tall))
    small = Material.clear(1.5, 0.0) if glass else white
    scene.add(Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(two_pi * (-197.0 / 360.0))
                     .translate((185.0, 82.5, 169.0))).material(small))
    if light == "quad":
        rect = polygon([(343.0, 548.8, 227.0), (343.0, 548.8, 332.0), (213.0, 548.8, 332.0), (213.0, 548.8, 227.0)])
        scene.add(Light.Object(Object(rect).material(Material.light(hex_color(0xFFFEFA), 100.0))))
    else:
        scene.add(Light.Point((40000.0, 40000.0, 38000.0), (278.0, 540.0, 279.5)))
    camera = Camera(eye=(278.0, 273.0, -800.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=0.686)
    return scene, camera


def params(w, h, b, spp, **kw):
    return make_params(w, h, b, spp, seed=kw.pop("seed", 29), flags=PERSISTENT, **kw)


def check(g, osc, cam, p):
    g.reset_stats()
    img = g.render_batch(cam, p)
    st = g.stats()
    ref, cnt = osc.render(cam, p, threads=0, counters=True)
    assert st.kernel_launches[_abi.RPT_K_PATHS] >= 1
    assert (img.view(np.int64) == ref.view(np.int64)).all(), (p.width, p.height, p.max_bounces, np.abs(img - ref).max())
    assert st.extend_rays == cnt["closest_rays"], (st.extend_rays, cnt["closest_rays"])
    assert st.shadow_rays == cnt["shadow_rays"], (st.shadow_rays, cnt["shadow_rays"])
    return img


@pytest.fixture(scope="module")
def c2(oracle):
    scene, cam, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    yield cam, g, oracle.OracleScene(scene)
    g.close()


@pytest.mark.parametrize("bounces", list(range(9)))
def test_c2_bounces(c2, bounces):
    cam, g, osc = c2
    check(g, osc, cam, params(63, 37, bounces, 4))


def test_c2_odd_sizes_and_seeds(c2):
    cam, g, osc = c2
    check(g, osc, cam, params(101, 57, 8, 7, seed=7))
    check(g, osc, cam, params(17, 131, 5, 13, seed=11))


def test_c2_later_sample_batches(c2):
    cam, g, osc = c2
    for base in (5, 64, 1001):
        check(g, osc, cam, params(80, 45, 8, 5, sample_index_base=base))


@pytest.mark.parametrize("kind", ["point", "glass", "metal"])
def test_variants(oracle, kind):
    scene, cam = cornell(light="point" if kind == "point" else "quad", glass=kind == "glass", metal=kind == "metal")
    g = GpuScene(scene, 0)
    try:
        osc = oracle.OracleScene(scene)
        for b in (0, 1, 8):
            check(g, osc, cam, params(71, 41, b, 6))
        check(g, osc, cam, params(64, 36, 8, 5, sample_index_base=37))
    finally:
        g.close()
