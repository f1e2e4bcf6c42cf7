"""rpt_paths<KdFlat, false, true, true> (kernels/paths_consts.inc SceneConsts, RPT_SCENE_CONSTS) on a real MI355X: what a hit
derives from the scene alone — the material's m2, f0, lobe probability and gen_bool's integer, a cube's world normals,
and in builds with that group (-DRPT_SCENE_CONSTS=7) the pdf of the light's triangle — is computed once per wave into
tables and read from there.  The tables are filled by the
loop's own expressions, so every frame must equal the oracle's BIT for bit, with the oracle's ray counts, and every scene
here must run through that kernel (the launch diagnostics say so: a scene that fell back to the kernel without the tables
cannot pass).  The scenes: four walls of four different materials, one of them a white metal whose lobe probability is
exactly 1.0 (gen_bool then takes no draw); a mesh light of three triangles of unequal area; two consecutive cubes rotated
about two axes and scaled unevenly, seen from outside, and with one of them around the camera and the light (exit normals,
five faces in view), at 0 bounces (the pre-trace pass) and 8 (the bounce slot); a wall's material and a cube's placement
changed on a live handle; and the same frames from a library built with -DRPT_SCENE_CONSTS=0, when there is one."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rpt_amd import Camera, GpuScene, Light, Material, Object, Scene, _abi, cube, hex_color, make_params, polygon  # noqa: E402

gpu = pytest.mark.gpu

PERSISTENT = _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_PROFILE_KERNELS
FUSED = "shadow and bounce rays in one query"
TABLES = "a hit's scene constants from the wave's tables"
AB_LIB = os.path.join(ROOT, "rpt_amd", "lib", "librptgpu_sc0.so")  # scripts/build_variant.sh sc0 "-DRPT_SCENE_CONSTS=0"

WHITE_METAL = Material.metallic_((1.0, 1.0, 1.0), 0.3)
WALL_MATERIALS = (
    WHITE_METAL,                                                              # floor: fs == 1.0
    Material((0.70, 0.62, 0.51), index=1.3, roughness=0.4, metallic=0.0),     # back
    Material(hex_color(0xBC0000), index=2.2, roughness=0.7, metallic=0.5),    # right
    Material.specular(hex_color(0x00BC00), 0.15),                             # left
)


def lobe_probability(m):
    """sample_f's f (material.rs), in the oracle's operation order"""
    f0 = ((m.index - 1.0) / (m.index + 1.0)) ** 2
    mean = ((m.color[0] + m.color[1]) + m.color[2]) / 3.0
    f = (1.0 - m.metallic) * f0 + m.metallic * mean
    return f * (1.0 - 0.2) + 1.0 * 0.2


def room(around_camera=False, floor=WHITE_METAL, tall_angle=-253.0):
    """Cornell's room without its ceiling wall (so that a third light triangle fits the wave's tables), the walls of
    WALL_MATERIALS, the two boxes turned about two axes and scaled unevenly, a pentagon for a light.  around_camera: the
    second box encloses the camera, the light and the first box."""
    scene = Scene()
    walls = [
        [(0.0, 0.0, 0.0), (0.0, 0.0, 559.2), (556.0, 0.0, 559.2), (556.0, 0.0, 0.0)],
        [(0.0, 0.0, 559.2), (0.0, 548.9, 559.2), (556.0, 548.9, 559.2), (556.0, 0.0, 559.2)],
        [(556.0, 0.0, 0.0), (556.0, 0.0, 559.2), (556.0, 548.9, 559.2), (556.0, 548.9, 0.0)],
        [(0.0, 0.0, 0.0), (0.0, 548.9, 0.0), (0.0, 548.9, 559.2), (0.0, 0.0, 559.2)],
    ]
    for pts, m in zip(walls, (floor,) + WALL_MATERIALS[1:]):
        scene.add(Object(polygon(pts)).material(m))
    two_pi = 2.0 * math.pi
    scene.add(Object(cube().scale((165.0, 330.0, 120.0)).rotate_y(two_pi * (tall_angle / 360.0)).rotate_x(0.21)
                     .translate((368.0, 190.0, 351.0))).material(Material.metallic_(hex_color(0xD4AF37), 0.25)))
    if around_camera:
        scene.add(Object(cube().scale((520.0, 580.0, 500.0)).rotate_y(0.1).rotate_z(0.05)
                         .translate((278.0, 280.0, 300.0))).material(Material((0.8, 0.8, 0.9), 1.8, 0.6, 0.0)))
    else:
        scene.add(Object(cube().scale((150.0, 165.0, 190.0)).rotate_y(two_pi * (-197.0 / 360.0)).rotate_z(-0.33)
                         .translate((185.0, 110.0, 169.0))).material(Material((0.8, 0.8, 0.9), 1.8, 0.6, 0.0)))
    # a triangle fan of three triangles: areas 1 575, 1 312.5 and 6 825
    pent = polygon([(343.0, 548.8, 227.0), (343.0, 548.8, 257.0), (238.0, 548.8, 332.0), (213.0, 548.8, 332.0),
                    (213.0, 548.8, 227.0)])
    scene.add(Light.Object(Object(pent).material(Material.light(hex_color(0xFFFEFA), 100.0))))
    camera = Camera(eye=(278.0, 273.0, 100.0), direction=(0.0, -0.2, 1.0), up=(0.0, 1.0, 0.0), fov=1.4)
    return scene, camera


def params(bounces, spp=8, seed=41):
    return make_params(96, 72, bounces, spp, seed=seed, flags=PERSISTENT)


# every frame the tests compare: name -> (scene arguments, bounces)
CASES = {
    "outside_b8": ({}, 8),
    "outside_b0": ({}, 0),
    "inside_b8": ({"around_camera": True}, 8),
    "inside_b0": ({"around_camera": True}, 0),
    "updated_b8": ({"floor": WALL_MATERIALS[3], "tall_angle": -200.0}, 8),
}
_refs = {}


def reference(oracle, name):
    """the oracle's frame and ray counts of a case, rendered once"""
    if name not in _refs:
        kw, b = CASES[name]
        scene, cam = room(**kw)
        _refs[name] = oracle.OracleScene(scene).render(cam, params(b), threads=0, counters=True)
    return _refs[name]


def launch_lines(g, cam, capfd):
    capfd.readouterr()
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    try:
        g.render_batch(cam, make_params(16, 9, 2, 1, seed=1, flags=PERSISTENT))
    finally:
        del os.environ["RPTGPU_PRINT_LAUNCH"]
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]


def assert_tables(g, cam, capfd):
    lines = launch_lines(g, cam, capfd)
    assert lines and all(FUSED in ln and TABLES in ln for ln in lines), lines


def check(g, cam, oracle, name):
    ref, cnt = reference(oracle, name)
    g.reset_stats()
    img = g.render_batch(cam, params(CASES[name][1]))
    st = g.stats()
    assert st.kernel_launches[_abi.RPT_K_PATHS] >= 1
    assert (img.view(np.int64) == ref.view(np.int64)).all(), (name, np.abs(img - ref).max())
    assert st.extend_rays == cnt["closest_rays"], (st.extend_rays, cnt["closest_rays"])
    assert st.shadow_rays == cnt["shadow_rays"], (st.shadow_rays, cnt["shadow_rays"])
    return img


def test_white_metal_has_lobe_probability_one():
    """the precondition of the gen_bool case: with the oracle's formula f is exactly 1.0, and no other material's is"""
    assert lobe_probability(WHITE_METAL) == 1.0
    assert all(lobe_probability(m) < 1.0 for m in WALL_MATERIALS[1:])
    assert len({(m.roughness, m.index, m.metallic, m.color) for m in WALL_MATERIALS}) == 4


@gpu
@pytest.mark.parametrize("name", ["outside_b8", "outside_b0"])
def test_materials_light_triangles_and_cubes(oracle, capfd, name):
    scene, cam = room(**CASES[name][0])
    g = GpuScene(scene, 0)
    try:
        assert_tables(g, cam, capfd)
        img = check(g, cam, oracle, name)
        assert np.isfinite(img).all() and img.max() > 0.0
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("name", ["inside_b8", "inside_b0"])
def test_cube_around_the_camera_and_the_light(oracle, capfd, name):
    scene, cam = room(**CASES[name][0])
    g = GpuScene(scene, 0)
    try:
        assert_tables(g, cam, capfd)
        img = check(g, cam, oracle, name)
        assert np.isfinite(img).all() and img.max() > 0.0
    finally:
        g.close()


@gpu
def test_live_update_of_a_material_and_a_cube(oracle, capfd):
    """the tables are filled per launch from the records as they stand: an updated handle gives a new handle's frame"""
    scene, cam = room()
    g = GpuScene(scene, 0)
    try:
        first = check(g, cam, oracle, "outside_b8")
        new, _ = room(**CASES["updated_b8"][0])
        g.update(new)
        assert_tables(g, cam, capfd)
        img = check(g, cam, oracle, "updated_b8")
        assert not (img == first).all()
        h = GpuScene(new, 0)
        try:
            assert (h.render_batch(cam, params(8)).view(np.int64) == img.view(np.int64)).all()
        finally:
            h.close()
        g.update(scene)
        assert (check(g, cam, oracle, "outside_b8") == first).all()
    finally:
        g.close()


def render_cases(path):
    """(a process of its own, under RPTGPU_LIB) every case's frame and ray counts into an .npz, the launch lines beside them"""
    out = {}
    for name, (kw, b) in CASES.items():
        scene, cam = room(**kw)
        g = GpuScene(scene, 0)
        g.reset_stats()
        out[name] = g.render_batch(cam, params(b))
        st = g.stats()
        out[name + "_rays"] = np.array([st.extend_rays, st.shadow_rays], dtype=np.uint64)
        os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
        g.render_batch(cam, make_params(16, 9, 2, 1, seed=1, flags=PERSISTENT))
        del os.environ["RPTGPU_PRINT_LAUNCH"]
        g.close()
    np.savez(path, **out)


@gpu
@pytest.mark.skipif(not os.path.exists(AB_LIB), reason="no library built with -DRPT_SCENE_CONSTS=0 (scripts/build_variant.sh sc0)")
def test_library_without_the_tables_gives_the_same_frames(oracle, tmp_path):
    out = str(tmp_path / "frames.npz")
    env = dict(os.environ, RPTGPU_LIB=AB_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("rpt_paths<")]
    assert len(lines) >= len(CASES) and all(FUSED in ln and TABLES not in ln for ln in lines), lines
    got = np.load(out)
    for name in CASES:
        ref, cnt = reference(oracle, name)
        assert (got[name].view(np.int64) == ref.view(np.int64)).all(), name
        assert tuple(int(v) for v in got[name + "_rays"]) == (cnt["closest_rays"], cnt["shadow_rays"]), name


if __name__ == "__main__":
    render_cases(sys.argv[1])
