"""The shadow ray's window in the two-ray query (kernels/paths_flat.inc run_beyond, RPT_SHADOW_WINDOW; the proof stands at
scene_plan.h axis_flat_mesh) on a real MI355X.  The rule leaves out, for the shadow ray only, the leaf test of an axis-flat
wall whose plane lies beyond the light; it may change no bit.  Tolerance 0 throughout, 8 bounces, 4 spp:

(1) frames equal to the oracle's with its ray counts, each through the fused kernel: cornell at 96x64 and 33x17; the Cornell
    room (less its right wall: the wave's LDS share holds no more) with one more axis-flat quad under half of the light — well in front of it, 1e-9 in front of the light's plane, coplanar with
    the light and overlapping it, 1e-9 behind it, 0.05 behind it — and with that quad tilted into a ramp, a table user
    without the mark; the room lit by a point light, and the room without its ceiling lit by a sun (the sequence form of the
    shading, the same query; t_stop = DBL_MAX under the sun: nothing is dropped);
(2) caller rays whose first hits lie at exactly the height of a point light, so that the shadow rays run exactly parallel to
    floor and ceiling (d_y == 0: infinite quotients in the table; as a FRAME this cannot be had against the oracle — a light
    exactly parallel to a wall makes the reference's own bsdf 0 / 0 there), and one views call and one trace_rays call on
    cornell 37x21: the persistent forms, which take the query through the same text, equal to the unflagged calls';
(3) live updates on the handle: rptgpu_scene_set_mesh stays refused on a scene the flat kernel walks (a wall bent out of
    its plane needs a new handle, whose wall then has no mark: the ramp above), and leaves the handle's frame what it
    was; rptgpu_scene_set_objects, which rewrites every object's record, keeps the marks: the frame after it is a fresh handle's;
(4) a library built with -DRPT_SHADOW_WINDOW=0 (scripts/build_variant.sh shadowwin0 "-DRPT_SHADOW_WINDOW=0"), when there is
    one, gives the same frames, counts and ray results."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rpt_amd import Camera, GpuScene, Light, Material, Object, Scene, _abi, cube, hex_color, make_params, polygon, scenes  # noqa: E402

gpu = pytest.mark.gpu

AB_LIB = os.path.join(ROOT, "rpt_amd", "lib", "librptgpu_shadowwin0.so")  # scripts/build_variant.sh shadowwin0 "-DRPT_SHADOW_WINDOW=0"
PERSISTENT = _abi.RPT_FLAG_PERSISTENT
FUSED = "shadow and bounce rays in one query"
BOUNCES, SPP = 8, 4
LIGHT_Y = 548.8

WALLS = [  # examples/cornell.rs: floor, ceiling, back wall, left wall, right wall
    ([(0.0, 0.0, 0.0), (0.0, 0.0, 559.2), (556.0, 0.0, 559.2), (556.0, 0.0, 0.0)], 0xAAAAAA),
    ([(0.0, 548.9, 0.0), (556.0, 548.9, 0.0), (556.0, 548.9, 559.2), (0.0, 548.9, 559.2)], 0xAAAAAA),
    ([(0.0, 0.0, 559.2), (0.0, 548.9, 559.2), (556.0, 548.9, 559.2), (556.0, 0.0, 559.2)], 0xAAAAAA),
    ([(556.0, 0.0, 0.0), (556.0, 0.0, 559.2), (556.0, 548.9, 559.2), (556.0, 548.9, 0.0)], 0xBC0000),
    ([(0.0, 0.0, 0.0), (0.0, 548.9, 0.0), (0.0, 548.9, 559.2), (0.0, 0.0, 559.2)], 0x00BC00),
]
CEILING, RIGHT = 1, 4


def boxes(large=(368.0, 165.0, 351.0)):
    two_pi = 2.0 * math.pi
    return [cube().scale((165.0, 330.0, 165.0)).rotate_y(two_pi * (-253.0 / 360.0)).translate(large),
            cube().scale((165.0, 165.0, 165.0)).rotate_y(two_pi * (-197.0 / 360.0)).translate((185.0, 82.5, 169.0))]


def room(extra=None, light="quad", skip=(), large=(368.0, 165.0, 351.0)):
    """the Cornell room without the walls in `skip`; extra: the corners of one more quad, right behind the walls (one table run)"""
    scene = Scene()
    camera = Camera(eye=(278.0, 273.0, -800.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=0.686)
    for i, (pts, color) in enumerate(WALLS):
        if i not in skip:
            scene.add(Object(polygon(pts)).material(Material.diffuse(hex_color(color))))
    if extra is not None:
        scene.add(Object(polygon(extra)).material(Material.diffuse(hex_color(0x8080C0))))
    for b in boxes(large):
        scene.add(Object(b).material(Material.diffuse(hex_color(0xAAAAAA))))
    if light == "quad":
        rect = polygon([(343.0, LIGHT_Y, 227.0), (343.0, LIGHT_Y, 332.0), (213.0, LIGHT_Y, 332.0), (213.0, LIGHT_Y, 227.0)])
        scene.add(Light.Object(Object(rect).material(Material.light(hex_color(0xFFFEFA), 100.0))))
    elif light == "point":
        scene.add(Light.Point((6e4, 6e4, 5e4), (120.0, 100.0, 400.0)))
    else:  # (oblique: under a sun exactly parallel to a wall the REFERENCE's bsdf is 0 / 0 on that wall, and the frame NaN)
        scene.add(Light.Directional((3.0, 3.0, 2.5), (0.3, -1.0, -0.2)))
    return scene, camera


def shelf(y, ramp=False):
    """An axis-flat quad at height y under the light, about half of which it covers: its slanted edge runs through the light.
    The wave's LDS share sets the shape — next to the fused query's two quotient tables it holds one plane coordinate more
    than the walls', the shelf's y, and that only in a room of four walls (scene_plan.h plan_flat) — so the shelf's corners lie
    on the walls' x and z, and its room stands without the right wall.  ramp: from the floor at x = 0 to the ceiling at
    x = 556 instead — tilted, a table user without the mark"""
    ya, yb, yc = (0.0, 548.9, 548.9 * 20.0 / 556.0) if ramp else (y, y, y)
    return [(0.0, ya, 0.0), (0.0, ya, 559.2), (556.0, yb, 559.2), (20.0, yc, 0.0)]


def shelf_room(y, ramp=False, **kw):
    return room(shelf(y, ramp), skip=(RIGHT,), **kw)


# ---- frames: name -> (scene builder, width, height, seed)
FRAMES = {
    "cornell_96x64": (lambda: scenes.cornell()[:2], 96, 64, 411),
    "cornell_33x17": (lambda: scenes.cornell()[:2], 33, 17, 412),  # a partial last wave
    "shelf_well_in_front": (lambda: shelf_room(400.0), 48, 32, 413),
    "shelf_1e-9_in_front": (lambda: shelf_room(LIGHT_Y - 1e-9), 48, 32, 414),
    "shelf_coplanar": (lambda: shelf_room(LIGHT_Y), 48, 32, 415),
    "shelf_1e-9_behind": (lambda: shelf_room(LIGHT_Y + 1e-9), 48, 32, 416),
    "shelf_0.05_behind": (lambda: shelf_room(LIGHT_Y + 0.05), 48, 32, 417),
    "shelf_ramp": (lambda: shelf_room(0.0, ramp=True), 48, 32, 418),
    "point_light": (lambda: room(light="point"), 48, 32, 419),
    "sun": (lambda: room(light="sun", skip=(CEILING,)), 48, 32, 420),
}
_refs = {}
_here = {}


def frame_inputs(name):
    build, w, h, seed = FRAMES[name]
    scene, cam = build()
    return scene, cam, make_params(w, h, BOUNCES, SPP, seed=seed, flags=PERSISTENT)


def reference(oracle, name):
    """the oracle's frame and counters of a frame, rendered once"""
    if name not in _refs:
        scene, cam, p = frame_inputs(name)
        _refs[name] = oracle.OracleScene(scene).render(cam, p, threads=0, counters=True)
    return _refs[name]


def parallel_rays():
    """rays along +z at the height of the point light of room(light="point"): every first hit has y == 100.0 exactly, so
    the first shadow ray's direction has d_y == 0"""
    n = 601
    o = np.stack([np.linspace(3.0, 553.0, n), np.full(n, 100.0), np.full(n, 10.0)], axis=1)
    d = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def cornell_rays():
    """a 37x21 fan of unit directions from inside the room"""
    w, h = 37, 21
    o, d = np.empty((w * h, 3)), np.empty((w * h, 3))
    for j in range(h):
        for i in range(w):
            v = np.array([(i + 0.5) / w - 0.5, (j + 0.5) / h - 0.5, 0.7])
            o[j * w + i] = (278.0, 273.0, 20.0)
            d[j * w + i] = v / np.sqrt((v * v).sum())
    return o, d


def render_all(flagged_only=False):
    """everything this file compares, with this process's library"""
    out = {}
    for name in FRAMES:
        scene, cam, p = frame_inputs(name)
        g = GpuScene(scene, 0)
        try:
            g.reset_stats()
            out[name] = g.render_batch(cam, p)
            st = g.stats()
            out[name + "_rays"] = np.array([st.extend_rays, st.shadow_rays], dtype=np.uint64)
        finally:
            g.close()
    for name, (scene, cam), (o, d) in (("parallel", room(light="point"), parallel_rays()), ("cornell", scenes.cornell()[:2], cornell_rays())):
        g = GpuScene(scene, 0)
        try:
            for tag, flag in (("_rays_persistent", _abi.RPT_FLAG_RAYS_PERSISTENT), ("_rays_plain", 0)):
                if flag or not flagged_only:
                    out[name + tag] = g.trace_rays(o, d, BOUNCES, samples=SPP, seed=431, flags=flag)
            if name == "cornell":
                for tag, flag in (("_views_persistent", _abi.RPT_FLAG_VIEWS_PERSISTENT), ("_views_plain", 0)):
                    if flag or not flagged_only:
                        out[name + tag] = g.render_views([cam], 37, 21, BOUNCES, samples=SPP, seed=432, flags=flag)
        finally:
            g.close()
    return out


def here():
    if not _here:
        _here.update(render_all())
    return _here


def test_the_shelves_straddle_the_light():
    ys = [shelf(LIGHT_Y + dy)[0][1] for dy in (-1e-9, 0.0, 1e-9)]
    assert ys[0] < ys[1] < ys[2] < 548.9 and ys[1] == LIGHT_Y  # (1e-9 is thousands of ulps of 548.8: three distinct planes)


@gpu
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frames_equal_the_oracles(oracle, capfd, name):
    ref, cnt = reference(oracle, name)
    img, rays = here()[name], here()[name + "_rays"]
    print(name, "max |delta|", np.abs(img - ref).max(), "rays", rays, cnt["closest_rays"], cnt["shadow_rays"])
    assert np.isfinite(ref).all() and ref.max() > 0.0
    assert (img.view(np.int64) == ref.view(np.int64)).all(), (name, np.abs(img - ref).max())
    assert (int(rays[0]), int(rays[1])) == (cnt["closest_rays"], cnt["shadow_rays"]), (name, rays, cnt)
    # the frame ran through the fused kernel, whose query holds the rule
    scene, cam, p = frame_inputs(name)
    g = GpuScene(scene, 0)
    try:
        capfd.readouterr()
        os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
        try:
            g.render_batch(cam, make_params(16, 9, 2, 1, seed=1, flags=PERSISTENT))
        finally:
            del os.environ["RPTGPU_PRINT_LAUNCH"]
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]
        assert lines and all(FUSED in ln for ln in lines), lines
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("name", ["parallel_rays", "cornell_rays", "cornell_views"])
def test_persistent_forms_equal_the_unflagged_calls(name):
    assert _abi.rays_persistent_supported() and _abi.views_persistent_supported()
    a, b = here()[name + "_persistent"], here()[name + "_plain"]
    assert np.isfinite(b).all() and b.max() > 0.0
    assert (np.asarray(a).view(np.int64) == np.asarray(b).view(np.int64)).all(), (name, np.abs(a - b).max())


@gpu
def test_live_updates_keep_the_marks(oracle):
    scene, cam, p = frame_inputs("shelf_well_in_front")
    first = here()["shelf_well_in_front"]
    g = GpuScene(scene, 0)
    try:
        # a wall bent out of its plane: refused as before on a scene the flat kernel walks, and nothing changed
        rows = np.zeros((2, 18))
        bent = [(0.0, 0.0, 0.0), (0.0, 30.0, 559.2), (556.0, 30.0, 559.2), (556.0, 0.0, 0.0)]
        for k, tri in enumerate(((0, 1, 2), (0, 2, 3))):
            rows[k, :9] = np.array([bent[v] for v in tri]).ravel()
            rows[k, 9:] = np.tile([0.0, 1.0, 0.0], 3)
        with pytest.raises(Exception, match="flat path kernel"):
            g.set_mesh(0, rows)
        assert (g.render_batch(cam, p).view(np.int64) == first.view(np.int64)).all()
        # every object's record rewritten, the tall box moved: the marks stay where they were
        moved = (300.0, 165.0, 380.0)
        scene2, _ = shelf_room(400.0, large=moved)
        n = len(scene2.objects)
        g.set_objects(range(n), scene2.objects)
        got = g.render_batch(cam, p)
        fresh = GpuScene(scene2, 0)
        try:
            want = fresh.render_batch(cam, p)
        finally:
            fresh.close()
        ref = oracle.OracleScene(scene2).render(cam, p, threads=0)
        assert (got.view(np.int64) == want.view(np.int64)).all() and (want.view(np.int64) == ref.view(np.int64)).all()
        assert not (got.view(np.int64) == first.view(np.int64)).all()  # (the update is seen)
        # ... and back
        g.set_objects(range(n), scene.objects)
        assert (g.render_batch(cam, p).view(np.int64) == first.view(np.int64)).all()
    finally:
        g.close()


@gpu
@pytest.mark.skipif(not os.path.exists(AB_LIB), reason="no library built with -DRPT_SHADOW_WINDOW=0 (scripts/build_variant.sh shadowwin0)")
def test_library_without_the_window_gives_the_same(tmp_path):
    path = str(tmp_path / "old.npz")
    env = dict(os.environ, RPTGPU_LIB=AB_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    old, new = np.load(path), here()
    assert len(old.files) >= 2 * len(FRAMES) + 3
    for name in old.files:
        a, b = np.asarray(old[name]), np.asarray(new[name])
        assert a.dtype == b.dtype and (a.view(np.uint64) == b.view(np.uint64)).all(), name


if __name__ == "__main__":
    np.savez(sys.argv[1], **render_all(flagged_only=True))
