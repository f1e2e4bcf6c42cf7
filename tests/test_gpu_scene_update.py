"""Live updates of a scene handle (rptgpu_scene_set_objects / _lights, GpuScene.update) on a real MI355X.  The contract:
after an update every frame, closest-hit query and buffer result is BIT-EQUAL to what a handle freshly created from the
updated scene gives, and a refused update leaves the handle rendering what it rendered before."""
import math

import numpy as np
import pytest

from rpt_amd import (Buffer, Camera, DeviceBuffer, GpuScene, Light, Material, Object, Renderer, Scene, _abi, cube,
                     hex_color, make_params, plane, scenes, sphere)
from rpt_amd.ode import MarblesSystem

pytestmark = pytest.mark.gpu

W, H = 128, 96
FLAGS = {"persistent": _abi.RPT_FLAG_PERSISTENT, "wavefront": _abi.RPT_FLAG_WAVEFRONT}


def params(spp=8, bounces=3, flags=0, seed=0x5550, base=0, size=(W, H)):
    return make_params(size[0], size[1], bounces, spp, seed=seed, sample_index_base=base, flags=flags)


def fresh(scene, cam, p):
    g = GpuScene(scene, 0)
    try:
        return g.render_batch(cam, p)
    finally:
        g.close()


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def video(frame=0, cube_at=None):
    """scenes.simple_video's frame, optionally with its cube placed at `cube_at` instead"""
    scene, cam, _ = scenes.simple_video(frame)
    if cube_at is not None:
        scene.objects[1] = Object(cube().rotate_y(math.pi / 6.0).scale((0.5, 0.3, 0.4)).translate(cube_at)) \
            .material(Material.specular(hex_color(0xFF00FF), 0.5))
    return scene, cam


@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_simple_video_frames_through_one_handle(mode):
    p = params(flags=FLAGS[mode])
    scene0, cam = video(0)
    g = GpuScene(scene0, 0)
    first = g.render_batch(cam, p)
    # frames 1, 37, 59, then the cube several units outside the grid of the filter boxes made at creation (x, y and z
    # beyond every bounded object of frame 0): with the creation's boxes its pixels would be filtered away
    for scene, _ in (video(1), video(37), video(59), video(cube_at=(2.8, 1.8, -4.0)), video(0)):
        g.update(scene)
        img = g.render_batch(cam, p)
        assert np.isfinite(img).all()
        assert same(img, fresh(scene, cam, p))
    assert same(img, first)  # back at frame 0
    moved, _ = video(cube_at=(2.8, 1.8, -4.0))
    assert not same(fresh(moved, cam, p), first)  # (the moved cube is in view)
    g.close()


def test_object_exempted_from_the_filter_and_back():
    """an object whose placement becomes ill-conditioned, or not finite, joins obj_always; updated back, it leaves it"""
    p = params()
    scene0, cam = video(0)
    g = GpuScene(scene0, 0)
    first = g.render_batch(cam, p)
    for xf in (lambda s: s.scale((0.5, 1e-5, 0.5)).translate((1.5, -0.5, 1.0)),      # condition number 1e5
               lambda s: s.scale((0.5, 0.5, 0.5)).translate((1.5, math.inf, 1.0)),   # a box that is not finite
               lambda s: s.scale((0.5, 0.5, 0.5)).translate((math.nan, -0.5, 1.0))):
        scene, _ = video(0)
        scene.objects[2] = Object(xf(sphere())).material(Material.specular(hex_color(0x0000FF), 0.1))
        g.update(scene)
        assert same(g.render_batch(cam, p), fresh(scene, cam, p))
        g.update(scene0)
        assert same(g.render_batch(cam, p), first)
    g.close()


def test_metal_instances_moved_and_rematerialled():
    """two Transformed instances of one mesh (a kd-tree walked in-kernel), under the wavefront pipeline; the tree is
    untouched; rptgpu_closest_hit agrees too"""
    scene, cam, _ = scenes.metal(hdri_size=(64, 32))
    p = params(spp=4, bounces=3, flags=_abi.RPT_FLAG_WAVEFRONT)
    g = GpuScene(scene, 0)
    before = g.render_batch(cam, p)
    mesh = scene.objects[0].shape.shape
    new = Scene()
    new.environment = scene.environment
    new.add(Object(mesh.scale((0.4, 0.6, 0.4)).rotate_y(0.8).translate((0.6, -1.5, 0.3)))
            .material(Material.diffuse(hex_color(0x33AA66))))
    new.add(Object(mesh.scale((0.5, 0.5, 0.5)).rotate_x(0.3).translate((-0.4, 0.4, -0.5)))
            .material(Material.clear(1.5, 0.0001)))
    g.update(new)
    img = g.render_batch(cam, p)
    assert same(img, fresh(new, cam, p))
    assert not same(img, before)
    rng = np.random.default_rng(11)
    o = np.tile([0.0, 0.0, 10.0], (20000, 1)) + rng.uniform(-0.2, 0.2, (20000, 3))
    d = np.stack([rng.uniform(-0.3, 0.3, 20000), rng.uniform(-0.35, 0.3, 20000), -np.ones(20000)], axis=1)
    got = g.closest_hit(o, d)
    f = GpuScene(new, 0)
    want = f.closest_hit(o, d)
    f.close()
    assert (got[2] >= 0).sum() > 500
    for a, b in zip(got, want):
        assert same(a, b)
    g.close()


def lit_scene(light_at=(0.0, 3.0, 2.0), light_scale=0.5, light_color=(1.0, 0.9, 0.8), point_at=(-2.0, 4.0, 3.0),
              point_color=(20.0, 20.0, 20.0)):
    scene = Scene()
    scene.add(Object(sphere()).material(Material.diffuse((0.7, 0.7, 0.7))))
    scene.add(Object(cube().scale((0.8, 0.8, 0.8)).translate((1.6, -0.6, 0.5))).material(Material.specular((0.2, 0.4, 0.9), 0.3)))
    scene.add(Object(plane((0.0, 1.0, 0.0), -1.0)).material(Material.diffuse((0.6, 0.6, 0.6))))
    scene.add(Light.Object(Object(sphere().scale((light_scale,) * 3).translate(light_at))
                           .material(Material.light(light_color, 30.0))))
    scene.add(Light.Point(point_color, point_at))
    scene.add(Light.Ambient((0.01, 0.01, 0.01)))
    return scene


def test_lights_moved_and_recoloured():
    cam = Camera()
    p = params(spp=8, bounces=3)
    g = GpuScene(lit_scene(), 0)
    first = g.render_batch(cam, p)
    moved = lit_scene(light_at=(1.0, 2.5, 3.0), light_scale=0.3, light_color=(0.3, 0.5, 1.0), point_at=(2.0, 3.0, 4.0))
    g.update(moved)
    img = g.render_batch(cam, p)
    assert same(img, fresh(moved, cam, p)) and not same(img, first)
    # the same through set_lights alone: the point light's colour and the light object
    only = lit_scene(point_color=(5.0, 1.0, 1.0), light_at=(-1.0, 2.0, 2.0))
    g.update(lit_scene())
    g.set_lights([1, 0], [only.lights[1], only.lights[0]])
    assert same(g.render_batch(cam, p), fresh(only, cam, p))
    g.close()


def test_material_only_updates():
    cam = Camera()
    p = params(spp=8, bounces=4)
    base = lit_scene()
    g = GpuScene(base, 0)
    variants = []
    s = lit_scene()
    s.objects[0] = Object(sphere()).material(Material.clear(1.5, 0.0001))  # diffuse -> clear glass
    variants.append(s)
    s = lit_scene()
    s.objects[1] = Object(s.objects[1].shape).material(Material.light((1.0, 0.5, 0.2), 3.0))  # emittance
    variants.append(s)
    s = lit_scene()
    s.lights[0] = Light.Object(Object(s.lights[0].object.shape).material(Material.light((0.2, 1.0, 0.2), 80.0)))
    variants.append(s)
    for s in variants:
        g.update(s)
        assert same(g.render_batch(cam, p), fresh(s, cam, p))
    g.close()


def test_a_b_a_leaks_nothing():
    cam = Camera()
    p = params(spp=8, bounces=3)
    a, b = lit_scene(), lit_scene(light_at=(2.0, 2.0, 1.0), point_at=(0.0, 1.0, 6.0))
    b.objects[0] = Object(sphere().scale((0.7, 1.2, 0.7)).translate((-0.5, 0.0, 0.0))) \
        .material(Material.metallic_((0.9, 0.8, 0.4), 0.2))
    a.objects[0] = Object(sphere().scale((1.0, 1.0, 1.0))).material(Material.diffuse((0.7, 0.7, 0.7)))
    g = GpuScene(a, 0)
    first = g.render_batch(cam, p)
    g.update(b)
    assert same(g.render_batch(cam, p), fresh(b, cam, p))
    g.update(a)
    assert same(g.render_batch(cam, p), first)
    g.close()


def test_refused_updates_change_nothing():
    scene0, cam = video(0)
    p = params()
    g = GpuScene(scene0, 0)
    before = g.render_batch(cam, p)
    good = Object(sphere().scale((0.5, 0.5, 0.5)).translate((1.0, 0.5, 2.0))).material(Material.diffuse((1.0, 1.0, 1.0)))
    bad_material = Object(sphere().scale((0.5, 0.5, 0.5))).material(Material(metallic=5.0))
    cases = [
        (lambda: g.set_objects([5], [good]), "out of range"),
        (lambda: g.set_objects([2, 2], [good, good]), "named twice"),
        (lambda: g.set_objects([2, 1], [good, Object(sphere().translate((0.0, 0.0, 1.0)))]), "differs from the kind"),
        (lambda: g.set_objects([2, 0], [good, Object(sphere().translate((0.0, 0.0, 1.0)))]), "Transformed"),
        (lambda: g.set_objects([2, 3], [good, bad_material]), "outside [0, 1]"),
        (lambda: g.set_lights([2], [Light.Ambient((1.0, 1.0, 1.0))]), "out of range"),
        (lambda: g.set_lights([0, 1], [Light.Ambient((0.2, 0.2, 0.2)), Light.Directional((1.0, 1.0, 1.0), (0, -1, 0))]),
         "differs from the kind"),
    ]
    for call, why in cases:
        with pytest.raises(_abi.RptGpuError) as e:
            call()
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT
        assert why in str(e.value), str(e.value)
        assert same(g.render_batch(cam, p), before), why
    with pytest.raises(ValueError, match="objects"):
        g.update(Scene())
    g.close()


def test_device_buffer_across_an_update():
    cam = Camera()
    a, b = lit_scene(), lit_scene(light_at=(1.5, 2.0, 2.0), point_at=(3.0, 3.0, 3.0))
    g = GpuScene(a, 0)
    dbuf = DeviceBuffer(g, W, H)
    host = Buffer(W, H)
    for k, s in enumerate((a, b, a)):
        g.update(s)
        p = params(spp=4, base=4 * k)
        dbuf.sample(cam, p)
        host.add_samples(fresh(s, cam, p))
    assert dbuf.num_batches() == 3
    assert (dbuf.image() == host.image()).all()
    assert dbuf.variance() == host.variance()
    dbuf.close()
    g.close()


def test_emulate_ranks_after_an_update():
    scene0, cam = video(0)
    p = params()
    g = GpuScene(scene0, 0)
    g.render_batch_emulate_ranks(cam, p, 2)
    scene, _ = video(30)
    g.update(scene)
    got = g.render_batch_emulate_ranks(cam, p, 2)
    f = GpuScene(scene, 0)
    want = f.render_batch_emulate_ranks(cam, p, 2)
    f.close()
    assert same(got, want)
    g.close()


def test_marbles_frames_through_update(oracle):
    state = scenes.marbles_start()
    system = MarblesSystem(scenes.MARBLES_R)
    p = make_params(200, 150, 7, 1, seed=0x4D41)
    g = None
    for frame in range(5):
        scene, cam, cfg = scenes.marbles(state, test=True)
        assert (cfg["width"], cfg["height"], cfg["max_bounces"], cfg["num_samples"]) == (200, 150, 7, 1)
        if g is None:
            g = GpuScene(scene, 0)
            img = g.render_batch(cam, p)
            ref = oracle.OracleScene(scene).render(cam, p, threads=0)
            assert np.isfinite(img).all() and img.max() > 0
            assert (img == ref).all()
        else:
            g.update(scene)
            img = g.render_batch(cam, p)
        assert same(img, fresh(scene, cam, p)), frame
        # the Renderer over the kept handle: the PNG scripts/marbles.py writes, with and without --rebuild
        assert (Renderer(scene, cam).width(200).height(150).max_bounces(7).num_samples(1).with_gpu_scene(g).render()
                == Renderer(scene, cam).width(200).height(150).max_bounces(7).num_samples(1).render()).all()
        system.rk4_integrate(state, 1.0 / 16.0, 1.0 / 10000.0)
    g.close()
