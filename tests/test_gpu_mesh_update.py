"""A deforming mesh on a live scene handle (rptgpu_scene_set_mesh[_device], GpuScene.set_mesh) on a real MI355X.  The
contract: after the call every result — frames under every pipeline flag, rptgpu_closest_hit,
rptgpu_render_aov, rptgpu_trace_rays, rptgpu_bake_probes, the device Buffer — is BIT-EQUAL to that of a handle freshly
created from the scene in which the mesh has the new triangles, and a refused call leaves the handle rendering what it
rendered before.  Every comparison here is tobytes() equality against such a fresh handle."""
import math

import numpy as np
import pytest

from rpt_amd import (Camera, DeviceBuffer, GpuScene, KdTree, Light, Material, Mesh, Object, RptGpuError, Scene, _abi,
                     make_params, plane, polygon, scenes, sphere)
from rpt_amd.device import kdtree_build

pytestmark = pytest.mark.gpu

W, H = 64, 48
FLAGS = {"default": 0, "wavefront": _abi.RPT_FLAG_WAVEFRONT, "persistent": _abi.RPT_FLAG_PERSISTENT,
         "general": _abi.RPT_FLAG_GENERAL_TRAVERSAL}
KNOT = scenes.knot_mesh(nu=48, nv=16)            # 1 536 triangles: the mesh that deforms
OTHER = scenes.knot_mesh(nu=24, nv=8, seed=3)    # 384 triangles: the mesh that stays
assert KNOT.shape == (1536, 18) and OTHER.shape == (384, 18)
CAM = Camera()


def params(flags=0, spp=4, bounces=3, seed=0x4D45):
    return make_params(W, H, bounces, spp, seed=seed, flags=flags)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def place(mesh, at=(-0.6, 0.2, 0.0), turn=0.4):
    return mesh.scale((2.6, 2.6, 2.6)).rotate_y(turn).translate(at)


def base_scene(tris, at=(-0.6, 0.2, 0.0), turn=0.4):
    """the deforming knot (object 0, Transformed), a second mesh, a sphere, a plane, a point light, a Light::Object sphere"""
    s = Scene()
    s.add(Object(place(Mesh(tris), at, turn)).material(Material.diffuse((0.8, 0.5, 0.3))))
    s.add(Object(Mesh(OTHER).scale((1.4, 1.4, 1.4)).translate((1.5, 0.1, 0.4))).material(Material.specular((0.3, 0.6, 0.9), 0.2)))
    s.add(Object(sphere().scale((0.4, 0.4, 0.4)).translate((0.6, -0.6, 1.5))).material(Material.diffuse((0.7, 0.7, 0.7))))
    s.add(Object(plane((0.0, 1.0, 0.0), -1.0)).material(Material.diffuse((0.6, 0.6, 0.6))))
    s.add(Light.Point((30.0, 30.0, 30.0), (-2.0, 4.0, 4.0)))
    s.add(Light.Object(Object(sphere().scale((0.3, 0.3, 0.3)).translate((1.0, 2.4, 2.0))).material(Material.light((1.0, 0.9, 0.8), 40.0))))
    return s


def handle(scene, **options):
    options.setdefault("deep_depth", 1)
    return GpuScene(scene, 0, **options)


def rays(n=20000, seed=5):
    """from around the eye towards both meshes, the sphere and the floor"""
    rng = np.random.default_rng(seed)
    o = np.tile([0.0, 0.0, 10.0], (n, 1)) + rng.uniform(-0.2, 0.2, (n, 3))
    d = np.stack([rng.uniform(-0.28, 0.28, n), rng.uniform(-0.2, 0.2, n), -np.ones(n)], axis=1)
    return o, d


RAYS = rays()


def verts(tris):
    return tris[:, :9].reshape(-1, 3)


def with_verts(tris, v):
    out = tris.copy()
    out[:, :9] = v.reshape(-1, 9)
    return out


def tree_of(tris):
    """the tree of these triangles' boxes by the library's host builder: what a test says about depth and entries"""
    v = tris[:, :9].reshape(-1, 3, 3)
    return kdtree_build(np.concatenate([v.min(axis=1), v.max(axis=1)], axis=1))


# ---- the deformations of the issue, each a function of the creation's triangles
def sine(t, phase=0.0):
    v = verts(t).copy()
    v[:, 1] += 0.05 * np.sin(9.0 * v[:, 0] + phase) * np.cos(7.0 * v[:, 2])
    return with_verts(t, v)


def far_and_large(t):
    far = np.array([40.0, -25.0, 10.0])
    return with_verts(t, (verts(t) - far) * 1000.0 + far)


def squashed(t):
    v = verts(t).copy()
    v[:, 1] = np.where(np.arange(len(v)) % 3 == 0, -0.0, 0.0)  # y = 0 as a mix of both zeros
    return with_verts(t, v)


def half_collapsed(t):
    out = t.copy()
    out[::2, 3:6] = out[::2, 0:3]
    out[::2, 6:9] = out[::2, 0:3]
    return out


def clustered(t):
    v = verts(t).copy()
    rng = np.random.default_rng(1)
    pull = rng.uniform(size=len(v)) < 0.9
    c = np.array([0.1, -0.2, 0.05])
    v[pull] = c + (v[pull] - c) * 1e-3
    return with_verts(t, v)


def shrunk(t):
    v = t[:, :9].reshape(-1, 3, 3)
    c = v.mean(axis=1, keepdims=True)
    return with_verts(t, (c + (v - c) * 0.15).reshape(-1, 3))


def non_finite(t):
    out = sine(t, 1.0)
    out[100, 4] = math.nan
    out[900, 6] = math.inf
    return out


DEFORMATIONS = [("sine", sine), ("far_and_large", far_and_large), ("squashed", squashed), ("half_collapsed", half_collapsed),
                ("clustered", clustered), ("shrunk", shrunk), ("non_finite", non_finite), ("original", lambda t: t.copy())]


def test_the_deformations_do_what_their_names_say():
    base = tree_of(KNOT)
    deep = tree_of(clustered(KNOT))
    assert deep["max_depth"] > base["max_depth"] and len(deep["refs"]) > len(base["refs"])
    assert len(tree_of(shrunk(KNOT))["refs"]) < len(base["refs"])
    y = verts(squashed(KNOT))[:, 1]
    assert (y == 0.0).all() and np.signbit(y).any() and not np.signbit(y).all()


def check_against_fresh(g, scene, p, options, what):
    """a frame and closest_hit on 20 000 rays: the updated handle against a fresh one of `scene`"""
    f = handle(scene, **options)
    try:
        got, want = g.render_batch(CAM, p), f.render_batch(CAM, p)
        assert same(got, want), "%s: frame differs in %d values" % (what, (got != want).sum())
        hit_g, hit_f = g.closest_hit(*RAYS), f.closest_hit(*RAYS)
        for a, b in zip(hit_g, hit_f):
            assert same(a, b), "%s: closest_hit differs" % what
        assert (hit_g[2] == 1).sum() > 200, "the rays reach the untouched mesh"
        return got, hit_g
    finally:
        f.close()


@pytest.mark.parametrize("device_build_min", [0, 16])
@pytest.mark.parametrize("mode", sorted(FLAGS))
def test_deformations_equal_a_fresh_handle(mode, device_build_min):
    p = params(flags=FLAGS[mode])
    options = {"device_build_min": device_build_min}
    g = handle(base_scene(KNOT), **options)
    first = g.render_batch(CAM, p)
    first_hits = g.closest_hit(*RAYS)
    assert (first_hits[2] == 0).sum() > 200, "the rays reach the knot"
    other = first_hits[2] == 1
    for name, deform in DEFORMATIONS:
        tris = deform(KNOT)
        g.set_mesh(0, tris)
        img, hits = check_against_fresh(g, base_scene(tris), p, options, name)
        if name in ("sine", "half_collapsed", "shrunk", "non_finite"):  # (the knot stays where it was: it hides what it hid)
            keep = other & (hits[2] == 1)
            assert keep.sum() > 200 and same(hits[0][keep], first_hits[0][keep])
    assert same(img, first)  # back to the original: the creation handle's first frame
    g.close()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 257, 1536])
def test_sizes(n):
    """the root leaf, the device builder's threshold, block tails"""
    p = params()
    options = {"device_build_min": 16}
    g = handle(base_scene(KNOT[:n].copy()), **options)
    tris = sine(KNOT[:n])
    g.set_mesh(0, tris)
    check_against_fresh(g, base_scene(tris), p, options, "n = %d" % n)
    g.close()


def test_a_tree_that_becomes_one_leaf_and_back():
    """every triangle the same: no split separates them, the 1 536 entries are the root's"""
    p = params()
    g = handle(base_scene(KNOT))
    first = g.render_batch(CAM, p)
    tris = np.tile(KNOT[:1], (len(KNOT), 1))
    assert tree_of(tris)["max_depth"] == 0
    g.set_mesh(0, tris)
    check_against_fresh(g, base_scene(tris), p, {}, "one leaf")
    g.set_mesh(0, KNOT)
    assert same(g.render_batch(CAM, p), first)
    g.close()


def two_instances(tris):
    s = base_scene(tris)
    s.objects[1] = Object(Mesh(tris).scale((1.4, 1.4, 1.4)).rotate_x(0.5).translate((1.5, 0.1, 0.4))) \
        .material(Material.specular((0.3, 0.6, 0.9), 0.2))
    return s


def test_two_instances_of_one_mesh_both_follow():
    p = params()
    g = handle(two_instances(KNOT))
    tris = sine(KNOT, 2.0)
    for index in (0, 1):  # named through either instance
        g.set_mesh(index, tris if index == 0 else KNOT)
        f = handle(two_instances(tris if index == 0 else KNOT))
        assert same(g.render_batch(CAM, p), f.render_batch(CAM, p))
        hit_g, hit_f = g.closest_hit(*RAYS), f.closest_hit(*RAYS)
        for a, b in zip(hit_g, hit_f):
            assert same(a, b)
        assert (hit_g[2] == 0).sum() > 200 and (hit_g[2] == 1).sum() > 200
        f.close()
    g.close()


def test_device_entry_point_on_a_torch_tensor():
    torch = pytest.importorskip("torch")
    p = params()
    tris = sine(KNOT, 0.5)
    g = handle(base_scene(KNOT))
    g.set_mesh(0, tris)
    host_bits = g.render_batch(CAM, p)
    g.set_mesh(0, KNOT)
    t = torch.from_numpy(tris).to("cuda:0")
    before = t.clone()
    g.set_mesh(0, t)
    assert same(g.render_batch(CAM, p), host_bits)  # the host entry point's bits
    assert torch.equal(t, before)                   # an untouched input
    # a producer on a side stream: the call waits for torch's current stream
    g.set_mesh(0, KNOT)
    side = torch.cuda.Stream()
    base = torch.from_numpy(KNOT).to("cuda:0")
    delta = torch.from_numpy(tris - KNOT).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        made = base.clone()
        for _ in range(64):  # (work that is still running when the call is made)
            made = made + delta / 64.0 - delta / 64.0
        made = base + delta
        g.set_mesh(0, made)
    side.synchronize()
    f = handle(base_scene(made.cpu().numpy()))
    assert same(g.render_batch(CAM, p), f.render_batch(CAM, p))
    f.close()
    g.close()


def test_aov_rays_probes_and_buffer_across_an_update():
    p = params()
    tris = sine(KNOT, 3.0)
    g = handle(base_scene(KNOT))
    buf = DeviceBuffer(g, W, H)  # made before the update, sampled after it: it stays valid
    g.set_mesh(0, tris)
    f = handle(base_scene(tris))
    fbuf = DeviceBuffer(f, W, H)
    for base in (0, 4):
        pb = make_params(W, H, 3, 4, seed=0x4D45, sample_index_base=base)
        buf.sample(CAM, pb)
        fbuf.sample(CAM, pb)
    assert buf.num_batches() == 2 and same(buf.totals(), fbuf.totals()) and same(buf.image(), fbuf.image())
    a, b = g.render_aov(CAM, p), f.render_aov(CAM, p)
    assert sorted(a) == sorted(b)
    for k in a:
        assert same(a[k], b[k]), k
    o, d = rays(64, seed=9)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    assert same(g.trace_rays(o, d, 3, samples=4, seed=7), f.trace_rays(o, d, 3, samples=4, seed=7))
    pos = np.random.default_rng(2).uniform(-1.0, 1.0, (8, 3)) + np.array([0.0, 0.5, 1.5])
    kw = dict(kind=_abi.RPT_PROBE_SH9, samples=16, max_bounces=3, seed=11)
    assert same(g.bake_probes(pos, **kw), f.bake_probes(pos, **kw))
    for x in (buf, fbuf):
        x.close()
    f.close()
    g.close()


def test_set_mesh_and_update_in_either_order():
    p = params()
    tris = sine(KNOT, 4.0)
    moved = dict(at=(-0.2, 0.4, -0.5), turn=1.1)
    f = handle(base_scene(tris, **moved))
    want = f.render_batch(CAM, p)
    f.close()
    for mesh_first in (True, False):
        g = handle(base_scene(KNOT))
        if mesh_first:
            g.set_mesh(0, tris)
        g.update(base_scene(KNOT, **moved))  # (placements and materials only: the geometry is the creation's)
        if not mesh_first:
            g.set_mesh(0, tris)
        assert same(g.render_batch(CAM, p), want)
        g.close()


def test_one_frame_against_the_oracle(oracle):
    p = params()
    tris = sine(KNOT, 5.0)
    g = handle(base_scene(KNOT))
    g.set_mesh(0, tris)
    ref = oracle.OracleScene(base_scene(tris)).render(CAM, p, threads=0)
    assert same(g.render_batch(CAM, p), ref)
    g.close()


def refused(g, call, message, p, first):
    with pytest.raises(RptGpuError) as e:
        call()
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and message in str(e.value), str(e.value)
    assert same(g.render_batch(CAM, p), first)  # an unchanged next frame


def test_refusals_leave_the_handle_as_it_was():
    p = params()
    g = handle(base_scene(KNOT))
    first = g.render_batch(CAM, p)
    lib, T = g.lib, _abi.C.POINTER(_abi.RptTriangle)

    def null_array():
        _abi.check(lib.rptgpu_scene_set_mesh(g.handle, 0, len(KNOT), T()), g.handle)

    def null_device_array():
        _abi.check(lib.rptgpu_scene_set_mesh_device(g.handle, 0, len(KNOT), None, None), g.handle)

    for call, message in ((lambda: g.set_mesh(4, KNOT), "object 4 is out of range (the scene has 4)"),
                          (lambda: g.set_mesh(2, KNOT), "object 2 is not a mesh"),
                          (lambda: g.set_mesh(3, KNOT), "object 3 is not a mesh"),
                          (lambda: g.set_mesh(0, KNOT[:100]), "n = 100 differs from the triangle count of object 0 at creation (1536)"),
                          (lambda: g.set_mesh(1, KNOT), "n = 1536 differs from the triangle count of object 1 at creation (384)"),
                          (null_array, "rptgpu_scene_set_mesh: null triangle array"),
                          (null_device_array, "rptgpu_scene_set_mesh_device: null triangle array")):
        refused(g, call, message, p, first)
    g.close()


def small_flat_scene():
    s = Scene()
    s.add(Object(polygon([(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (1.0, 1.0, 0.0), (-1.0, 1.0, 0.0)]).rotate_y(0.3)).material(Material.diffuse((0.8, 0.5, 0.3))))
    s.add(Object(sphere().scale((0.4, 0.4, 0.4)).translate((0.0, 0.0, 1.5))).material(Material.diffuse((0.7, 0.7, 0.7))))
    s.add(Light.Point((30.0, 30.0, 30.0), (-2.0, 4.0, 4.0)))
    return s


def test_meshes_that_need_a_new_handle_are_refused_by_name():
    p = params()
    # every tree one leaf, default deep_depth: the flat path kernel's LDS layout holds the mesh
    s = small_flat_scene()
    g = GpuScene(s, 0)
    first = g.render_batch(CAM, p)
    tris = s.objects[0].shape.shape.triangles
    refused(g, lambda: g.set_mesh(0, tris), "flat path kernel", p, first)
    refused(g, lambda: g.set_mesh(0, tris), "needs a new handle", p, first)
    g.close()
    # a group's child and a Light::Object's shape: instances of the tree of object 0
    for extra, message in ((lambda s: s.add(Object(KdTree([Mesh(KNOT).translate((0.0, 2.0, -3.0)), sphere().translate((2.0, 2.0, -3.0))]))),
                            "also a Light::Object's shape or a group's child"),
                           (lambda s: s.add(Light.Object(Object(Mesh(KNOT).translate((0.0, 3.0, 0.0))).material(Material.light((1.0, 1.0, 1.0), 5.0)))),
                            "also a Light::Object's shape or a group's child")):
        s = base_scene(KNOT)
        extra(s)
        g = handle(s)
        first = g.render_batch(CAM, p)
        refused(g, lambda: g.set_mesh(0, sine(KNOT)), message, p, first)
        if len(s.objects) == 5:
            refused(g, lambda: g.set_mesh(4, sine(KNOT)), "object 4 is not a mesh", p, first)  # the group itself
        g.close()
