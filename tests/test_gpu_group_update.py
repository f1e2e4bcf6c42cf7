"""A group whose children move on a live scene handle (rptgpu_scene_set_group[_device], GpuScene.set_group) on a real
MI355X.  The contract: after the call every result — frames under every pipeline flag,
rptgpu_closest_hit, rptgpu_render_aov, rptgpu_trace_rays, rptgpu_bake_probes, the device Buffer — is BIT-EQUAL to that of
a handle freshly created from the scene in which the group has the new children, and a refused call leaves the handle
rendering what it rendered before.  Every comparison here is tobytes() equality against such a fresh handle.

The one test that needs no GPU (the motions do what their names say, by the library's host kd builder) is not marked."""
import math

import numpy as np
import pytest

from rpt_amd import (Camera, DeviceBuffer, GpuScene, KdTree, Light, Material, Mesh, MonomialSurface, Object, RptGpuError,
                     Scene, Transformed, _abi, cube, make_params, plane, scenes, sphere, transform_records)
from rpt_amd.device import kdtree_build

gpu = pytest.mark.gpu

W, H = 64, 48
FLAGS = {"default": 0, "wavefront": _abi.RPT_FLAG_WAVEFRONT, "persistent": _abi.RPT_FLAG_PERSISTENT,
         "general": _abi.RPT_FLAG_GENERAL_TRAVERSAL}
OTHER = scenes.knot_mesh(nu=24, nv=8, seed=3)  # 384 triangles: the mesh that stays
assert OTHER.shape == (384, 18)
CAM = Camera()
ROUTES = {"in_kernel": {}, "per_tree": {"deep_depth": 1}}  # how the handle walks G


def params(flags=0, spp=4, bounces=3, seed=0x4752):
    return make_params(W, H, bounces, spp, seed=seed, flags=flags)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- children: (kind, A) with A the 4x4 placement (None: the child is not Transformed)
def translation(v):
    a = np.eye(4)
    a[:3, 3] = v
    return a


def scaling(v):
    return np.diag([v[0], v[1], v[2], 1.0])


def rotation_y(t):
    a = np.eye(4)
    a[0, 0], a[0, 2], a[2, 0], a[2, 2] = math.cos(t), math.sin(t), -math.sin(t), math.cos(t)
    return a


def about(c, m):
    return translation(c) @ m @ translation(-np.asarray(c))


def make_children(n, seed=11, plain=(5, 6)):
    """spheres and cubes mixed over [-2, 2]^3, radii 0.15 .. 0.4; the children `plain` are not Transformed"""
    rng = np.random.default_rng(seed)
    kids = []
    for i in range(n):
        kind = "cube" if i % 3 == 0 else "sphere"
        r = rng.uniform(0.15, 0.4)
        a = translation(rng.uniform(-2.0, 2.0, 3)) @ rotation_y(rng.uniform(0.0, 3.0)) @ scaling((r, 1.3 * r, 0.8 * r))
        kids.append((kind, None if i in plain and n > max(plain) else a))
    return kids


def shapes(kids):
    out = []
    for kind, a in kids:
        base = cube() if kind == "cube" else sphere()
        out.append(base if a is None else Transformed(base, [float(x) for x in a.T.ravel()]))
    return out


KIDS = make_children(40)
STAY = [("sphere", translation(p) @ scaling((0.12, 0.12, 0.12)))
        for p in np.random.default_rng(4).uniform(-0.7, 0.7, (20, 3))]


def moved(kids, f):
    """f(i, A) -> the new placement, for the Transformed children"""
    return [(kind, None if a is None else f(i, a)) for i, (kind, a) in enumerate(kids)]


# ---- the motions of the issue, each a function of the creation's children
def jitter(kids, seed=1):
    rng = np.random.default_rng(seed)
    return moved(kids, lambda i, a: translation(rng.uniform(-0.1, 0.1, 3)) @ a)


def spread(kids):
    return moved(kids, lambda i, a: about((40.0, -25.0, 10.0), scaling((1000.0, 1000.0, 1000.0))) @ a)


def flattened(kids):
    return moved(kids, lambda i, a: scaling((1.0, 0.0, 1.0)) @ a)  # (singular: inverse_transform and normal_transform are zeros)


def clustered(kids):
    rng = np.random.default_rng(4)
    pull = rng.uniform(size=len(kids)) < 0.9
    return moved(kids, lambda i, a: about((0.3, -0.2, 0.1), scaling((1e-3, 1e-3, 1e-3))) @ a if pull[i] else a)


def coincident(kids):
    first = next(a for _, a in kids if a is not None)
    return moved(kids, lambda i, a: first.copy())


def tiny(kids):
    return moved(kids, lambda i, a: about(a[:3, 3], scaling((1e-3, 1e-3, 1e-3))) @ a)


def non_finite(kids):
    out = jitter(kids, seed=3)
    out[10][1][1, 3] = math.nan
    out[30][1][0, 0] = math.inf
    return out


MOTIONS = [("jitter", jitter), ("spread", spread), ("flattened", flattened), ("clustered", clustered),
           ("coincident", coincident), ("tiny", tiny), ("non_finite", non_finite), ("original", lambda kids: list(kids))]


# ---- what the library's host builder makes of the children's boxes (numpy: for what a test says about a motion)
def boxes_of(kids):
    out = []
    for kind, a in kids:
        h = 0.5 if kind == "cube" else 1.0
        corners = np.array([[x, y, z, 1.0] for x in (-h, h) for y in (-h, h) for z in (-h, h)])
        if a is not None:
            corners = corners @ a.T
        out.append(np.concatenate([corners[:, :3].min(axis=0), corners[:, :3].max(axis=0)]))
    return np.array(out)


def tree_of(kids):
    return kdtree_build(boxes_of(kids))


def unfiltered_spheres(kids):
    """the Transformed spheres the leaf filter leaves alone (shape_records.h quadric_too_small), on the grid of these children"""
    b = boxes_of(kids)
    step = ((b[:, 3:].max(axis=0) - b[:, :3].min(axis=0)) / 65529.0).max()
    count = 0
    for kind, a in kids:
        if kind == "sphere" and a is not None:
            count += not (1.0 / np.linalg.norm(np.linalg.inv(a)[:3, :3]) >= 64.0 * step)
    return count


def test_the_motions_do_what_their_names_say():
    base, deep = tree_of(KIDS), tree_of(clustered(KIDS))
    assert base["max_depth"] >= 1
    assert deep["max_depth"] > base["max_depth"] and len(deep["refs"]) > len(base["refs"])
    one = tree_of(coincident(KIDS))
    assert one["max_depth"] == 0 and len(one["refs"]) == len(KIDS)
    spheres = sum(1 for kind, a in KIDS if kind == "sphere" and a is not None)
    assert unfiltered_spheres(KIDS) == 0 and unfiltered_spheres(tiny(KIDS)) == spheres > 20
    assert tree_of(STAY)["max_depth"] >= 1  # the group that stays is a real tree: no handle here is all-flat
    rec = transform_records(shapes(flattened(KIDS)))
    assert (rec[0, 25:50] == 0.0).all() and not (rec[0, :16] == 0.0).all()  # singular: a zero inverse, as glm::inverse gives


# ---- scenes and handles
def place(group):
    return group.scale((0.45, 0.45, 0.45)).rotate_y(0.4).translate((-0.7, 0.2, 0.0))


def base_scene(kids, placed=True, stay=STAY):
    """G (object 0), a second group created after it, the knot, a plane, a point light, a Light::Object sphere"""
    s = Scene()
    g = KdTree(shapes(kids))
    s.add(Object(place(g) if placed else g).material(Material.diffuse((0.8, 0.5, 0.3))))
    s.add(Object(KdTree(shapes(stay)).translate((1.5, 0.4, 0.6))).material(Material.specular((0.3, 0.6, 0.9), 0.2)))
    s.add(Object(Mesh(OTHER).scale((1.3, 1.3, 1.3)).translate((1.3, -0.9, 1.2))).material(Material.diffuse((0.7, 0.7, 0.7))))
    s.add(Object(plane((0.0, 1.0, 0.0), -1.6)).material(Material.diffuse((0.6, 0.6, 0.6))))
    s.add(Light.Point((30.0, 30.0, 30.0), (-2.0, 4.0, 4.0)))
    s.add(Light.Object(Object(sphere().scale((0.3, 0.3, 0.3)).translate((1.0, 2.4, 2.0))).material(Material.light((1.0, 0.9, 0.8), 40.0))))
    return s


def rays(n=20000, seed=5):
    """from around the eye towards both groups, the knot and the floor"""
    rng = np.random.default_rng(seed)
    o = np.tile([0.0, 0.0, 10.0], (n, 1)) + rng.uniform(-0.2, 0.2, (n, 3))
    d = np.stack([rng.uniform(-0.28, 0.28, n), rng.uniform(-0.2, 0.2, n), -np.ones(n)], axis=1)
    return o, d


RAYS = rays()
PROBES = np.random.default_rng(2).uniform(-1.0, 1.0, (8, 3)) + np.array([0.0, 0.5, 1.5])
PROBE_KW = dict(kind=_abi.RPT_PROBE_SH9, samples=16, max_bounces=3, seed=11)
_ORIGINAL = {}


def original_handle_results(route):
    """what a handle of the creation's scene gives, computed once per route: the first frame, the hits, one Buffer batch"""
    if route not in _ORIGINAL:
        f = GpuScene(base_scene(KIDS), 0, **ROUTES[route])
        buf = DeviceBuffer(f, W, H)
        buf.sample(CAM, make_params(W, H, 3, 4, seed=0x4752, sample_index_base=0))
        _ORIGINAL[route] = {"frame": f.render_batch(CAM, params()), "hits": f.closest_hit(*RAYS), "totals": buf.totals()}
        buf.close()
        f.close()
    return _ORIGINAL[route]


def check_frames_and_hits(g, f, what, flags=FLAGS):
    for mode in sorted(flags):
        p = params(flags=flags[mode])
        got, want = g.render_batch(CAM, p), f.render_batch(CAM, p)
        assert same(got, want), "%s, %s: frame differs in %d values" % (what, mode, (got != want).sum())
    hit_g, hit_f = g.closest_hit(*RAYS), f.closest_hit(*RAYS)
    for a, b in zip(hit_g, hit_f):
        assert same(a, b), "%s: closest_hit differs" % what
    return hit_g


@gpu
@pytest.mark.parametrize("motion", [name for name, _ in MOTIONS])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_motions_equal_a_fresh_handle(route, motion, oracle):
    kids = dict(MOTIONS)[motion](KIDS)
    scene = base_scene(kids)
    first = original_handle_results(route)
    g = GpuScene(base_scene(KIDS), 0, **ROUTES[route])
    buf = DeviceBuffer(g, W, H)  # samples before and after the update
    buf.sample(CAM, make_params(W, H, 3, 4, seed=0x4752, sample_index_base=0))
    g.set_group(0, shapes(kids))
    f = GpuScene(scene, 0, **ROUTES[route])
    hits = check_frames_and_hits(g, f, motion)
    assert (first["hits"][2] == 0).sum() > 200, "the rays reach G"
    stays = (first["hits"][2] == 1) & (hits[2] == 1)
    if motion in ("jitter", "original", "tiny", "non_finite"):  # (G stays where it was: the other group is hit where it was)
        assert stays.sum() > 100 and same(hits[0][stays], first["hits"][0][stays])
    # the Buffer: the batch before the update is the creation scene's, the batch after it a fresh handle's
    fbuf = DeviceBuffer(f, W, H)
    later = make_params(W, H, 3, 4, seed=0x4752, sample_index_base=4)
    buf.sample(CAM, later)
    fbuf.sample(CAM, later)
    assert buf.num_batches() == 2 and same(buf.totals(), first["totals"] + fbuf.totals())
    a, b = g.render_aov(CAM, params()), f.render_aov(CAM, params())
    assert sorted(a) == sorted(b)
    for k in a:
        assert same(a[k], b[k]), k
    o, d = rays(64, seed=9)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    assert same(g.trace_rays(o, d, 3, samples=4, seed=7), f.trace_rays(o, d, 3, samples=4, seed=7))
    assert same(g.bake_probes(PROBES, **PROBE_KW), f.bake_probes(PROBES, **PROBE_KW))
    ref = oracle.OracleScene(scene).render(CAM, params(), threads=0)
    assert same(g.render_batch(CAM, params()), ref)
    if motion == "original":
        assert same(g.render_batch(CAM, params()), first["frame"])
    for x in (buf, fbuf, f, g):
        x.close()


@gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_sequence_of_updates_on_one_handle(route):
    g = GpuScene(base_scene(KIDS), 0, **ROUTES[route])
    for name in ("clustered", "coincident", "jitter", "spread", "tiny", "original"):  # deeper, one leaf, a tree again, ...
        kids = dict(MOTIONS)[name](KIDS)
        g.set_group(0, shapes(kids))
        f = GpuScene(base_scene(kids), 0, **ROUTES[route])
        check_frames_and_hits(g, f, name, {"default": 0, "wavefront": _abi.RPT_FLAG_WAVEFRONT})
        f.close()
    assert same(g.render_batch(CAM, params()), original_handle_results(route)["frame"])
    g.close()


@gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 150, 750])
def test_child_counts(n):
    """the root leaf (next to the real trees of the other group and the knot), the device builder's threshold, block
    tails; G itself not Transformed"""
    options = {"device_build_min": 16}
    kids = make_children(n, seed=20 + n)
    g = GpuScene(base_scene(kids, placed=False), 0, **options)
    new = jitter(kids, seed=n)
    g.set_group(0, shapes(new))
    f = GpuScene(base_scene(new, placed=False), 0, **options)
    check_frames_and_hits(g, f, "n = %d" % n, {"default": 0, "wavefront": _abi.RPT_FLAG_WAVEFRONT})
    f.close()
    g.close()


@gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_device_builder_builds_the_groups_tree(route):
    options = dict(ROUTES[route], device_build_min=16)
    g = GpuScene(base_scene(KIDS), 0, **options)
    for name in ("jitter", "clustered", "non_finite"):  # (non-finite boxes: kdbuild.hip refuses them, the host builds)
        kids = dict(MOTIONS)[name](KIDS)
        g.set_group(0, shapes(kids))
        f = GpuScene(base_scene(kids), 0, **options)
        check_frames_and_hits(g, f, name, {"default": 0})
        f.close()
    g.close()


@gpu
def test_records_from_numpy_and_from_a_torch_tensor_give_the_host_entrys_bits():
    torch = pytest.importorskip("torch")
    p = params()
    kids = jitter(KIDS, seed=8)
    rec = transform_records(shapes(kids))
    assert rec.shape == (40, 51) and rec.dtype == np.float64
    g = GpuScene(base_scene(KIDS), 0)
    g.set_group(0, shapes(kids))
    host_bits = g.render_batch(CAM, p)
    assert not same(host_bits, original_handle_results("in_kernel")["frame"])
    for source in (rec, torch.from_numpy(rec).to("cuda:0")):
        g.set_group(0, shapes(KIDS))
        g.set_group(0, source)
        assert same(g.render_batch(CAM, p), host_bits)
    # a producer on a side stream: the call waits for torch's current stream
    g.set_group(0, shapes(KIDS))
    side = torch.cuda.Stream()
    base = torch.from_numpy(transform_records(shapes(KIDS))).to("cuda:0")
    delta = torch.from_numpy(rec - transform_records(shapes(KIDS))).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        made = base.clone()
        for _ in range(64):  # (work that is still running when the call is made)
            made = made + delta / 64.0 - delta / 64.0
        made = base + delta
        before = made.clone()
        g.set_group(0, made)
    side.synchronize()
    assert torch.equal(made, before)  # an untouched input
    # (base + delta need not be rec to the bit: the reference is a handle made from the records themselves)
    n = GpuScene(base_scene(KIDS), 0)
    n.set_group(0, made.cpu().numpy())
    assert same(g.render_batch(CAM, p), n.render_batch(CAM, p))
    n.close()
    g.close()


@gpu
def test_set_group_and_update_in_either_order():
    p = params()
    kids = jitter(KIDS, seed=9)

    def turned(k):
        s = base_scene(k)
        s.objects[0] = Object(KdTree(shapes(k)).scale((0.5, 0.5, 0.5)).rotate_y(1.1).translate((-0.4, 0.4, -0.5))) \
            .material(Material.diffuse((0.2, 0.7, 0.3)))
        return s

    f = GpuScene(turned(kids), 0)
    want = f.render_batch(CAM, p)
    f.close()
    for group_first in (True, False):
        g = GpuScene(base_scene(KIDS), 0)
        if group_first:
            g.set_group(0, shapes(kids))
        g.set_objects([0], [turned(KIDS).objects[0]])  # (the placement and material of G itself)
        if not group_first:
            g.set_group(0, shapes(kids))
        assert same(g.render_batch(CAM, p), want)
        g.close()


# ---- refusals: each leaves the handle rendering what it rendered before
def refused(g, call, message, p, first):
    with pytest.raises(RptGpuError) as e:
        call()
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and message in str(e.value), str(e.value)
    assert same(g.render_batch(CAM, p), first)  # an unchanged next frame


@gpu
def test_refusals_leave_the_handle_as_it_was():
    p = params()
    g = GpuScene(base_scene(KIDS), 0)
    first = g.render_batch(CAM, p)
    lib, S = g.lib, _abi.C.POINTER(_abi.RptShape)
    new = shapes(jitter(KIDS))

    def null_array():
        _abi.check(lib.rptgpu_scene_set_group(g.handle, 0, len(KIDS), S()), g.handle)

    def null_device_array():
        _abi.check(lib.rptgpu_scene_set_group_device(g.handle, 0, len(KIDS), None, None), g.handle)

    def other_kind():
        k = list(new)
        k[1] = Transformed(cube(), k[1].transform_m)  # (child 1 was a sphere)
        g.set_group(0, k)

    def dropped_transformed():
        k = list(new)
        k[2] = sphere()
        g.set_group(0, k)

    def added_transformed():
        k = list(new)
        k[5] = sphere().translate((0.1, 0.0, 0.0))
        g.set_group(0, k)

    for call, message in ((lambda: g.set_group(4, new), "object 4 is out of range (the scene has 4)"),
                          (lambda: g.set_group(2, new), "object 2 is not a group"),
                          (lambda: g.set_group(3, new), "object 3 is not a group"),
                          (lambda: g.set_group(0, new[:10]), "n = 10 differs from the child count of object 0 at creation (40)"),
                          (lambda: g.set_group(1, new), "n = 40 differs from the child count of object 1 at creation (20)"),
                          (null_array, "rptgpu_scene_set_group: null children array"),
                          (null_device_array, "rptgpu_scene_set_group_device: null transform array"),
                          (other_kind, "child 1 of object 0: shape kind 2 differs from the kind at creation (0)"),
                          (dropped_transformed, "child 2 of object 0: the shape is not Transformed and was at creation"),
                          (added_transformed, "child 5 of object 0: the shape is Transformed and was not at creation")):
        refused(g, call, message, p, first)
    for call in (other_kind, dropped_transformed, added_transformed):
        refused(g, call, "needs a new handle", p, first)
    g.close()


@gpu
def test_groups_that_need_a_new_handle_are_refused_by_name():
    p = params()
    # a mesh, a monomial surface or a group among the children
    for extra in (Mesh(OTHER).translate((0.0, 0.5, 0.0)), MonomialSurface(1.0, 4.0).translate((0.0, 0.5, 0.0)),
                  KdTree([sphere().translate((0.0, 0.5, 0.0)), cube()])):
        s = base_scene(KIDS)
        kids = shapes(KIDS[:20]) + [extra]
        s.objects[0] = Object(place(KdTree(kids))).material(Material.diffuse((0.8, 0.5, 0.3)))
        g = GpuScene(s, 0)
        first = g.render_batch(CAM, p)
        refused(g, lambda: g.set_group(0, kids), "child 20 of object 0 is a mesh, a monomial surface or a group", p, first)
        refused(g, lambda: g.set_group(0, kids), "needs a new handle", p, first)
        g.close()
    # every tree one leaf, default deep_depth: the flat path kernel
    s = Scene()
    few = shapes(KIDS[:5])
    s.add(Object(KdTree(few)).material(Material.diffuse((0.8, 0.5, 0.3))))
    s.add(Object(sphere().scale((0.4, 0.4, 0.4)).translate((0.0, 0.0, 1.5))).material(Material.diffuse((0.7, 0.7, 0.7))))
    s.add(Light.Point((30.0, 30.0, 30.0), (-2.0, 4.0, 4.0)))
    g = GpuScene(s, 0)
    first = g.render_batch(CAM, p)
    refused(g, lambda: g.set_group(0, few), "flat path kernel", p, first)
    refused(g, lambda: g.set_group(0, few), "needs a new handle", p, first)
    g.close()
    # a rebuilt tree deeper than the stacks of the path kernels that walk G
    depth = tree_of(KIDS)["max_depth"]
    g = GpuScene(base_scene(KIDS), 0, fast_max_depth=depth)
    first = g.render_batch(CAM, p)
    deeper = shapes(clustered(KIDS))
    refused(g, lambda: g.set_group(0, deeper), "levels deep and object 0 is walked inside the path kernels, whose stacks hold %d" % depth, p, first)
    refused(g, lambda: g.set_group(0, deeper), "needs a new handle", p, first)
    g.set_group(0, shapes(jitter(KIDS)))  # (a tree within the stacks is taken)
    g.close()
    # the same group routed to the per-tree pipeline takes any depth
    g = GpuScene(base_scene(KIDS), 0, fast_max_depth=depth, deep_depth=1)
    g.set_group(0, deeper)
    f = GpuScene(base_scene(clustered(KIDS)), 0, fast_max_depth=depth, deep_depth=1)
    assert same(g.render_batch(CAM, p), f.render_batch(CAM, p))
    f.close()
    g.close()
    # an empty group (the C ABI's: Python's KdTree([]) is an empty Mesh): n == 0 is fine, and nothing is read
    s = base_scene(KIDS)
    s.add(Object(Mesh(np.zeros((0, 18)))).material(Material.diffuse((0.5, 0.5, 0.5))))
    desc, keep = s.lower()
    desc.objects[4].shape.kind = _abi.RPT_SHAPE_GROUP
    lib, h = _abi.load_library(), _abi.C.c_void_p()
    _abi.check(lib.rptgpu_scene_create(_abi.C.byref(desc), 0, _abi.C.byref(h)))
    try:
        assert lib.rptgpu_scene_set_group(h, 4, 0, None) == _abi.RPTGPU_OK
        assert lib.rptgpu_scene_set_group_device(h, 4, 0, None, None) == _abi.RPTGPU_OK
        assert lib.rptgpu_scene_set_group(h, 4, 1, None) == _abi.RPTGPU_E_INVALID_ARGUMENT
        assert b"n = 1 differs from the child count of object 4 at creation (0)" in lib.rptgpu_last_error_detail(h)
    finally:
        lib.rptgpu_scene_destroy(h)


# (Not reached by any test, as for rptgpu_scene_set_mesh: an abandoned handle — a handle is abandoned only when an aborted
# multi-GPU batch never drains — and 32-bit node or entry index overflow, which needs a scene of 2^32 leaf entries.)
