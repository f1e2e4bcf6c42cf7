"""Parity of the HIP path with the CPU oracle, through the C ABI, on a real MI355X.

Stated bar (parity mode = RPT_PRECISION_F64_STRICT, same seed, same sample count):
  * closest-hit records (t, normal, object): BIT-EQUAL;
  * framebuffer: BIT-EQUAL to the oracle — both sides evaluate IEEE f64 without FMA contraction and
    the same include/rpt_math.h transcendental functions.
Fast mode (FMA contraction) is compared statistically only (see the test).
"""
import os

import numpy as np
import pytest

import rpt_amd
from rpt_amd import GpuScene, _abi, make_params, scenes

import small_scenes
from test_golden import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            scene, cam, p = small_scenes.small(name)
            cache[name] = (scene, cam, p, GpuScene(scene, 0))
        return cache[name]

    yield get
    for v in cache.values():
        v[3].close()


def test_device_present():
    assert rpt_amd.device_count() >= 1


def test_device_math_is_bit_identical_to_host(oracle, built):
    g = built("sphere")[3]
    rs = np.random.RandomState(7)
    n = 1 << 20
    args = [(0, rs.uniform(-745, 709, n), None), (0, -rs.exponential(3.0, n), None),
            (1, rs.rand(n), None), (1, np.exp(rs.uniform(-700, 700, n)), None),
            (2, np.exp(rs.uniform(-30, 30, n)), None), (3, rs.uniform(0, np.pi / 2, n), None),
            (4, rs.uniform(0, np.pi / 2, n), None), (5, rs.uniform(-1, 1, n), None),
            (6, rs.randn(n), rs.randn(n))]
    for fn, x, y in args:
        a = g.eval_math(fn, x, y)
        b = oracle.math_eval(fn, x, y)
        assert (a.view(np.int64) == b.view(np.int64)).all(), fn
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-310, 1e300, 0.5, -0.5])
    # the kernels call the range-converged forms (csrc/math_converged.h): every boundary between two ranges of the five
    # functions, +- 3 ulps, both signs (the host-side sweep of the same: tests/test_math_converged.py)
    hi = np.array([0x44100000, 0x3fdc0000, 0x3e200000, 0x3fe60000, 0x3ff30000, 0x40038000, 0x3ff00000, 0x3fe00000, 0x3c600000,
                   0x40862E42, 0x3fd62e42, 0x3FF0A2B2, 0x3e300000, 0x4002d97c, 0x3fe921fb, 0x3ff921fb, 0x3e400000, 0x3FD33333,
                   0x3fe90000, 0x40874910, 0x4086232b], dtype=np.uint64)
    edges = ((hi[:, None, None] << np.uint64(32)) + np.array([0, 1, 0xffffffff], dtype=np.uint64)[None, :, None]
             + np.arange(-3, 4).astype(np.int64).view(np.uint64)[None, None, :]).ravel()
    edges = np.concatenate([edges, edges | np.uint64(1 << 63)]).view(np.float64)
    special = np.concatenate([special, edges])
    for fn in range(6):
        a, b = g.eval_math(fn, special), oracle.math_eval(fn, special)
        assert ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all(), fn
    yy, xx = np.meshgrid(special[:80], special[:80])
    a, b = g.eval_math(6, xx.ravel().copy(), yy.ravel().copy()), oracle.math_eval(6, xx.ravel().copy(), yy.ravel().copy())
    assert ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all()
    y1 = np.concatenate([rs.randn(2048), special])
    x1 = np.ones(len(y1))
    a, b = g.eval_math(6, x1, y1), oracle.math_eval(6, x1, y1)  # atan2(y, 1) = atan(y)
    assert ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all()


def test_shared_reciprocal_division_is_ieee(built):
    """Where several quotients share a denominator the kernels divide through a shared refined reciprocal
    (kernels.inc `div_fast`, guarded by `RcpD::ok` and `safe_range`); wherever that guard holds the result
    must be the correctly rounded IEEE quotient, bit for bit — numpy's `/` is the reference.  (In the
    kernels the guard is evaluated per wave and the other side is the plain division, so the guard can
    only select between two ways of computing the same bits.)"""
    g = built("sphere")[3]
    rs = np.random.RandomState(17)
    n = 1 << 22

    def rand_exp(lo, hi, size):
        m = rs.uniform(1.0, 2.0, size) * rs.choice([-1.0, 1.0], size)
        return np.ldexp(m, rs.randint(lo, hi, size))

    cases = [(rs.randn(n), rs.randn(n)), (rs.uniform(-600, 600, n), rs.uniform(-1, 1, n)),
             (rand_exp(-450, 450, n), rand_exp(-450, 450, n)),      # around the fast-path range edges
             (rand_exp(-1070, 1023, n), rand_exp(-1070, 1023, n)),  # denormals, overflow, underflow
             (rs.randint(-3, 4, n).astype(float), rs.randint(-3, 4, n).astype(float))]  # zeros, exact cases
    for k in range(20):  # more volume in the normal range: ~10^8 pairs in total
        cases.append((rand_exp(-30, 30, n), rand_exp(-30, 30, n)))
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, 1.7976931348623157e308, 2.0 ** -400,
                        2.0 ** 400, 2.0 ** -401, 3.0])
    yy, xx = np.meshgrid(special, special)
    cases.append((yy.ravel().copy(), xx.ravel().copy()))
    with np.errstate(all="ignore"):
        for y, x in cases:
            got = g.eval_math(7, x, y)
            ref = y / x
            same = (got.view(np.int64) == ref.view(np.int64)) | (np.isnan(got) & np.isnan(ref))
            assert same.all(), (y[~same][:4], x[~same][:4], got[~same][:4], ref[~same][:4])


@pytest.mark.parametrize("name", small_scenes.NAMES)
def test_closest_hit_bit_equal_to_golden_and_oracle(oracle, built, name):
    scene, cam, p, g = built(name)
    z = load(name)
    t, n, obj = g.closest_hit(z["ray_o"], z["ray_d"])
    assert (t == z["hit_t"]).all() and (n == z["hit_n"]).all() and (obj == z["hit_obj"]).all()
    # secondary rays: from the hit points towards random directions (as bounce / shadow rays are)
    osc = oracle.OracleScene(scene)
    hit = z["hit_obj"] >= 0
    pos = z["ray_o"][hit] + z["hit_t"][hit, None] * z["ray_d"][hit]
    rs = np.random.RandomState(5)
    reps = 40
    o = np.repeat(pos, reps, axis=0)
    d = rs.randn(len(o), 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t0, n0, ob0 = osc.closest_hit(o, d)
    t1, n1, ob1 = g.closest_hit(o, d)
    assert (t0 == t1).all() and (ob0 == ob1).all()
    assert (n0.view(np.int64) == n1.view(np.int64)).all()


def test_monomial_surface_rays_bit_equal_including_the_nan_quirk(oracle):
    # MonomialSurface::intersect on its own: random rays from every side, axis-parallel rays (zero
    # direction components: infinities in the slab test), and the exactly vertical corner ray for
    # which the reference's Newton step divides by -0 and reports a hit at time NaN
    scene = rpt_amd.Scene()
    scene.add(rpt_amd.Object(rpt_amd.monomial_surface(2.0, 4.0)))
    scene.add(rpt_amd.Object(rpt_amd.monomial_surface(0.7, 4.0).rotate_x(2.0).scale((1.5, 0.8, 1.1)).translate((2.5, 0.3, -0.4))))
    rs = np.random.RandomState(12)
    n = 20000
    o = rs.uniform(-3, 3, (n, 3)) * np.array([1.5, 1.0, 1.0]) + np.array([1.0, 1.0, 0.0])
    d = rs.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = np.eye(3)[rs.randint(0, 3, 400)] * rs.choice([-1.0, 1.0], 400)[:, None]
    o = np.concatenate([o, rs.uniform(-1, 1, (400, 3)) + np.array([0.0, 1.0, 0.0]) - 3.0 * axis,
                        np.array([[0.9, 5.0, 0.9], [0.0, 5.0, 0.0], [0.5, -1.0, 0.0]])])
    d = np.concatenate([d, axis, np.array([[0.0, -1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 1.0, 0.0]])])
    g = GpuScene(scene, 0)
    t1, n1, ob1 = g.closest_hit(o, d)
    g.close()
    t0, n0, ob0 = oracle.OracleScene(scene).closest_hit(o, d)
    # (NaN payloads / signs are not part of the contract: x86 and gfx950 generate different quiet NaNs)
    same_t = (t0.view(np.int64) == t1.view(np.int64)) | (np.isnan(t0) & np.isnan(t1))
    assert same_t.all(), (np.flatnonzero(~same_t)[:8], t0[~same_t][:8], t1[~same_t][:8])
    assert (ob0 == ob1).all(), np.flatnonzero(ob0 != ob1)[:8]
    same_n = (n0.view(np.int64) == n1.view(np.int64)) | (np.isnan(n0) & np.isnan(n1))
    assert same_n.all(), (np.flatnonzero(~same_n.all(axis=1))[:8])
    assert np.isnan(t1[-3]) and ob1[-3] >= 0 and abs(t1[-2] - 5.0) < 1e-9 and abs(t1[-1] - 1.125) < 1e-9
    assert (ob1[:n] >= 0).mean() > 0.05


PIPELINES = {"auto": 0, "persistent": _abi.RPT_FLAG_PERSISTENT, "wavefront": _abi.RPT_FLAG_WAVEFRONT,
             "persistent-general-traversal": _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_GENERAL_TRAVERSAL,
             "wavefront-general-traversal": _abi.RPT_FLAG_WAVEFRONT | _abi.RPT_FLAG_GENERAL_TRAVERSAL}


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
@pytest.mark.parametrize("name", small_scenes.NAMES)
def test_render_bit_equal_to_golden(built, name, pipeline):
    scene, cam, p, g = built(name)
    p = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=PIPELINES[pipeline])
    img = g.render_batch(cam, p)
    ref = load(name)["image"]
    assert np.isfinite(img).all()
    assert (img == ref).all(), "max |delta| = %g on %d pixels" % (np.abs(img - ref).max(), (img != ref).any(axis=1).sum())


@pytest.mark.parametrize("pipeline", ["auto", "persistent", "wavefront"])
@pytest.mark.parametrize("name", small_scenes.HI_NAMES)
def test_high_sample_render_bit_equal_to_golden(name, pipeline):
    # 256x144 at 32 spp: ~10^6 samples per scene, every one of them the oracle's bits
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    p = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=PIPELINES[pipeline])
    img = g.render_batch(cam, p)
    g.close()
    ref = load(name)["image"]
    assert (img == ref).all(), "max |delta| = %g on %d pixels" % (np.abs(img - ref).max(), (img != ref).any(axis=1).sum())


@pytest.mark.parametrize("route", ["per_tree", "per_tree_unsorted", "in_kernel", "default", "per_tree_zeros_rare", "per_tree_unsorted_zeros_rare"])
def test_axis_parallel_rays_and_origins_on_split_planes(oracle, route, monkeypatch):
    """Rays with one or two direction components exactly zero — and, among them, origins that lie exactly ON a split
    plane (or a face of the bounds) of an axis the ray does not move along, where the reference's (value - o) / d is
    0/0 = NaN — through rptgpu_closest_hit: with every tree sent through rpt_tree_enter / rpt_tree_trace /
    rpt_tree_general, with the in-kernel traversal (kd_intersect_fast and its restart in the general form), and with
    the defaults.  Bit-equal to the oracle."""
    from rpt_amd.device import kdtree_build
    if route.startswith("per_tree"):
        monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "1")
        monkeypatch.setenv("RPTGPU_SORT_RAYS", "0" if "unsorted" in route else "1")
        monkeypatch.setenv("RPTGPU_SORT_MIN_RAYS", "0")
    if route == "in_kernel":
        monkeypatch.setenv("RPTGPU_RAYS_IN_KERNEL", "1")
    # *_zeros_rare: no light makes zero components common, so the per-tree pipeline has no ZEROS launch and every such
    # ray of a tree goes through rpt_tree_generic (round 5)
    scene, cam = small_scenes.axis_sun(oblique=route.endswith("zeros_rare"))
    rows = np.asarray(scene.objects[0].shape.triangles)
    v = rows[:, :9].reshape(-1, 3, 3)
    boxes = np.concatenate([v.min(axis=1), v.max(axis=1)], axis=1)
    tree = kdtree_build(boxes)
    inner = np.flatnonzero((tree["info"] & 3) != 3)
    assert len(inner) > 100 and tree["regular"] == 1
    lo, hi = boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)
    rs = np.random.RandomState(11)
    n = 60000
    o = lo + rs.rand(n, 3) * (hi - lo) * 1.2 - 0.1 * (hi - lo)
    d = rs.randn(n, 3)
    ax = rs.randint(0, 3, n)
    d[np.arange(n), ax] = 0.0
    two = rs.rand(n) < 0.3
    d[np.arange(n)[two], (ax[two] + 1) % 3] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # a third of the origins ON a split plane of their zero axis: the root's, or any inner node's of that axis
    for i in range(0, n, 3):
        cand = inner[(tree["info"][inner] & 3) == ax[i]]
        node = 0 if ((tree["info"][0] & 3) == ax[i] and i % 2 == 0) else cand[rs.randint(len(cand))]
        o[i, ax[i]] = tree["split"][node]
    # and some ON the faces of the bounds (the root slab test's own 0/0)
    for i in range(1, n, 30):
        o[i, ax[i]] = (lo if i % 2 else hi)[ax[i]]
    with np.errstate(all="ignore"):
        assert np.isnan((tree["split"][0] - o[:, tree["info"][0] & 3]) / d[:, tree["info"][0] & 3]).sum() > 1000
    g = GpuScene(scene, 0)
    t0, n0, ob0 = oracle.OracleScene(scene).closest_hit(o, d)
    t1, n1, ob1 = g.closest_hit(o, d)
    g.close()
    assert (ob0 == 0).sum() > 5000 and (ob0 == 1).sum() > 50
    same_t = (t0.view(np.int64) == t1.view(np.int64)) | (np.isnan(t0) & np.isnan(t1))
    assert same_t.all(), (route, int((~same_t).sum()), np.flatnonzero(~same_t)[:5])
    assert (ob0 == ob1).all() and (n0.view(np.int64) == n1.view(np.int64)).all()


@pytest.mark.parametrize("route", ["default", "per_tree"])
@pytest.mark.parametrize("order,negative", small_scenes.MIXED_ZERO_ORDERS)
def test_rays_from_a_zero_split_plane_of_either_sign(oracle, order, negative, route, monkeypatch):
    """A mesh whose root split is a zero median of mixed-sign zeros (kdtree.rs:251-255: the stable sort's order among
    equal keys decides its sign; tests/test_kdtree.py) and rays that start ON that plane, from +0.0 and from -0.0, a
    third of them without motion along x: value - origin is a zero of either sign there, t_split a signed zero or 0/0.
    Hit records bit-equal to the oracle's, whose tree has the same signed split."""
    from rpt_amd.device import kdtree_build
    if route == "per_tree":
        monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "1")
        monkeypatch.setenv("RPTGPU_SORT_MIN_RAYS", "0")
    rows = small_scenes.mixed_zero_mesh(order)
    v = rows[:, :9].reshape(-1, 3, 3)
    tree = kdtree_build(np.concatenate([v.min(axis=1), v.max(axis=1)], axis=1))
    assert tree["info"][0] == 0 and tree["split"][0] == 0.0 and np.signbit(tree["split"][0]) == negative
    scene = small_scenes.Scene()
    scene.add(small_scenes.Object(small_scenes.Mesh(rows)).material(small_scenes.Material.diffuse(small_scenes.hex_color(0x808080))))
    rs = np.random.RandomState(5)
    n = 30000
    o = np.stack([np.where(rs.rand(n) < 0.5, 0.0, -0.0), rs.rand(n) * 0.5 - 0.1, rs.rand(n) * 0.5 - 0.1], axis=1)
    d = rs.randn(n, 3)
    d[::3, 0] = 0.0
    d[1::7, 0] = -0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[::5, 0] = rs.randn(len(o[::5])) * 0.5  # and some from either side
    g = GpuScene(scene, 0)
    t0, n0, ob0 = oracle.OracleScene(scene).closest_hit(o, d)
    t1, n1, ob1 = g.closest_hit(o, d)
    g.close()
    assert (ob0 == 0).sum() > 1000
    same_t = (t0.view(np.int64) == t1.view(np.int64)) | (np.isnan(t0) & np.isnan(t1))
    assert same_t.all(), (route, int((~same_t).sum()), np.flatnonzero(~same_t)[:5])
    assert (ob0 == ob1).all() and (n0.view(np.int64) == n1.view(np.int64)).all()


@pytest.mark.parametrize("name", ["dragon", "coverage", "fractal_spheres"])
def test_scene_options_route_like_the_environment_did(name, monkeypatch):
    """ABI v6: the routing knobs as RptSceneOptions fields (rptgpu_scene_create_opts) — every tree through the per-tree
    pipeline, every query sorted, leaf boxes off — give the golden frame like the environment variables of the same
    names; the handle reports what it runs with, and an environment variable still overrides the struct."""
    scene, cam, p = small_scenes.small(name)
    pw = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=_abi.RPT_FLAG_WAVEFRONT)
    g = GpuScene(scene, 0, deep_depth=1, sort_rays=1, sort_min_rays=0, leaf_boxes=0, paths_chunk=3)
    o = g.options()
    assert (o["deep_depth"], o["sort_rays"], o["sort_min_rays"], o["leaf_boxes"], o["paths_chunk"]) == (1, 1, 0, 0, 3)
    assert (o["sort_min_bytes"], o["workspace_bytes"]) == (8 << 20, 240 << 30)  # untouched fields: the defaults
    img = g.render_batch(cam, pw)
    g.close()
    assert (img == load(name)["image"]).all()
    monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "5")
    g = GpuScene(scene, 0, deep_depth=1)
    assert g.options()["deep_depth"] == 5
    g.close()


@pytest.mark.parametrize("batch", [1, 7, 256])
@pytest.mark.parametrize("name", ["cornell", "glass", "spheres", "simple_video"])
def test_work_item_pools_are_scheduling_only(name, batch):
    """A wave of rpt_paths claims work items in batches (RptSceneOptions::paths_batch, kernels/paths.inc fetch_item): one
    at a time as before round 5, an odd size, more than the frame has items per wave — the fixture's frame, and every
    sample rendered exactly once (the sample count of the stats)."""
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0, paths_batch=batch, paths_chunk=1 if batch == 7 else 0)
    assert g.options()["paths_batch"] == batch
    g.reset_stats()
    img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed,
                                          flags=_abi.RPT_FLAG_PERSISTENT))
    assert (img == load(name)["image"]).all(), (name, batch)
    assert g.stats().samples == p.width * p.height * p.iterations
    g.close()


@pytest.mark.parametrize("batch", [0, 1, 7, 256, 1024])
def test_work_counter_ends_within_the_bound_the_host_leaves_room_for(batch, monkeypatch, capfd):
    """The KERNEL's own bookkeeping, not a model of it: rpt_paths's 32-bit work counter after a launch, read back
    by the library (RPTGPU_PRINT_LAUNCH).  Every item is claimed (counter >= items) and the claims past the end stay within
    waves x (64 askers + one last claim of at most the batch) — what render_plan.h's item_limit leaves room for below
    2^32; the image being the fixture's says every item was rendered exactly once."""
    import re
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    scene, cam, p = small_scenes.small("cornell")
    g = GpuScene(scene, 0, paths_batch=batch)
    capfd.readouterr()
    img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed,
                                          flags=_abi.RPT_FLAG_PERSISTENT))
    err = capfd.readouterr().err
    g.close()
    assert (img == load("cornell")["image"]).all()
    found = re.findall(r"work counter: ended at (\d+) for (\d+) items; (\d+) waves, claims of at most (\d+): dead claims (-?\d+) of at most (\d+)", err)
    assert found, err[-500:]
    for ended, items, waves, claim, dead, bound in (tuple(int(x) for x in f) for f in found):
        assert ended >= items and dead == ended - items
        assert claim == (batch if batch else claim) and claim <= 1024
        assert 0 <= dead <= bound == waves * (64 + claim), (ended, items, waves, claim)


def _hdri_scene(kind):
    """glass.rs's pair of spheres, a ring of seven glass / metal / diffuse spheres (the object filter of flat scenes), a
    glass cube on a polygon with a lamp (a flat scene with its triangles in LDS) — each under a synthetic HDRI"""
    from rpt_amd import Camera, Environment, Light, Material, Object, Scene, cube, hex_color, polygon, sphere
    if kind == "glass":
        return small_scenes.small("glass")
    scene = Scene()
    scene.environment = Environment.Hdri(scenes.synthetic_hdri(128, 64, seed=21))
    if kind == "ring":
        mats = [Material.clear(1.5, 0.0001), Material.metallic_(hex_color(0xFFFFFF), 0.0001), Material.diffuse(hex_color(0x6F5D48))]
        for i in range(7):
            ang = 2.0 * math.pi * i / 7.0
            scene.add(Object(sphere().scale((0.45, 0.45, 0.45)).translate((1.4 * math.cos(ang), 1.4 * math.sin(ang), -0.3 * i)))
                      .material(mats[i % 3]))
        cam = Camera()
    else:
        scene.add(Object(cube().scale((0.8, 0.8, 0.8)).rotate_y(0.6).translate((0.0, 0.4, 0.0))).material(Material.clear(1.5, 0.0001)))
        scene.add(Object(polygon([(-3.0, 0.0, -3.0), (-3.0, 0.0, 3.0), (3.0, 0.0, 3.0), (3.0, 0.0, -3.0)]))
                  .material(Material.diffuse(hex_color(0x6F5D48))))
        scene.add(Light.Object(Object(sphere().scale((0.5, 0.5, 0.5)).translate((2.0, 3.0, 1.0)))
                               .material(Material.light(hex_color(0xFFFFFF), 40.0))))
        cam = Camera.look_at((2.5, 2.0, 3.5), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 0.7)
    return scene, cam, make_params(64, 48, 6, 4, seed=130)


@pytest.mark.parametrize("kind", ["glass", "ring", "cube"])
def test_parked_environment_lookups_are_scheduling_only(kind, oracle):
    """rpt_paths<.., PARK> parks the texture lookups of escaped rays in per-lane queues and drains them for the wave together
    (RptSceneOptions::env_park, kernels/paths.inc): bit-equal to the oracle with and without, through the three flat
    instantiations of the persistent kernel, at bounce limits of 1-3 — where the parked paths and the running one press
    against the record ring's bound — and of 12, with one sample per work item and with sixteen."""
    scene, cam, p = _hdri_scene(kind)
    osc = oracle.OracleScene(scene)
    for bounces, spp in ((p.max_bounces, p.iterations), (1, 16), (2, 16), (3, 16), (12, 8)):
        pr = make_params(p.width, p.height, bounces, spp, p.exposure_value, p.seed + bounces, flags=_abi.RPT_FLAG_PERSISTENT)
        ref = osc.render(cam, pr, threads=0)
        for park, chunk in ((1, 1), (1, 0), (0, 0)):
            g = GpuScene(scene, 0, env_park=park, paths_chunk=chunk)
            assert g.options()["env_park"] == park
            img = g.render_batch(cam, pr)
            g.close()
            assert (img == ref).all(), (kind, bounces, park, chunk)


@pytest.mark.parametrize("name", ["wine_glass", "monomial_glass", "pegasus", "metal"])
def test_texture_environments_through_the_other_instantiations(name):
    # (scenes whose wave has no LDS left for the queues look the environment up on the spot: the fixture's frame either way)
    scene, cam, p = small_scenes.small(name)
    for park in (1, 0):
        g = GpuScene(scene, 0, env_park=park)
        for flags in (_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_GENERAL_TRAVERSAL):
            img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=flags))
            assert (img == load(name)["image"]).all(), (name, park, flags)
        g.close()


def _thin_lens_scene(kernel):
    """-> (scene, focused camera): three spheres under a colour environment (rpt_paths<KdFlatG>), the polygon room at the
    smallest wall count whose objects (four walls and a cube, with the lamp) reach the object filter's threshold (KdFlatF), the
    small dragon's multi-leaf mesh (KdLds)"""
    from rpt_amd import Camera, Environment, Material, Object, Scene, hex_color, sphere
    if kernel == "KdFlatG":
        scene = Scene()
        scene.environment = Environment.Color((0.6, 0.7, 0.9))
        mats = [Material.clear(1.5, 0.0001), Material.metallic_(hex_color(0xFFFFFF), 0.1), Material.diffuse(hex_color(0x6F5D48))]
        for i in range(3):
            scene.add(Object(sphere().scale((0.6, 0.6, 0.6)).translate((1.4 * (i - 1), 0.1 * i, -0.8 * i))).material(mats[i]))
        return scene, Camera.look_at((0.3, 0.8, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.7).focus((0.0, 0.0, 0.0), 0.2)
    if kernel == "KdFlatF":
        scene, cam = _polygon_room(4)
        return scene, cam.focus((0.0, 0.0, 0.0), 0.15)
    scene, cam, _ = small_scenes.small("dragon")
    return scene, cam.focus(tuple(cam.eye[k] + 3.0 * cam.direction[k] for k in range(3)), 0.05)


@pytest.mark.parametrize("kernel", ["KdFlatG", "KdFlatF", "KdLds"])
def test_thin_lens_camera_through_the_instantiations_without_a_ray_stash(kernel, monkeypatch, capfd):
    """aperture > 0 where rpt_paths generates its camera rays in the loop itself (kernels/paths.inc: the ray-generation
    site of the instantiations without a stash repeats camera_ray's body): the persistent kernel's frame is the wavefront
    pipeline's, bit for bit, and the launch diagnostics name the instantiation."""
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    scene, cam = _thin_lens_scene(kernel)
    assert cam.aperture > 0.0
    g = GpuScene(scene, 0)
    frames = {}
    try:
        for flags in (_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT):
            g.reset_stats()
            capfd.readouterr()
            frames[flags] = g.render_batch(cam, make_params(64, 48, 3, 4, seed=131, flags=flags))
            lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]
            if flags == _abi.RPT_FLAG_PERSISTENT:
                assert g.stats().kernel_launches[_abi.RPT_K_PATHS] >= 1  # the persistent kernel ran
                assert lines and all(ln.startswith("rpt_paths<%s>" % kernel) for ln in lines), lines
    finally:
        g.close()
    a, b = frames[_abi.RPT_FLAG_PERSISTENT], frames[_abi.RPT_FLAG_WAVEFRONT]
    assert ((a == b) | (np.isnan(a) & np.isnan(b))).all(), (kernel, np.abs(a - b).max())
    assert (b != 0).any()


@pytest.mark.parametrize("sort", ["0", "1"])
@pytest.mark.parametrize("name", small_scenes.NAMES)
def test_per_tree_queries_and_ray_sorting_do_not_change_the_image(name, sort, monkeypatch):
    # every tree treated as "deep" (object-by-object queries with per-tree compaction and persistent
    # traversal), with and without the ray sort in front of the traversal: scheduling only
    monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "1")
    monkeypatch.setenv("RPTGPU_SORT_RAYS", sort)
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    pw = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=_abi.RPT_FLAG_WAVEFRONT)
    img = g.render_batch(cam, pw)
    g.close()
    assert (img == load(name)["image"]).all()


@pytest.mark.parametrize("reorder", ["0", "1"])
@pytest.mark.parametrize("name", small_scenes.NAMES)
def test_path_reorder_of_in_kernel_scenes_is_scheduling_only(name, reorder, monkeypatch):
    """Round 6: scenes whose trees are walked inside rpt_extend / rpt_shadow_rays get the paths of a depth re-ordered by ray
    key (dense path state makes the order free).  Forced on for every depth of every fixture (threshold 1 path) through the
    wavefront pipeline, and off: the fixture's frame either way."""
    monkeypatch.setenv("RPTGPU_PATH_REORDER", reorder)
    monkeypatch.setenv("RPTGPU_PATH_REORDER_MIN", "1")
    monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "1000")  # nothing is "deep": every tree in-kernel
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    pw = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=_abi.RPT_FLAG_WAVEFRONT)
    img = g.render_batch(cam, pw)
    g.close()
    assert (img == load(name)["image"]).all()


@pytest.mark.parametrize("knobs", [{"RPTGPU_LEAF_BOXES": "0"}, {"RPTGPU_SORT_RAYS": "1"},
                                   {"RPTGPU_LEAF_BOXES": "0", "RPTGPU_SORT_RAYS": "1"},
                                   {"RPTGPU_NEST_TRACE": "0"},  # kd-trees of kd-trees through rpt_tree_generic instead of rpt_nest_trace
                                   {"RPTGPU_NEST_TRACE": "0", "RPTGPU_LEAF_BOXES": "0"}])
@pytest.mark.parametrize("name", ["dragon", "wine_glass", "coverage", "fractal_spheres", "fractal_teapots", "nested_groups", "deep_nest", "seven_nest"])
def test_leaf_box_filter_and_ray_sort_are_scheduling_only(name, knobs, monkeypatch):
    # the conservative box filter switched off, and the ray sort forced on, with every tree sent through the per-tree
    # kernels: the same image as the fixture
    monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    for flags in (_abi.RPT_FLAG_WAVEFRONT, 0):
        img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=flags))
        assert (img == load(name)["image"]).all(), (name, knobs, flags)
    g.close()


@pytest.mark.parametrize("name", ["fractal_teapots", "nested_groups", "seven_nest"])
def test_groups_with_tree_children_take_the_per_tree_pipeline_whatever_is_asked(name):
    # a tree inside a tree is only walked by the per-tree kernels (rpt_nest_trace, rpt_tree_generic): RPT_FLAG_PERSISTENT
    # is a request such a scene cannot honour — the same image, and no launch of the persistent path kernel
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    for flags in (_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_GENERAL_TRAVERSAL, _abi.RPT_FLAG_GENERAL_TRAVERSAL):
        g.reset_stats()
        img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed,
                                              flags=flags | _abi.RPT_FLAG_PROFILE_KERNELS))
        assert (img == load(name)["image"]).all(), (name, flags)
        assert g.stats().kernel_launches[_abi.RPT_K_PATHS] == 0
    g.close()


@pytest.mark.parametrize("name", ["dragon", "wine_glass", "axis_sun", "fractal_teapots", "seven_nest"])
def test_trees_deeper_than_the_fast_stacks(name, monkeypatch, oracle):
    """A tree deeper than the in-kernel traversals' private stacks (KD_MAX_STACK = 32) is sent through the per-tree
    kernels, whose stack beyond the LDS levels is a global column as high as the scene's deepest tree, and a nested tree
    that deep through rpt_tree_generic.  The reference's build rule keeps real trees far below 32 (scene_plan.h route_object says why), so
    the threshold is lowered here (RPTGPU_FAST_MAX_DEPTH): every mesh of these fixtures is then "too deep"."""
    monkeypatch.setenv("RPTGPU_FAST_MAX_DEPTH", "3")
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    for flags in (0, _abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_GENERAL_TRAVERSAL):
        img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=flags))
        assert (img == load(name)["image"]).all(), (name, flags)
    z = load(name)
    t, n, obj = g.closest_hit(z["ray_o"], z["ray_d"])
    assert (t == z["hit_t"]).all() and (n == z["hit_n"]).all() and (obj == z["hit_obj"]).all()
    g.close()


def test_c1_full_config_bit_equal_to_oracle(oracle):
    # BASELINE configs[0]: examples/sphere.rs, 960x540, 2 bounces, 100 spp — in full
    scene, cam, cfg = scenes.sphere_scene()
    p = make_params(cfg["width"], cfg["height"], cfg["max_bounces"], cfg["num_samples"], seed=0x52505447)
    g = GpuScene(scene, 0)
    img = g.render_batch(cam, p)
    ref = oracle.OracleScene(scene).render(cam, p, threads=0)
    assert (img == ref).all()
    g.close()


def test_render_is_deterministic_and_seed_dependent(built):
    scene, cam, p, g = built("cornell")
    a = g.render_batch(cam, p)
    b = g.render_batch(cam, p)
    assert (a == b).all()
    p2 = make_params(p.width, p.height, p.max_bounces, p.iterations, seed=p.seed + 1)
    assert (g.render_batch(cam, p2) != a).any()


def test_partition_is_exact_and_image_independent_of_it(built):
    # Philox keyed by (pixel, sample) makes the image independent of the partition
    scene, cam, p, g = built("coverage")
    full = g.render_batch(cam, p)
    for parts, tile in ((2, (32, 8)), (3, (8, 4)), (8, (16, 16))):
        acc = np.zeros_like(full)
        for i in range(parts):
            pp = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed,
                             tile=tile, part=(i, parts))
            part = g.render_batch(cam, pp)
            assert ((part != 0).any(axis=1) & (acc != 0).any(axis=1)).sum() == 0  # disjoint
            acc += part
        assert (acc == full).all()


def test_batches_compose_like_iterative_render(built):
    # renderer.rs:103-115: sample(k) called repeatedly; with sample_index_base the batches are the
    # same paths as one big batch, so the batch means average to the full mean
    scene, cam, p, g = built("sphere")
    full = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, 8, seed=9))
    a = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, 4, seed=9, sample_index_base=0))
    b = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, 4, seed=9, sample_index_base=4))
    assert np.allclose((a + b) / 2.0, full, rtol=1e-14, atol=1e-300)
    assert (a != b).any()


def test_small_workspace_chunks_give_the_same_image(built, monkeypatch):
    # the per-pass sample chunking is an implementation detail: force tiny passes
    scene, cam, p, g = built("fractal_spheres")
    ref = g.render_batch(cam, p)
    monkeypatch.setenv("RPTGPU_TARGET_PATHS", "4096")
    g2 = GpuScene(scene, 0)
    pw = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=_abi.RPT_FLAG_WAVEFRONT)
    assert (g2.render_batch(cam, pw) == ref).all()
    g2.close()


@pytest.mark.parametrize("name", ["fractal_spheres", "dragon", "cornell", "glass"])
def test_a_pass_whose_record_pool_runs_out_starts_over(name, monkeypatch, capfd):
    """Round 6: depth records live in a pool of columns sized from a MEASURED average (columns per path).  A pass that needs
    more — another camera, a thin margin — must start over with room for more, having left nothing behind: forced here by
    claiming that a path needs a hundredth of a column (RPTGPU_REC_RATIO).  The fixture's frame, the sample count of ONE
    rendering, and the library says (RPTGPU_PRINT_LAUNCH) that it did start over."""
    monkeypatch.setenv("RPTGPU_REC_RATIO", "0.01")
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    scene, cam, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    g.reset_stats()
    capfd.readouterr()
    pw = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=_abi.RPT_FLAG_WAVEFRONT)
    img = g.render_batch(cam, pw)
    err = capfd.readouterr().err
    st = g.stats()
    g.close()
    assert (img == load(name)["image"]).all()
    assert st.samples == p.width * p.height * p.iterations
    if p.max_bounces > 0:
        assert "started over" in err, err[-400:]


def test_persistent_work_item_size_and_launch_split_do_not_change_the_image(built, monkeypatch):
    # samples per work item and the split of a batch into launches (per-sample radiance buffer cap)
    # are scheduling details: a pixel's samples are always summed in sample order
    for name in ("cornell", "sphere"):
        scene, cam, p, g = built(name)
        pp = make_params(p.width, p.height, p.max_bounces, 7, p.exposure_value, p.seed, flags=_abi.RPT_FLAG_PERSISTENT)
        ref = g.render_batch(cam, pp)
        for chunk, spp_cap in ((1, 7), (3, 7), (16, 2), (2, 3), (5, 1)):
            monkeypatch.setenv("RPTGPU_PATHS_CHUNK", str(chunk))
            monkeypatch.setenv("RPTGPU_LBUF_BYTES", str(p.width * p.height * 24 * spp_cap))
            g2 = GpuScene(scene, 0)
            pq = make_params(p.width, p.height, p.max_bounces, 7, p.exposure_value, p.seed,
                             flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_PROFILE_KERNELS)
            img = g2.render_batch(cam, pq)
            launches = g2.stats().kernel_launches[_abi.RPT_K_PATHS]
            g2.close()
            assert (img == ref).all(), (name, chunk, spp_cap)
            assert launches == -(-7 // spp_cap), (launches, spp_cap)


def test_removed_fast_mode_is_refused(built):
    # ABI v4: the FMA-contracted build (precision_mode 1) was slower than the parity build and not bit-exact; it is
    # gone, and asking for it is an error, not a silent strict render
    scene, cam, p, g = built("cornell")
    pf = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, precision=1)
    with pytest.raises(_abi.RptGpuError) as e:
        g.render_batch(cam, pf)
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and "precision_mode" in str(e.value)


def test_renderer_api_end_to_end(oracle):
    # the rpt builder API drives the GPU: render() -> image, iterative_render callback + variance
    scene, cam, _ = scenes.cornell()
    r = rpt_amd.Renderer(scene, cam).width(48).height(27).max_bounces(3).num_samples(6).seed(4).filter(rpt_amd.Filter.Box(1))
    img = r.render()
    assert img.shape == (27, 48, 3) and img.dtype == np.uint8 and img.max() > 50
    seen = []
    r.iterative_render(2, lambda it, buf: seen.append((it, buf.variance(), buf.image())))
    assert [s[0] for s in seen] == [2, 4, 6] and seen[-1][1] > 0
    # the three batches are exactly the oracle's batches
    osc = oracle.OracleScene(scene)
    b = rpt_amd.Buffer(48, 27, rpt_amd.Filter.Box(1))
    for i in range(3):
        b.add_samples(osc.render(cam, make_params(48, 27, 3, 2, seed=4, sample_index_base=2 * i), threads=0))
    assert (b.image() == seen[-1][2]).all()


def test_full_size_properties_cornell_1080p(oracle):
    """BASELINE configs[1] at its full frame size (1920x1080, 8 bounces; 2 spp instead of 512 —
    cost per sample is spp-independent): size-independent properties + an oracle spot check."""
    scene, cam, cfg = scenes.cornell()
    g = GpuScene(scene, 0)
    W, H, B = cfg["width"], cfg["height"], cfg["max_bounces"]
    p = make_params(W, H, B, 2, seed=77, flags=_abi.RPT_FLAG_PROFILE_KERNELS)
    g.reset_stats()
    full = g.render_batch(cam, p)
    st = g.stats()
    assert np.isfinite(full).all() and (full >= 0).all()
    assert st.samples == W * H * 2 and st.extend_rays >= st.samples and st.shadow_rays > 0
    assert st.kernel_ms[_abi.RPT_K_PATHS] > 0 and st.kernel_launches[_abi.RPT_K_PATHS] == 1  # auto -> persistent here
    # the wavefront pipeline gives the same bits and the same ray counts
    ext, sh = st.extend_rays, st.shadow_rays
    g.reset_stats()
    pw = make_params(W, H, B, 2, seed=77, flags=_abi.RPT_FLAG_PROFILE_KERNELS | _abi.RPT_FLAG_WAVEFRONT)
    assert (g.render_batch(cam, pw) == full).all()
    st = g.stats()
    assert all(st.kernel_ms[k] > 0 for k in range(5))
    assert (st.extend_rays, st.shadow_rays) == (ext, sh)
    # idempotence
    assert (g.render_batch(cam, p) == full).all()
    # partition: 8 interleaved parts sum to the frame
    acc = np.zeros_like(full)
    for i in range(8):
        acc += g.render_batch(cam, make_params(W, H, B, 2, seed=77, tile=(32, 8), part=(i, 8)))
    assert (acc == full).all()
    # oracle spot check at full size: 1/64 of the tiles, bit-equal
    pp = make_params(W, H, B, 2, seed=77, tile=(32, 8), part=(5, 64))
    part_gpu = g.render_batch(cam, pp)
    part_ref = oracle.OracleScene(scene).render(cam, pp, threads=0)
    assert (part_gpu == part_ref).all()
    sel = (part_ref != 0).any(axis=1)
    assert (full[sel] == part_ref[sel]).all()
    # symmetry-free sanity: the red wall is on the image's left, the green wall on its right
    img = full.reshape(H, W, 3)
    assert img[400:700, 250:350, 0].mean() > 2 * img[400:700, 250:350, 1].mean()
    assert img[400:700, 1570:1670, 1].mean() > 2 * img[400:700, 1570:1670, 0].mean()
    g.close()


def test_error_paths_on_device(built):
    scene, cam, p, g = built("sphere")
    with pytest.raises(rpt_amd.RptGpuError) as e:
        g.render_batch(cam, make_params(0, 10, 1, 1))
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT
    with pytest.raises(rpt_amd.RptGpuError):
        g.render_batch(cam, make_params(8, 8, 1, 1, part=(3, 2)))
    with pytest.raises(rpt_amd.RptGpuError):
        GpuScene(scene, 99)
    # empty scene: every pixel is the environment colour
    empty = rpt_amd.Scene()
    empty.environment = rpt_amd.Environment.Color((0.25, 0.5, 1.0))
    ge = GpuScene(empty, 0)
    img = ge.render_batch(rpt_amd.Camera(), make_params(16, 8, 3, 2))
    assert (img == np.array([0.25, 0.5, 1.0])).all()
    ge.close()


def test_another_callers_failed_hip_call_is_not_reported_as_this_calls(built):
    """hipGetLastError() reports the thread's LAST failed runtime call, whoever made it, until somebody reads it: every
    entry point starts from a clean slate (api_internal.h guarded).  A call of the process's own HIP runtime with an
    out-of-range ordinal — refused before any device is touched — stands for another library's failed call here.
    rptgpu_closest_hit, whose only check behind its launch is hipGetLastError, used to report such a failure as its own
    ("invalid device ordinal" from a call that names no ordinal)."""
    import ctypes
    scene, cam, p, g = built("sphere")
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "the HIP runtime is loaded"
    hip = ctypes.CDLL(paths[0])  # (loaded already: the same runtime, not a second one)
    rs = np.random.RandomState(2)
    o, d = rs.uniform(-3.0, 3.0, (64, 3)) + (0.0, 3.0, 6.0), rs.standard_normal((64, 3)) - (0.0, 0.4, 1.0)
    want = g.closest_hit(o, d)
    assert (want[2] >= 0).any()
    assert hip.hipSetDevice(1 << 20) != 0
    got = g.closest_hit(o, d)
    assert all((a.view(np.int64 if a.dtype == np.float64 else np.int32) == b.view(np.int64 if b.dtype == np.float64 else np.int32)).all()
               for a, b in zip(got, want))
    assert hip.hipSetDevice(1 << 20) != 0
    small = make_params(16, 9, 1, 1, seed=3)
    assert (g.render_batch(cam, small) == g.render_batch(cam, small)).all()


def test_bench_two_ranks_equal_one_rank(tmp_path):
    """bench.py's N>1 path on the real GPU: two ranks (gloo stands in for RCCL, both on device 0)
    shard the tiles and reduce; the reduced f32 frame equals the single-rank frame bit for bit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--scene", "cornell", "--steps", "1", "--warmup", "0", "--spp", "4", "--width", "320", "--height", "180",
              "--no-cpu-baseline", "--no-live-pmc", "--fixed-samples"]
    one = str(tmp_path / "one.npy")
    two = str(tmp_path / "two.npy")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--dump-frame", one,
                        "--dump-outputs", str(tmp_path / "out1")] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["steps"] == 1
    # NO launcher: `python bench.py --gpus 2` starts its own two ranks (the driver's form of the call)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["RPT_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dump-frame", two,
                        "--dump-outputs", str(tmp_path / "out2")] + common, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines  # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["value"] > 0
    assert "bench.py itself" in out["config"]["launched_by"]
    assert out["exchange"]["ranks"] == 2 and out["exchange"]["library_exchange_ran"] is False  # gloo stand-in: said so
    # the N > 1 line reads on its own: the ranks' render times as max / min, and the committed 1-GPU line of the same
    # workload when there is one (none for this test's frame size)
    assert out["rank_render_ms"]["max"] >= out["rank_render_ms"]["min"] >= 0 and len(out["per_rank"]) == 2  # (0 under the gloo stand-in: the library's own exchange did not run)
    assert "n1_reference" in out and out["n1_reference"] is None
    a, b = np.load(one), np.load(two)
    assert a.shape == b.shape == (320 * 180 * 3,) and (a == b).all() and a.max() > 0
    for d in ("out1", "out2"):  # --dump-outputs: the same last frame, shaped (H, W, 3)
        assert os.listdir(str(tmp_path / d)) == ["cornell.npy"]
        c = np.load(str(tmp_path / d / "cornell.npy"))
        assert c.shape == (180, 320, 3) and c.dtype == np.float32 and (c.reshape(-1) == a).all()


def test_bench_plain_run_dumps_what_full_dumps(tmp_path):
    """bench.py without --full times the headline and nothing else: no roofline, CPU baseline or other configs on its
    line.  With --dump-outputs it still writes the other configs' frames, each rendered once with the parameters of the
    last step --full times; they equal the frames of --full's timed steps bit for bit.  The default run's other configs
    are cut to two cheap ones here: the C3 mesh (wavefront pipeline) and the glass spheres (persistent)."""
    import json
    import subprocess
    import sys
    bench = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
    run = ("import importlib.util; spec = importlib.util.spec_from_file_location('bench_mod', %r); "
           "b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b); "
           "b.OTHER_CONFIGS = (('dragon', 4), ('glass', 2)); b.main()" % bench)
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--spp", "4", "--width", "320", "--height", "180"]
    lines = {}
    for form, extra in (("plain", []), ("full", ["--full", "--no-live-pmc", "--no-cpu-baseline"])):
        r = subprocess.run([sys.executable, "-c", run] + common + extra + ["--dump-outputs", str(tmp_path / form)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[form] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    assert not {"roofline", "cpu_baseline", "other_configs", "c3_msamples"} & set(plain)
    assert plain["value"] > 0 and plain["config"]["pipeline"] == "auto -> persistent"
    assert {"roofline", "other_configs", "c3_msamples", "c5_glass_spheres_msamples"} <= set(full) and full["cpu_baseline"] is None
    assert [o["workload"].split(" ")[0] for o in full["other_configs"]] == ["dragon", "glass"]
    assert all(o.get("value", 0) > 0 for o in full["other_configs"])
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k]
    names = sorted(os.listdir(str(tmp_path / "full")))
    assert names == sorted(os.listdir(str(tmp_path / "plain"))) == ["cornell.npy", "dragon.npy", "glass.npy"]
    for n in names:
        a, b = np.load(str(tmp_path / "plain" / n)), np.load(str(tmp_path / "full" / n))
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32 and (a == b).all() and a.max() > 0, n


@pytest.mark.parametrize("failing_rank", ["1", "all"])
def test_bench_two_ranks_fall_back_when_the_library_collective_is_unavailable(tmp_path, failing_rank):
    """The set-up of the library's RCCL collective in bench.py, exercised without eight GPUs: two ranks (gloo stand-in,
    both on device 0) are told to try the library collective (RPT_BENCH_FORCE_LIB_COLLECTIVE), and one rank — or every
    rank — finds RCCL unavailable (RPTGPU_FAIL_COMM through RPT_BENCH_FAIL_COMM_RANK).  The ranks must agree on that
    BEFORE anyone enters ncclCommInitRank (a rank that cannot would leave the others blocked in the rendezvous), say
    why on the line they print, reduce through torch.distributed instead, and produce the single-rank frame."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--scene", "cornell", "--steps", "1", "--warmup", "0", "--spp", "4", "--width", "320", "--height", "180",
              "--no-cpu-baseline", "--no-live-pmc", "--fixed-samples"]
    one, two = str(tmp_path / "one.npy"), str(tmp_path / "two.npy")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--dump-frame", one] + common,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, RPT_BENCH_BACKEND="gloo", RPT_BENCH_FORCE_LIB_COLLECTIVE="1")
    if failing_rank == "all":
        env["RPTGPU_FAIL_COMM"] = "1"
    else:
        env["RPT_BENCH_FAIL_COMM_RANK"] = failing_rank
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", os.path.join(root, "bench.py"),
                        "--gpus", "2", "--dump-frame", two] + common, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and "could not be set up" in out["config"]["collective"], out["config"]["collective"]
    assert "RPTGPU_FAIL_COMM" in out["config"]["collective"]
    a, b = np.load(one), np.load(two)
    assert (a == b).all() and a.max() > 0


def test_edge_cases_match_the_oracle(oracle):
    """Small / degenerate configurations, every one compared bit for bit with the oracle."""
    cases = []
    s, c, _ = scenes.cornell()
    cases += [(s, c, make_params(1, 1, 3, 5, seed=1)), (s, c, make_params(7, 3, 0, 1, seed=2)),   # 1x1 frame; B = 0, 1 spp
              (s, c, make_params(33, 17, 40, 2, seed=3)),                                           # B larger than any path
              (s, c, make_params(16, 9, 2, 3, seed=4, tile=(4, 4), part=(5, 64))),                # a part that owns few tiles
              (s, c, make_params(16, 9, 2, 3, seed=4, tile=(64, 64), part=(1, 2))),               # a part that owns nothing
              (s, c, make_params(24, 8, 2, 2, seed=2 ** 63 + 5, sample_index_base=2 ** 40 + 3)),   # 64-bit seed / sample index
              (s, c, make_params(12, 8, 2, 5, seed=7, sample_index_base=2 ** 32 - 2))]              # the batch crosses 2^32 samples
    only_lights = rpt_amd.Scene()
    only_lights.add(rpt_amd.Light.Point((1, 1, 1), (0, 1, 0)))
    only_lights.add(rpt_amd.Light.Ambient((0.5, 0.5, 0.5)))
    cases.append((only_lights, rpt_amd.Camera(), make_params(8, 8, 2, 2)))
    # HDRI looked at along the poles and the seam (environment.rs:25-52 reads x0+1 / y0+1 unguarded)
    env = rpt_amd.Scene()
    env.environment = rpt_amd.Environment.Hdri(scenes.synthetic_hdri(32, 16, seed=3))
    for d in ((0, 1, 0), (0, -1, 0), (-1, 0, 0), (-1, 0, 1e-17), (1, 0, 0)):
        up = (0, 0, 1) if d[0] == 0 else (0, 1, 0)
        cases.append((env, rpt_amd.Camera(eye=(0, 0, 0), direction=d, up=up, fov=1e-3), make_params(5, 5, 1, 2, seed=6)))
    # geometry exactly on coordinate planes, negative zero bounds, a ray direction with zero components
    flat = rpt_amd.Scene()
    flat.add(rpt_amd.Object(rpt_amd.polygon([(-1, -0.0, -1), (-1, -0.0, 1), (1, -0.0, 1), (1, -0.0, -1)]))
             .material(rpt_amd.Material.diffuse((0.5, 0.5, 0.5))))
    flat.add(rpt_amd.Object(rpt_amd.Mesh(scenes.knot_mesh(64, 12))).material(rpt_amd.Material.specular((0.7, 0.8, 0.3), 0.2)))
    flat.add(rpt_amd.Light.Directional((1, 1, 1), (0, -1, 0)))   # shadow rays along +y: two zero components
    flat.add(rpt_amd.Light.Point((3, 3, 3), (0, 2, 0)))
    cases.append((flat, rpt_amd.Camera(eye=(0, 3, 0), direction=(0, -1, 0), up=(0, 0, 1), fov=0.8), make_params(24, 24, 3, 3, seed=8)))
    for scene, cam, p in cases:
        g = GpuScene(scene, 0)
        ref = oracle.OracleScene(scene).render(cam, p, threads=0)
        for flags in (_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT, 0):
            pp = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, p.sample_index_base,
                             (p.tile_width, p.tile_height), (p.part_index, p.part_count), flags=flags)
            img = g.render_batch(cam, pp)
            same = (img == ref) | (np.isnan(img) & np.isnan(ref))
            assert same.all(), (p.width, p.height, p.max_bounces, flags, np.abs(img - ref).max())
        g.close()


def _polygon_room(n_walls, transformed_every=0, sides=(4, 5, 6, 8), seed=3):
    scene, cam, _ = scenes.polygon_room(n_walls, transformed_every, sides, seed)
    return scene, cam


import math  # noqa: E402


@pytest.mark.parametrize("n_walls,transformed_every", [(5, 0), (9, 0), (14, 4), (23, 0), (40, 5), (160, 7)])
def test_flat_scenes_batched_leaf_tests_match_the_oracle(oracle, n_walls, transformed_every):
    # runs of 5 (one batch), 9 and 14 (split at FLAT_RUN = 6 / at Transformed meshes / at cubes and spheres),
    # polygons of 2..6 triangles (leaf loops of different lengths inside one wave), and scenes whose tables
    # do or do not fit a wave's LDS share (160 walls: the general kernel takes over) — all bit-equal to the oracle
    scene, cam = _polygon_room(n_walls, transformed_every)
    p = make_params(48, 32, 4, 3, seed=1000 + n_walls)
    g = GpuScene(scene, 0)
    ref = oracle.OracleScene(scene).render(cam, p, threads=0)
    for flags in (0, _abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_GENERAL_TRAVERSAL, _abi.RPT_FLAG_WAVEFRONT):
        pp = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=flags)
        img = g.render_batch(cam, pp)
        assert (img == ref).all(), (n_walls, flags, np.abs(img - ref).max())
    # scenes of 8..64 objects run the flat kernel behind the object filter (paths_flat.inc flat_query_filtered); the same
    # scene without it (the batched runs alone), and with it from the first object on
    for min_objects in ("0", "1"):
        os.environ["RPTGPU_OBJECT_FILTER_MIN"] = min_objects
        try:
            g2 = GpuScene(scene, 0)
        finally:
            del os.environ["RPTGPU_OBJECT_FILTER_MIN"]
        img = g2.render_batch(cam, p)
        g2.close()
        assert (img == ref).all(), (n_walls, "RPTGPU_OBJECT_FILTER_MIN=" + min_objects, np.abs(img - ref).max())
    # closest hits and random secondary rays through rptgpu_closest_hit as well
    rs = np.random.RandomState(n_walls)
    o = rs.uniform(-2.5, 2.5, (4000, 3))
    d = rs.randn(4000, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t0, n0, ob0 = oracle.OracleScene(scene).closest_hit(o, d)
    t1, n1, ob1 = g.closest_hit(o, d)
    assert (t0 == t1).all() and (ob0 == ob1).all() and (n0.view(np.int64) == n1.view(np.int64)).all()
    g.close()


def test_object_filter_far_cameras_axis_parallel_rays_and_unfilterable_objects(oracle):
    # the object filter (host_scene.cpp fill_object_boxes, paths_flat.inc flat_query_filtered) where its f32 arithmetic and
    # its exemptions are stressed: an unbounded Plane among the objects, a sphere a thousand times smaller than the
    # scene, a placement with condition number 1e5 (exempt), a mesh with a sliver (exempt), objects in the corners of
    # the grid, a directional light along an axis (shadow rays with two zero components), cameras inside an object's
    # box, far outside the grid (1e3 and 1e7 scene sizes away: the latter switches the filter off per ray) and looking
    # exactly along an axis
    rs = np.random.RandomState(11)
    S = rpt_amd.Scene()
    S.add(rpt_amd.Object(rpt_amd.plane((0.0, 1.0, 0.0), -1.0)).material(rpt_amd.Material.diffuse((0.6, 0.6, 0.6))))
    for i in range(10):
        c = rs.uniform(-2.0, 2.0, 3)
        a = rs.randn(3); a /= np.linalg.norm(a)
        b = np.cross(a, rs.randn(3)); b /= np.linalg.norm(b)
        k = (3, 4, 5, 7)[i % 4]
        verts = [tuple(c + 0.8 * (math.cos(t) * a + math.sin(t) * b)) for t in np.linspace(0, 2 * math.pi, k, endpoint=False)]
        shape = rpt_amd.polygon(verts)
        if i % 3 == 2:
            shape = shape.rotate_y(0.4 * i).translate((0.1, 0.0, -0.1))
        S.add(rpt_amd.Object(shape).material(rpt_amd.Material.diffuse(tuple(rs.uniform(0.3, 0.9, 3)))))
    S.add(rpt_amd.Object(rpt_amd.sphere().scale((2e-3, 2e-3, 2e-3)).translate((0.2, 0.3, 1.0))).material(rpt_amd.Material.specular((0.9, 0.2, 0.2), 0.3)))
    S.add(rpt_amd.Object(rpt_amd.sphere().scale((1.0, 1e-5, 1.0)).translate((-1.0, 0.5, 0.0))).material(rpt_amd.Material.diffuse((0.2, 0.9, 0.2))))
    S.add(rpt_amd.Object(rpt_amd.cube().rotate_y(0.7).scale((0.5, 1.5, 0.5)).translate((2.5, 0.0, -2.5))).material(rpt_amd.Material.clear(1.5, 0.05)))
    S.add(rpt_amd.Object(rpt_amd.cube().translate((-3.0, -0.5, 3.0))))                      # a corner of the grid, axis-aligned
    S.add(rpt_amd.Object(rpt_amd.sphere().translate((3.0, 2.0, 3.0))).material(rpt_amd.Material.metallic_((0.9, 0.9, 0.9), 0.1)))
    S.add(rpt_amd.Object(rpt_amd.polygon([(0.0, 1.5, 0.0), (0.0, 1.5, 0.0), (1.0, 1.5, 0.0), (1.0, 1.5000000001, 1e-9)])))  # sliver
    S.add(rpt_amd.Light.Directional((0.4, 0.4, 0.4), (0.0, -1.0, 0.0)))
    S.add(rpt_amd.Light.Point((30.0, 30.0, 30.0), (0.5, 3.0, 0.5)))
    S.add(rpt_amd.Light.Object(rpt_amd.Object(rpt_amd.sphere().scale((0.2, 0.2, 0.2)).translate((0.0, 2.5, 0.0)))
                               .material(rpt_amd.Material.light((1.0, 1.0, 1.0), 40.0))))
    cams = [rpt_amd.Camera.look_at((0.0, 0.8, 6.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 0.9),
            rpt_amd.Camera.look_at((-3.0, -0.4, 3.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 1.2),           # inside the corner cube
            rpt_amd.Camera.look_at((0.0, 2.0e3, 6.0e3), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 0.0012),
            rpt_amd.Camera.look_at((0.0, 0.0, 6.0e7), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 1.2e-7),
            rpt_amd.Camera(eye=(0.2, 0.3, 5.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=0.5)]
    g = GpuScene(S, 0)
    osc = oracle.OracleScene(S)
    for ci, cam in enumerate(cams):
        p = make_params(48, 32, 4, 3, seed=500 + ci)
        ref = osc.render(cam, p, threads=0)
        img = g.render_batch(cam, p)
        same = (img == ref) | (np.isnan(img) & np.isnan(ref))
        assert same.all(), (ci, np.abs(img - ref).max())
        assert (ref != 0).any()
    g.close()


def test_flat_scenes_exact_ties_and_coplanar_surfaces(oracle):
    # adversarial for the batched leaf tests: the same quad twice (exact ties: the first object must win), a cube
    # standing on a coplanar floor quad, quads that share edges and corners, a quad inside another quad's plane,
    # a Transformed copy of an untransformed quad (same place, different arithmetic), zero-area and sliver triangles
    S = rpt_amd.Scene()
    floor = [(-2.0, 0.0, -2.0), (-2.0, 0.0, 2.0), (2.0, 0.0, 2.0), (2.0, 0.0, -2.0)]
    S.add(rpt_amd.Object(rpt_amd.polygon(floor)).material(rpt_amd.Material.diffuse((0.7, 0.7, 0.7))))
    S.add(rpt_amd.Object(rpt_amd.polygon(floor)).material(rpt_amd.Material.diffuse((0.9, 0.1, 0.1))))        # duplicate
    S.add(rpt_amd.Object(rpt_amd.polygon([(-1.0, 0.0, -1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, -1.0)]))
          .material(rpt_amd.Material.specular((0.1, 0.9, 0.1), 0.3)))                                          # coplanar inset
    S.add(rpt_amd.Object(rpt_amd.polygon([(-2.0, 0.0, -2.0), (-2.0, 2.0, -2.0), (2.0, 2.0, -2.0), (2.0, 0.0, -2.0)]))
          .material(rpt_amd.Material.diffuse((0.2, 0.2, 0.9))))                                                # shares an edge
    S.add(rpt_amd.Object(rpt_amd.polygon([(-2.0, 0.0, -2.0), (-2.0, 0.0, 2.0), (-2.0, 2.0, 2.0), (-2.0, 2.0, -2.0)]))
          .material(rpt_amd.Material.diffuse((0.9, 0.9, 0.2))))                                                # shares a corner
    S.add(rpt_amd.Object(rpt_amd.polygon([(0.0, 0.5, 0.0), (0.0, 0.5, 0.0), (1.0, 0.5, 0.0), (1.0, 0.5000000001, 1e-9)]))
          .material(rpt_amd.Material.diffuse((0.5, 0.5, 0.5))))                                                # degenerate + sliver
    S.add(rpt_amd.Object(rpt_amd.cube().translate((0.5, 0.5, 0.5))).material(rpt_amd.Material.clear(1.5, 0.05)))  # on the floor
    S.add(rpt_amd.Object(rpt_amd.polygon(floor).translate((0.0, 0.0, 0.0))).material(rpt_amd.Material.diffuse((0.3, 0.8, 0.8))))
    S.add(rpt_amd.Object(rpt_amd.polygon(floor).rotate_y(math.pi / 2)).material(rpt_amd.Material.diffuse((0.8, 0.3, 0.8))))
    S.add(rpt_amd.Light.Object(rpt_amd.Object(rpt_amd.polygon([(-0.5, 1.9, -0.5), (-0.5, 1.9, 0.5), (0.5, 1.9, 0.5), (0.5, 1.9, -0.5)]))
                               .material(rpt_amd.Material.light((1.0, 1.0, 1.0), 20.0))))
    S.add(rpt_amd.Light.Directional((0.3, 0.3, 0.3), (0.0, -1.0, 0.0)))                                        # axis-parallel shadow rays
    cam = rpt_amd.Camera.look_at((0.3, 1.2, 3.5), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 0.9)
    g = GpuScene(S, 0)
    osc = oracle.OracleScene(S)
    p = make_params(64, 40, 5, 4, seed=77)
    ref = osc.render(cam, p, threads=0)
    for flags in (0, _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_GENERAL_TRAVERSAL, _abi.RPT_FLAG_WAVEFRONT):
        img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=flags))
        same = (img == ref) | (np.isnan(img) & np.isnan(ref))
        assert same.all(), (flags, np.abs(img - ref).max())
    # rays aimed exactly at shared edges / corners / along the planes
    rs = np.random.RandomState(2)
    tgt = np.array([(-2.0, 0.0, -2.0), (-2.0, 1.0, -2.0), (0.0, 0.0, -2.0), (1.0, 0.0, 1.0), (0.0, 0.0, 0.0), (0.5, 0.0, 0.5),
                    (1.0, 0.5, 0.0), (0.0, 1.0, 0.0)])
    o = rs.uniform(-1.5, 1.5, (len(tgt) * 200, 3)) + np.array([0.0, 1.6, 0.0])
    d = np.repeat(tgt, 200, axis=0) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o2 = np.array([[0.0, 1e-9, 0.0], [0.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [0.25, 1.0, 0.25]])
    d2 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    t0, n0, ob0 = osc.closest_hit(o, d)
    t1, n1, ob1 = g.closest_hit(o, d)
    same_t = (t0.view(np.int64) == t1.view(np.int64)) | (np.isnan(t0) & np.isnan(t1))
    assert same_t.all() and (ob0 == ob1).all()
    assert ((n0.view(np.int64) == n1.view(np.int64)) | (np.isnan(n0) & np.isnan(n1))).all()
    assert (ob0 == 0).sum() > 0 and (ob0 == 1).sum() == 0   # the duplicate never wins a tie against the first
    g.close()


def test_library_collective_single_rank_communicator(built):
    """rptgpu_comm_* / rptgpu_render_batch_reduce: a real RCCL communicator of one rank (all this box has) —
    the reduce runs through ncclReduce on the library's stream and the frame equals render_batch rounded to f32.
    Without a communicator the same call is a plain render + D2H."""
    scene, cam, p, g = built("cornell")
    ref = g.render_batch(cam, p).astype(np.float32).ravel()
    plain = g.render_batch_reduce(cam, p, root=0)
    assert (plain == ref).all()
    g2 = GpuScene(scene, 0)
    g2.comm_init(0, 1, GpuScene.comm_unique_id())
    with pytest.raises(rpt_amd.RptGpuError):
        g2.comm_init(0, 1, GpuScene.comm_unique_id())  # one communicator per handle
    a = g2.render_batch_reduce(cam, p, root=0)
    # the partition fields of the caller are overridden by (rank, world)
    pp = make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, tile=(4, 4), part=(1, 3))
    b = g2.render_batch_reduce(cam, pp, root=0)
    assert (a == ref).all() and (b == ref).all()
    with pytest.raises(rpt_amd.RptGpuError):
        g2.render_batch_reduce(cam, p, root=1)
    g2.comm_destroy()
    assert (g2.render_batch_reduce(cam, p, root=0) == ref).all()
    g2.close()


def test_gather_and_reduce_give_the_frame_of_a_plain_render(built, monkeypatch):
    """The batch's collective is a gather of the pixels each rank owns (default) or an ncclReduce of zero-filled frames
    (RPTGPU_COLLECTIVE=reduce): with a 1-rank communicator both must return the plain render; RptStats splits the
    batch's time.  The gather of N ranks minus the wire (every rank's packed pixels placed by the root's lists) is
    replayed on this one GPU for N = 1, 2, 3, 8 and more ranks than tiles, on a frame whose edge tiles are ragged."""
    scene, cam, p, g = built("cornell")
    pr = make_params(75, 41, p.max_bounces, 3, p.exposure_value, p.seed)
    ref = g.render_batch(cam, pr).astype(np.float32).ravel()
    for mode in ("gather", "reduce", "param_gather", "param_reduce"):
        # the exchange's kind through the environment (the override) and through RptRenderParams::collective (ABI v6)
        pm = pr
        if mode.startswith("param_"):
            monkeypatch.delenv("RPTGPU_COLLECTIVE", raising=False)
            pm = make_params(75, 41, p.max_bounces, 3, p.exposure_value, p.seed,
                             collective=_abi.RPT_COLLECTIVE_REDUCE if mode.endswith("reduce") else _abi.RPT_COLLECTIVE_GATHER)
        else:
            monkeypatch.setenv("RPTGPU_COLLECTIVE", mode)
        g2 = GpuScene(scene, 0)
        g2.comm_init(0, 1, GpuScene.comm_unique_id())
        g2.reset_stats()
        assert (g2.render_batch_reduce(cam, pm, root=0) == ref).all(), mode
        assert (g2.render_batch_reduce(cam, pm, root=0) == ref).all(), mode
        st = g2.stats()
        assert st.reduce_calls == 2 and st.reduce_render_ms > 0.0 and st.reduce_collective_ms >= 0.0 and st.reduce_copy_ms > 0.0
        g2.close()
    monkeypatch.delenv("RPTGPU_COLLECTIVE", raising=False)
    bad = make_params(75, 41, p.max_bounces, 3, p.exposure_value, p.seed, collective=7)
    with pytest.raises(rpt_amd.RptGpuError):
        g.render_batch_reduce(cam, bad, root=0)
    for world in (1, 2, 3, 8, 64):
        assert (g.render_batch_emulate_ranks(cam, pr, world) == ref).all(), world
    with pytest.raises(rpt_amd.RptGpuError):
        g.render_batch_emulate_ranks(cam, pr, 0)


def test_scene_destroy_releases_device_memory():
    # every device allocation behind a handle (scene, workspace, per-sample radiance buffer, sort buffers) is
    # returned by rptgpu_scene_destroy: create / render / destroy in a loop keeps free HBM where it was
    import torch
    scene, cam, _ = scenes.cornell()
    mesh_scene, mesh_cam, _ = scenes.dragon(nu=96, nv=16)

    def cycle(monkey_env=None):
        for sc, cm, flags in ((scene, cam, _abi.RPT_FLAG_PERSISTENT), (mesh_scene, mesh_cam, _abi.RPT_FLAG_WAVEFRONT)):
            g = GpuScene(sc, 0)
            g.render_batch(cm, make_params(512, 288, 4, 16, seed=1, flags=flags))  # 56 MB of per-sample radiance
            g.close()

    os.environ["RPTGPU_DEEP_DEPTH"] = "1"
    os.environ["RPTGPU_SORT_RAYS"] = "1"
    try:
        cycle()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        for _ in range(6):
            cycle()
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info(0)[0]
    finally:
        del os.environ["RPTGPU_DEEP_DEPTH"], os.environ["RPTGPU_SORT_RAYS"]
    assert free0 - free1 < (32 << 20), "leaked %.1f MB over 6 create/render/destroy cycles" % ((free0 - free1) / 2 ** 20)


def test_material_that_would_panic_gen_bool_is_rejected():
    # sample_f hands f = mix(lerp(f0, mean(color), metallic), 1, 0.2) to rng.gen_bool, which panics outside [0, 1]
    # (material.rs:233-235, 264); the device cannot panic, so scene_create refuses such a material
    for mat in (rpt_amd.Material.metallic_((3.0, 3.0, 3.0), 0.1), rpt_amd.Material.metallic_((float("nan"), 0.5, 0.5), 0.1)):
        s = rpt_amd.Scene()
        s.add(rpt_amd.Object(rpt_amd.sphere()).material(mat))
        with pytest.raises(rpt_amd.RptGpuError) as e:
            GpuScene(s, 0)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT


def test_degenerate_shell_mesh_builds_and_renders(oracle):
    # a chain of nested shells of tiny triangles (round 1 feared a tree deeper than the device stack here and refused
    # it; no depth is refused any more): whatever tree the build rule makes of it renders like the oracle's
    tris = []
    for i in range(40 * 16):
        r = 1.0 + i // 16
        tris.append(rpt_amd.Triangle.from_vertices((r, 0, 0), (r, 1e-3 * (i % 16 + 1), 0), (r, 0, 1e-3)))
    scene = rpt_amd.Scene()
    scene.add(rpt_amd.Object(rpt_amd.Mesh(tris)))
    scene.add(rpt_amd.Light.Point((5.0, 5.0, 5.0), (0.0, 2.0, 2.0)))
    cam = rpt_amd.Camera.look_at((20.0, 0.0, 6.0), (20.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.2)
    p = make_params(48, 16, 2, 2, seed=5)
    g = GpuScene(scene, 0)
    assert (g.render_batch(cam, p) == oracle.OracleScene(scene).render(cam, p, threads=0)).all()
    g.close()


def test_device_buffer_equals_host_buffer(oracle):
    """rptgpu_buffer_* (SURVEY §8f rank 1): image() and variance() of the device-resident Buffer equal
    the host Buffer fed with the same batches — and the oracle's Buffer restatement — exactly."""
    scene, cam, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    W, H = 80, 45
    for radius in (0, 1, 2):
        dev = rpt_amd.DeviceBuffer(g, W, H, rpt_amd.Filter.Box(radius))
        host = rpt_amd.Buffer(W, H, rpt_amd.Filter.Box(radius))
        batches = []
        for i in range(4):
            p = make_params(W, H, 3, 2, seed=12, sample_index_base=2 * i, exposure_value=1.0)
            dev.sample(cam, p)
            b = g.render_batch(cam, p)
            host.add_samples(b)
            batches.append(b)
        assert dev.num_batches() == 4
        img = dev.image()
        assert (img == host.image()).all()
        assert (img == oracle.buffer_image(W, H, radius, batches)).all()
        assert img.max() == 255 and img.min() < 40  # exposure +1 saturates the lit wall, corners stay dark
        assert dev.variance() == oracle.buffer_variance(W, H, batches)
        assert abs(dev.variance() - host.variance()) <= 1e-15 * abs(host.variance())
        dev.close()
    with pytest.raises(rpt_amd.RptGpuError):  # "Invalid sample dimension" (buffer.rs:33-36)
        dev = rpt_amd.DeviceBuffer(g, W, H)
        dev.sample(cam, make_params(W + 1, H, 1, 1))
    with pytest.raises(rpt_amd.RptGpuError):  # "Pixel found with no samples" (buffer.rs:89)
        rpt_amd.DeviceBuffer(g, W, H).image()
    # iterative_render(on_device=True) == iterative_render on the host
    r = rpt_amd.Renderer(scene, cam).width(W).height(H).max_bounces(2).num_samples(6).seed(3).filter(rpt_amd.Filter.Box(1))
    a, bimgs = [], []
    r.iterative_render(2, lambda it, buf: a.append((it, buf.variance(), buf.image())))
    r.iterative_render(2, lambda it, buf: bimgs.append((it, buf.variance(), buf.image())), on_device=True)
    assert [x[0] for x in a] == [x[0] for x in bimgs] == [2, 4, 6]
    for x, y in zip(a, bimgs):
        assert (x[2] == y[2]).all()
        assert (np.isnan(x[1]) and np.isnan(y[1])) or abs(x[1] - y[1]) <= 1e-15 * abs(x[1])
    g.close()
