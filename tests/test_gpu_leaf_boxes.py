"""The DEVICE's leaf-box filter (kernels/shapes.inc boxray_make / box_window / leaf_box_pass / kd_leaf_boxed and the
group branch of kd_leaf; the nested walker's own copy in kernels/tree_trace.inc) against the oracle, which has no filter,
on the rays of tests/leaf_box_rays.py: aimed at vertices and edges, grazing spheres, nearly and exactly axis-parallel,
from up to 1e16 extents away, and through stacks of triangles that share one leaf of up to 110 entries.  The filter's one
obligation is that an entry it rejects is an entry the exact test rejects, so every hit record is the oracle's, bit for
bit, through every route that hosts a call site — and once more with the filter off, which tells a filter bug from any
other.  Shadow rays, whose window ends at the light, go through render_batch with the light ON the mesh."""
import numpy as np
import pytest

from rpt_amd import Camera, GpuScene, _abi, make_params

import leaf_box_rays as R

pytestmark = pytest.mark.gpu

ROUTES = {  # as test_axis_parallel_rays_and_origins_on_split_planes selects them
    "default": {},
    "in_kernel": {"RPTGPU_RAYS_IN_KERNEL": "1"},
    "per_tree": {"RPTGPU_DEEP_DEPTH": "1", "RPTGPU_SORT_RAYS": "1", "RPTGPU_SORT_MIN_RAYS": "0"},
    "per_tree_unsorted": {"RPTGPU_DEEP_DEPTH": "1", "RPTGPU_SORT_RAYS": "0", "RPTGPU_SORT_MIN_RAYS": "0"},
}
GROUP_FAR_BANDS = ((-1.0, 1.0), (1.0, 2.18), (2.18, 3.5), (3.5, 4.5))   # 1e7 steps of the group's grid are ~152 extents
_reference = {}


def reference(oracle, scene, pop):
    """the oracle's hit records of a (scene, population) pair: computed once, read-only"""
    key = (scene, pop)
    if key not in _reference:
        o, d, _ = R.population(scene, pop)
        t, n, ob = oracle.OracleScene(R.build(scene).scene).closest_hit(o, d)
        for a in (t, n, ob):
            a.setflags(write=False)
        _reference[key] = (t, n, ob)
    return _reference[key]


def bands_of(scene, pop):
    if pop != "far":
        return None
    return GROUP_FAR_BANDS if scene == "group" else R.FAR_BANDS


def differing(ref, got):
    """rays whose record is not the oracle's bits (a NaN equals a NaN, as in test_gpu_parity.py)"""
    (t0, n0, ob0), (t1, n1, ob1) = ref, got
    same_t = (t0.view(np.int64) == t1.view(np.int64)) | (np.isnan(t0) & np.isnan(t1))
    same_n = ((n0.view(np.int64) == n1.view(np.int64)) | (np.isnan(n0) & np.isnan(n1))).all(axis=1)
    return ~(same_t & same_n & (ob0 == ob1))


# ---- conditions on the inputs: checked on the oracle's answers, whatever the device does ---------------------------------
@pytest.mark.parametrize("scene,pop", R.PAIRS)
def test_population_hits_its_scene(oracle, scene, pop):
    t, n, ob = reference(oracle, scene, pop)
    _, _, tag = R.population(scene, pop)
    hit = ob == 1                                               # object 0 is the floor
    print("%s/%s: %d rays, %.3f hit the mesh or group" % (scene, pop, len(t), hit.mean()))
    assert hit.mean() >= 0.2, hit.mean()
    for a, b in bands_of(scene, pop) or ():
        sel = (tag >= a) & (tag < b)
        print("   10^%g - 10^%g extents: %d rays, %.3f hit" % (a, b, sel.sum(), hit[sel].mean()))
        assert sel.sum() > 1000 and hit[sel].mean() >= 0.05, (a, b, hit[sel].mean())


def test_bundles_tree_has_leaves_of_every_size_class_and_winners_in_every_position(oracle):
    b = R.build("bundles")
    tree = R.mesh_tree(b.rows)
    counts = R.leaf_class_counts(tree)
    print("leaves with 3-8 / 9-16 / 17-32 / 33-64 / >64 entries:", counts)
    assert min(counts) >= 1, counts
    o, d, _ = R.population("bundles", "through")
    t, n, ob = reference(oracle, "bundles", "through")
    pos = R.winner_positions(b, tree, o, d, t, n)
    won = [int(((pos >= lo) & (pos <= hi)).sum()) for lo, hi in R.POSITION_CLASSES]
    print("first hits at leaf positions 0-7 / 8-31 / 32-63 / >=64:", won)
    assert min(won) >= 100, won


def test_group_children_straddle_the_quadric_threshold():
    g = R.build("group")
    print("spheres below / at or above 64 grid steps:", int(g.small.sum()), int((~g.small).sum()), "cubes:", len(g.cubes))
    assert g.small.sum() >= 20 and (~g.small).sum() >= 20 and len(g.cubes) >= 20


# ---- closest hits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("scene,pop", R.PAIRS)
def test_closest_hits_are_the_unfiltered_oracles(oracle, scene, pop, route, monkeypatch):
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    b = R.build(scene)
    o, d, tag = R.population(scene, pop)
    ref = reference(oracle, scene, pop)
    bad = {}
    for filtered in (True, False):                              # the control: the same rays with leaf_boxes = 0
        g = GpuScene(b.scene, 0) if filtered else GpuScene(b.scene, 0, leaf_boxes=0)
        assert g.options()["leaf_boxes"] == (1 if filtered else 0)
        bad[filtered] = differing(ref, g.closest_hit(o, d))
        g.close()
    bands = bands_of(scene, pop)
    per_band = [] if bands is None else [(a, c, int(bad[True][(tag >= a) & (tag < c)].sum())) for a, c in bands]
    if bad[False].any():
        verdict = "NOT the filter's: %d rays differ with leaf_boxes=0 too" % bad[False].sum()
    else:
        verdict = "the FILTER's: none differ with leaf_boxes=0"
    assert not bad[True].any() and not bad[False].any(), (
        "%s/%s via %s: %d of %d rays differ from the oracle (%s); per far band %s; first rays %s"
        % (scene, pop, route, bad[True].sum(), len(o), verdict, per_band, np.flatnonzero(bad[True] | bad[False])[:5]))


# ---- shadow windows ------------------------------------------------------------------------------------------------------
KNOT_ISLAND = 99   # a triangle of the knot's underside; its neighbours are cut away (leaf_box_rays.knot) so that a light just
#                    inside the tube lights something too
ON_TRIANGLE = ("vertex", "edge_midpoint", "centroid")


def _shadow_case(name, case):
    """-> (scene with one Point light ON the mesh, camera).  The shadow ray of a surface point then ends where it hits the
    light's own triangle, and `closest > dist_to_light` (renderer.rs:197) makes a hit at exactly the window's end occlude:
    box_window(..., fmin(rt, t_stop)) must let that triangle through."""
    if name == "knot":
        tri = R.knot_rows()[KNOT_ISLAND, :9].reshape(3, 3)
        back, aside = 0.6, np.array([0.05, 0.03, 0.02])
    else:
        b = R.build("bundles")
        first = b.n_knot + sum(R.BUNDLE_SIZES[:8])                                               # the bundle of 65
        c, nrm, e1, e2, h = b.frames[8]
        layers = b.tris[first:first + 65].reshape(65, 3, 3)
        tri = layers[np.argmin((layers.mean(axis=1) - c) @ nrm)]                                 # the stack's lowest layer
        back, aside = 1.0, np.array([0.3, 0.2, 0.1])
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    n /= np.linalg.norm(n)
    cen = tri.mean(axis=0)
    if case == "inside_stack":      # between the second and the third layer from below, near the rim of the smaller ones
        hs = np.sort(h)
        light = c + 0.5 * (hs[1] + hs[2]) * nrm + 0.2 * (np.cos(3.0) * e1 + np.sin(3.0) * e2)
    else:
        light = {"vertex": tri[0], "edge_midpoint": 0.5 * (tri[1] + tri[2]), "centroid": cen,
                 "above_centroid": cen + 1e-9 * n, "below_centroid": cen - 1e-9 * n}[case]
    built = R.knot(light=light, island=KNOT_ISLAND) if name == "knot" else R.bundles(light=light)
    return built, light, Camera.look_at(tuple(cen - back * n + aside), tuple(cen), (0.0, 1.0, 0.0), 0.9)


SHADOW_CASES = [("knot", c) for c in ON_TRIANGLE + ("above_centroid", "below_centroid")] + \
               [("bundles", c) for c in ON_TRIANGLE + ("above_centroid", "below_centroid", "inside_stack")]


@pytest.mark.parametrize("name,case", SHADOW_CASES)
def test_shadow_rays_whose_window_ends_on_the_mesh(oracle, name, case):
    b, light, cam = _shadow_case(name, case)
    p = make_params(48, 32, 2, 3, seed=900 + len(case))
    osc = oracle.OracleScene(b.scene)
    ref = osc.render(cam, p, threads=0)
    # conditions, on the oracle: first hits of the camera rays, then their shadow rays as renderer.rs:190-200 casts them
    rays = [oracle.camera_ray(cam, p, x, y, 0) for y in range(p.height) for x in range(p.width)]
    o, d = np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
    t, _, ob = osc.closest_hit(o, d)
    seen = ob >= 0
    pos = o[seen] + t[seen, None] * d[seen]
    dist = np.linalg.norm(light - pos, axis=1)
    ts, _, obs = osc.closest_hit(pos, (light - pos) / dist[:, None])
    occluded = (obs >= 0) & ~(ts > dist)
    at_end = (obs >= 0) & (np.abs(ts - dist) <= 1e-9 * dist)
    print("%s/%s: %d camera rays hit, %d lit, %d shadowed, %d shadow rays end within 1e-9 of their hit"
          % (name, case, seen.sum(), (~occluded).sum(), occluded.sum(), at_end.sum()))
    assert (~occluded).sum() >= 20 and occluded.sum() >= 20 and (ref != 0).any()
    assert at_end.sum() >= 20 or case not in ON_TRIANGLE
    g = GpuScene(b.scene, 0)
    for flags in (_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT):
        img = g.render_batch(cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=flags))
        same = (img == ref) | (np.isnan(img) & np.isnan(ref))
        assert same.all(), (name, case, flags, int((~same).any(axis=1).sum()), np.abs(img - ref).max())
    g.close()
