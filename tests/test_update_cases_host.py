"""What tests/test_gpu_update_matrix.py relies on, held true without a GPU: by the oracle, the library's host kd builder and
the scene planner (rpt_amd/csrc/scene_plan.h through tests/cpp/scene_plan_check.cpp) alone.

The floors.  Of a case's 600 rays at least 10 % hit something, at least 10 % miss everything and at least 10 % reach an
updated object before or after the step; at least 5 % of the hit distances and at least 5 % of the pixels of the 37 x 21
frame of view 0 change.  Two kinds of case cannot move a hit: lights — no answer about a ray changes, only the frame — and
materials — the distances stay, and at least 5 % of the rays' albedos change instead.  The GPU test asks the device for half
of each share measured here ("the update is seen"), so a floor that holds here with the oracle leaves it room."""
import os
import subprocess

import numpy as np
import pytest

from rpt_amd import _abi

import update_cases as C
from test_gpu_group_update import clustered as kids_clustered, coincident, jitter, tree_of as group_tree_of
from test_gpu_mesh_update import clustered, sine, tree_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH, GROUP = _abi.RPT_SHAPE_MESH, _abi.RPT_SHAPE_GROUP


def test_the_cases_are_the_ones_named():
    assert sorted(C.cases()) == sorted(C.NAMES) and len(C.NAMES) == 11
    assert C.N_RAYS == 600 and C.N_RAYS % 256 != 0 and (C.W * C.H) % 256 != 0 and C.W * C.H > 256
    for c in C.cases().values():
        o, d, max_t = C.rays(c.name)
        assert o.shape == d.shape == (C.N_RAYS, 3) and max_t.shape == (C.N_RAYS,)
        assert (abs((d * d).sum(axis=1) - 1.0) > 1e-6).all()  # no unit vectors
        assert C.points(c.name)[0].shape == (C.N_POINTS, 3)


@pytest.mark.parametrize("name", C.NAMES)
def test_the_oracle_alone_meets_the_floors(name):
    c = C.cases()[name]
    measured = C.shares(name)
    assert sorted(measured) == sorted(s.name for s in c.steps if not s.back)
    for step, m in measured.items():
        said = "%s, %s: " % (name, step) + ", ".join("%s %.1f %%" % (k, 100.0 * v) for k, v in m.items())
        assert m["hit"] >= 0.10 and m["miss"] >= 0.10, said
        assert m["frame"] >= 0.05, said
        if name == "lights":
            assert m["t"] == 0.0 and m["albedo"] == 0.0 and m["reached"] == 0.0, said
        elif not c.moves:
            assert m["t"] == 0.0 and m["reached"] >= 0.10 and m["albedo"] >= 0.05, said
        else:
            assert m["reached"] >= 0.10 and m["t"] >= 0.05, said


def test_the_trees_are_as_deep_as_the_cases_say():
    base, deep = tree_of(C.KNOT), tree_of(clustered(C.KNOT))
    assert base["max_depth"] == C.KNOT_DEPTH >= 1
    assert tree_of(sine(C.KNOT))["max_depth"] == base["max_depth"]          # mesh_same_depth
    assert tree_of(sine(C.KNOT, 4.0))["max_depth"] == base["max_depth"]     # mesh_then_objects
    assert deep["max_depth"] > base["max_depth"]                            # mesh_deeper: ws_stale, max_tree_depth, gen_levels
    assert tree_of(C.ONE_LEAF)["max_depth"] == 0
    c = C.cases()["mesh_past_fast_stacks"]
    assert c.options["fast_max_depth"] == base["max_depth"] < deep["max_depth"] and c.flags_rise
    assert "fast_max_depth" not in C.cases()["mesh_deeper"].options and not C.cases()["mesh_deeper"].flags_rise
    kids = group_tree_of(C.KIDS)
    assert group_tree_of(kids_clustered(C.KIDS))["max_depth"] > kids["max_depth"] >= 1
    assert group_tree_of(coincident(C.KIDS))["max_depth"] == 0 and group_tree_of(jitter(C.KIDS))["max_depth"] >= 1
    assert len(C.KNOT) == 1536 and len(C.KIDS) == 40
    two = tree_of(C.TWO_LEAVES)                                             # mesh_from_two_leaves: one split, a real tree
    assert two["max_depth"] == 1 and len(C.TWO_LEAVES) == len(C.KNOT) and C.cases()["mesh_from_two_leaves"].options == {"deep_depth": 1}
    kinds = [type(getattr(ob.shape, "shape", ob.shape)).__name__ for ob in C.lone_knot_scene(C.KNOT).objects]
    assert kinds == ["KdTree", "Sphere", "Plane"]  # the knot is the only tree of its scene (a Mesh is a KdTree of triangles)


def splits_across(tree, axes):
    """the most splits across one of `axes` on any path from the root to a leaf (info & 3: the axis, 3 a leaf; a: the left child)"""
    def below(node):
        axis = int(tree["info"][node]) & 3
        if axis == 3:
            return 0
        return (axis in axes) + max(below(int(tree["a"][node])), below(int(tree["a"][node]) + 1))
    return below(0)


def test_what_a_workspace_left_stale_could_show_at_these_depths():
    """swap_spare marks the workspace stale when a rebuilt tree is deeper than any before it.  What that re-sizes: the spill
    columns, whose height is max(KD_MAX_STACK = 32, depth + 1) less the LDS levels — the same for 12 and 15 levels —, and
    rpt_tree_generic's columns, gen_levels = depth + 1 high, which RPT_FLAG_GENERAL_TRAVERSAL and an irregular tree size
    themselves per call.  Left stale, they would be at least KNOT_DEPTH + 1 = 13 high for the default route's rays with a zero direction
    component, which defer one far child per split they cross.  The knot turns about y in its scene, so only a ray's y component
    stays exactly zero in the tree's frame, and such a ray crosses no y split: it defers at most `across` children.  So the
    cases that start from the knot cannot tell whether the workspace was marked (a tree that outgrows the spill columns is
    deeper than 32 levels, and the build rule needs more triangles than the knot has for one: scene_plan.h route_object,
    16 / 0.85^d).  mesh_from_two_leaves is the case that can: see test_level_rays_need_more_columns_than_two_leaves_had."""
    deep = tree_of(clustered(C.KNOT))
    assert splits_across(deep, (0, 1, 2)) == deep["max_depth"] == 15  # (the arrays are read as the kernels read them)
    across = splits_across(deep, (0, 2))
    assert across < C.KNOT_DEPTH + 1 < deep["max_depth"] + 1 <= 32, across


def deferred(tree, box, o, d, t_min=1e-12):
    """how many far children the walk of rpt_tree_generic holds deferred when it reaches its first leaf: one per split the ray
    crosses inside the cell it is in (the interval form of generic_walk's DESCEND; o, d in the tree's frame)"""
    with np.errstate(all="ignore"):
        t0, t1 = (box[:3] - o) / d, (box[3:] - o) / d
    lo, hi = max(np.nanmax(np.fmin(t0, t1)), t_min), np.nanmin(np.fmax(t0, t1))
    if not lo <= hi:
        return 0
    node, held = 0, 0
    while int(tree["info"][node]) & 3 != 3:
        axis, value = int(tree["info"][node]) & 3, tree["split"][node]
        with np.errstate(all="ignore"):
            ts = (value - o[axis]) / d[axis]
        left_first = o[axis] < value or (o[axis] == value and d[axis] <= 0.0)
        only_first = ts > hi or ts <= 0.0
        only_second = not only_first and ts < lo
        if not only_first and not only_second:
            held += 1
            hi = ts
        node = int(tree["a"][node]) + (0 if (left_first != only_second) else 1)
    return held


def test_level_rays_need_more_columns_than_two_leaves_had(oracle):
    """mesh_from_two_leaves: the handle is made with rpt_tree_generic's columns depth + 1 = 2 levels high; after set_mesh the
    level rays — a zero y component, in the knot's frame too, so the default route hands them to that kernel — hold more far
    children than that deferred on their way to the first leaf.  Columns left at two levels make the call fail
    (RPTGPU_E_TREE_TOO_DEEP); the walk checks its stack, nothing is written past it"""
    c = C.cases()["mesh_from_two_leaves"]
    o, d, _ = C.rays(c.name)
    level = np.arange(C.N_RAYS) % 4 == 0
    assert c.level and (d[level, 1] == 0.0).all() and (d[~level] != 0.0).all()
    placed = c.scene0.objects[0].shape
    inv = np.array(placed.inverse_transform).reshape(4, 4).T
    assert inv[1, 0] == 0.0 and inv[1, 2] == 0.0 and inv[3, 3] == 1.0  # turned about y only: a level ray stays level
    ol, dl = o @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T
    assert (dl[level, 1] == 0.0).all()
    knot = tree_of(C.KNOT)
    v = C.KNOT[:, :9].reshape(-1, 3)
    box = np.concatenate([v.min(axis=0), v.max(axis=0)])
    held = np.array([deferred(knot, box, ol[i], dl[i]) if level[i] else 0 for i in range(C.N_RAYS)])
    had = tree_of(C.TWO_LEAVES)["max_depth"] + 1
    hits = oracle.OracleScene(c.steps[0].scene).closest_hit(o, d)[2] == 0
    assert (held > had).mean() >= 0.05 and (level & hits).mean() >= 0.05, ((held > had).mean(), (level & hits).mean(), held.max())


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("update_cases") / "scene_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cpp", "scene_plan_check.cpp"), "-o", exe])

    def live(kind, tree, options, new):
        """the creation's route of `tree` under `options`, and its re-route after a rebuild into `new`"""
        args = [kind, tree["max_depth"], int(tree["regular"]), options.get("deep_depth", 8), options.get("fast_max_depth", 32),
                new["max_depth"], int(new["regular"])]
        r = subprocess.run([exe, "live"] + [str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
        names = ("deep", "tris", "tree_kids", "gen_all", "new_deep", "new_tris", "new_gen_all", "new_tree_kids", "refused")
        return dict(zip(names, (int(x) for x in r.stdout.split()[1:])))

    return live


def test_the_rebuilds_take_the_routes_the_cases_say(planner):
    knot = tree_of(C.KNOT)
    rebuilt = {"sine": tree_of(sine(C.KNOT)), "clustered": tree_of(clustered(C.KNOT)), "one leaf": tree_of(C.ONE_LEAF)}
    two = tree_of(C.TWO_LEAVES)
    r = planner(MESH, two, C.cases()["mesh_from_two_leaves"].options, knot)
    assert r["deep"] != 0 and r["new_deep"] == r["deep"] and not r["new_tree_kids"] and not r["new_gen_all"] and not r["refused"], r
    for name in ("mesh_same_depth", "mesh_deeper", "mesh_past_fast_stacks"):
        c = C.cases()[name]
        for step in c.steps:
            new = knot if step.back else rebuilt[step.name]
            r = planner(MESH, knot, c.options, new)
            assert r["deep"] != 0 and not r["tree_kids"] and not r["refused"], (name, r)  # the per-tree route, from creation on
            assert bool(r["new_tree_kids"]) == (name == "mesh_past_fast_stacks" and step.name == "clustered"), (name, step.name, r)
            assert bool(r["new_gen_all"]) == (not new["regular"]), (name, step.name, r)     # only where the tree is irregular
            assert bool(r["new_deep"] & 4) == (not new["regular"]) and r["new_deep"] & 3 == r["deep"] & 3
    # (every rebuilt tree of the cases is regular, so gen_all never rises in them; the planner does raise it for one that is not)
    assert all(t["regular"] for t in rebuilt.values())
    assert planner(MESH, knot, {"deep_depth": 1}, {"max_depth": knot["max_depth"], "regular": 0})["new_gen_all"] == 1
    kids = group_tree_of(C.KIDS)
    for route in ("in_kernel", "per_tree"):
        c = C.cases()["group_" + route]
        for step, motion in zip(c.steps, (jitter, kids_clustered, coincident, list)):
            new = group_tree_of(motion(C.KIDS))
            r = planner(GROUP, kids, c.options, new)
            assert (r["deep"] != 0) == (route == "per_tree") and not r["refused"] and not r["new_tree_kids"], (route, step.name, r)
            assert bool(r["new_gen_all"]) == (route == "per_tree" and not new["regular"]), (route, step.name, r)
            if route == "in_kernel":  # walked inside the kernels: only the one-leaf bit follows the tree
                assert r["new_deep"] == 0 and bool(r["new_tris"] & 16) == (new["max_depth"] == 0), (step.name, r)


# ---- the inputs of tests/test_gpu_update_newer.py: each can SEE the updates it is run across (a comparison of two wrong
# answers that agree would pass otherwise).  Every figure is the oracle's and is printed (-rP)
MOVING = [n for n in C.NAMES if C.cases()[n].moves]


def test_the_chart_owns_and_leaves_texels():
    import lightmap_model
    for name in C.NAMES:
        tris, uvs, w, h, offset = C.chart(name)
        assert tris.shape == (2, 3, 3) and uvs.shape == (2, 3, 2) and (w, h) == (13, 7) == (C.LM_W, C.LM_H)
        assert not tris.flags.writeable and not uvs.flags.writeable
        lo, hi = (np.array(v) for v in C.cases()[name].aim[0])
        v = tris.reshape(-1, 3)
        assert (v[:, 0].min(), v[:, 0].max(), v[:, 2].min(), v[:, 2].max()) == (lo[0], hi[0], lo[2], hi[2])      # the box's x-z extent
        assert len(set(v[:, 1].tolist())) == 1 and lo[1] < v[0, 1] < hi[1]                                        # level, inside it
        assert offset == 1e-3 * np.abs(tris).max() > 0.0
        raw = lightmap_model.raw(tris, None, uvs, w, h, offset=offset)
        owned = raw["owner"] >= 0
        assert owned.sum() >= 40 and (~owned).sum() >= 10, (name, int(owned.sum()))
        assert (raw["owner"] == 0).sum() >= 10 and (raw["owner"] == 1).sum() >= 10                                # both triangles own some
        assert not owned[0].any() and not owned[-1].any() and not owned[:, 0].any() and not owned[:, -1].any()   # a gutter on every side
        assert (raw["normal"][owned] == np.array([0.0, 1.0, 0.0])).all()                                          # the normal is up
        assert C.chart_texels(name)[1] is not None and len(C.chart_texels(name)[4]) == owned.sum()
    assert (C.LM_SAMPLES, C.PROBE_SAMPLES, C.DIRECT_SAMPLES) == (4, 6, 5)
    ids, base = C.streams("lights")
    assert len(set(ids.tolist())) == C.N_RAYS and (ids != np.arange(C.N_RAYS)).all() and base == C.points("lights")[2][0] != 0


@pytest.mark.parametrize("name", C.NAMES)
def test_ambient_occlusion_at_the_chart_sees_every_step_that_moves_geometry(name, oracle):
    """at max_distance = inf, the bake's first reach (the half-diagonal's figures are printed beside it): the unoccluded
    fraction is neither 0 nor 1 at every texel, before the update and after each step, and a step that moves geometry changes
    it on at least one texel (objects_filtered's second step takes away a sphere three units from the chart: one texel of
    55 sees it, at inf only); lights and materials change it nowhere"""
    c = C.cases()[name]
    ao = C.chart_ao(name)
    said = []
    for step, a in ao.items():
        differ = {far: int((a[far] != ao[None][far]).sum()) for far in ("inf", "half")}
        said.append("%s, %s: unoccluded %.2f (inf) %.2f (half); texels that differ from the creation's: %d (inf) %d (half) of %d"
                    % (name, step or "at creation", a["inf"].mean(), a["half"].mean(), differ["inf"], differ["half"], len(a["inf"])))
        assert not (a["inf"] == 0.0).all() and not (a["inf"] == 1.0).all(), said[-1]
        if step is not None:
            assert (differ["inf"] >= 1) if c.moves else (differ["inf"] == 0 and differ["half"] == 0), said[-1]
    assert len(ao) == len(c.steps)  # (the creation's scene and every step but the return)
    print("\n".join(said))


@pytest.mark.parametrize("name", C.NAMES)
def test_the_direct_light_at_the_points_changes_where_the_table_says(name, oracle):
    d = C.direct_at_points(name)
    assert sorted(C.DIRECT_CHANGES[name]) == sorted(k for k in d if k is not None)
    assert (d[None] != 0.0).any(axis=1).sum() >= 2 and (d[None] == 0.0).all(axis=1).sum() >= 2  # lit points, and dark ones
    said = []
    for step, want in C.DIRECT_CHANGES[name].items():
        changed = C.share(d[None], d[step])
        said.append("%s, %s: bake_direct changes at %.1f %% of the points; %d of 16 are lit" % (name, step, 100.0 * changed, (d[step] != 0.0).any(axis=1).sum()))
        assert (changed > 0.0) == want, said[-1]
    if name == "lights":
        assert C.DIRECT_CHANGES[name] == {"moved": True}
    if name == "materials_deeper":
        assert C.DIRECT_CHANGES[name] == {"glass and mirror": False}  # a shadow ray stops at any object
    print("\n".join(said))


@pytest.mark.parametrize("name", C.MESH_CASES)
def test_the_rays_end_on_triangles_of_the_updated_mesh(name, oracle):
    """Every step of a mesh case is a set_mesh of object 0, the return to the knot too, and after each the GPU test holds
    hit_surface's named triangles to surface_model.restate.  The floor — 10 % of the 600 rays end on a triangle of the
    updated mesh — is asked of the case: of the step after which most rays do.  Per step it cannot hold with the matrix's
    rays: mesh_deeper's `one leaf` is 1 536 copies of ONE triangle, which none of them hits (0 %), and its `clustered` draws
    the knot together (9.3 %; 10.3 % in mesh_past_fast_stacks, whose rays are other draws).  A step with rays on the mesh
    must show some; every share is printed"""
    found = C.on_updated_mesh(name)
    c = C.cases()[name]
    assert sorted(found) == sorted(s.name for s in c.steps) and name.startswith("mesh_") and c.updated == (0,)
    level = np.arange(C.N_RAYS) % 4 == 0
    print("\n".join("%s, %s: %.1f %% of the rays end on a triangle of the updated mesh (%.1f %% are level rays that do)"
                    % (name, k, 100.0 * v.mean(), 100.0 * (v & level).mean()) for k, v in found.items()))
    assert max(v.mean() for v in found.values()) >= 0.10
    for k, v in found.items():
        if k not in ("one leaf", "two leaves"):
            assert v.mean() >= 0.05, k
    if name == "mesh_from_two_leaves":
        assert c.level and found["the knot"].mean() >= 0.10 and (found["the knot"] & level).mean() >= 0.05
