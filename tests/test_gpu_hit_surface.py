"""rptgpu_hit_surface on the GPU: the triangle, the barycentrics and the group's child behind a ray's first hit
(include/rpt_gpu_hit_surface.h).

Every comparison is on bits (aov_model.bits).  The yardsticks are things the repository already pins, not the code under test:
t and object are GpuScene.closest_hit's; the triangle a ray names must REPRODUCE closest_hit's record — Triangle::intersect
restated in numpy (surface_model.tri_records: held to the oracle without a GPU by test_hit_surface_host.py) gives that time, the
reported weights, all >= 0, and that shading normal; the child a ray names must be hit at that t by the independent path tracer's
Shape::intersect, and a handle whose group holds ONLY that child must return the same t and normal.

Scenes and rays: test_gpu_occlusion.rays for cornell (flat), coverage (every shape, a transformed mesh, a group), wine_glass (a
deep mesh through the per-tree query), monomial (the ext build, NaN records), nested_groups (groups in groups with a mesh child:
the generic walker); routes_cases.rays for fractal_spheres (groups walked in-kernel) and fractal_teapots (groups of meshes,
rpt_nest_trace, the ext build).  600 rays each: three 256-thread blocks, the last one partial.  Those box rays land on a triangle
often in cornell (66 %) and wine_glass (34 %) but seldom in coverage (1 %), fractal_teapots (6 %) and nested_groups (0.3 %), whose
meshes are small; so every scene with triangles ALSO runs 600 rays aimed at its triangles (surface_model.aimed_rays), every
property is checked on both sets, and the condition that at least 10 % of a mesh scene's rays land on a triangle is asserted over
both together.

Transformed meshes and meshes inside groups: the local ray and the normal transform come from the host mirror's matrices
(rpt_amd/glm.py) in nalgebra's operation order, which restates the library's arithmetic to the bit (test_hit_surface_host.py holds
that against the oracle first), so they are held to the bits as well — not to test_independent_geometry.py's bound for numpy's own
inverses (|dt| <= 1e-11 max(1, |t|), normals to 1e-9), which would be the bound otherwise."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, KdTree, Material, Mesh, Object, Scene, _abi, polygon
from rpt_amd import shape as S
from rpt_amd.shape import Triangle

import routes_cases
import small_scenes
import surface_model as M
import test_gpu_occlusion as occ
import test_independent_pathtracer as P

pytestmark = pytest.mark.gpu

OCC_SCENES = ("cornell", "coverage", "wine_glass", "monomial", "nested_groups")
ROUTE_SCENES = ("fractal_spheres", "fractal_teapots")
SCENES = OCC_SCENES + ROUTE_SCENES
MESH_SCENES = ("cornell", "coverage", "wine_glass", "nested_groups", "fractal_teapots")  # a triangle can be hit
GROUP_SCENES = ("coverage", "nested_groups", "fractal_spheres", "fractal_teapots")      # a group's child can be hit
N = occ.N_RAYS
GENERAL = _abi.RPT_FLAG_GENERAL_TRAVERSAL
FLAGS = pytest.mark.parametrize("flags", [0, GENERAL], ids=["default", "general"])
CHANNELS = (("t", _abi.RPT_SURFACE_T), ("object", _abi.RPT_SURFACE_OBJECT), ("child", _abi.RPT_SURFACE_CHILD),
            ("primitive", _abi.RPT_SURFACE_PRIMITIVE), ("barycentric", _abi.RPT_SURFACE_BARYCENTRIC))
WALK = _abi.RPT_SURFACE_PRIMITIVE | _abi.RPT_SURFACE_BARYCENTRIC
EPSILON = 1e-12
INF = float("inf")
same = M.same
bits = M.bits


def scene_of(name):
    return small_scenes.small(name)[0]


@functools.lru_cache(maxsize=None)
def gpu(name):
    return occ.gpu(name) if name in OCC_SCENES else GpuScene(scene_of(name), 0)


def box_of(name):
    return occ.BOXES[name] if name in OCC_SCENES else routes_cases.BOXES[name]


def kinds(name):
    return ("box", "aimed") if name in MESH_SCENES else ("box",)


@functools.lru_cache(maxsize=None)
def rays(name, kind):
    if kind == "aimed":
        return M.aimed_rays(scene_of(name), box_of(name), sum(map(ord, name)) + 7)
    return occ.rays(name)[:2] if name in OCC_SCENES else routes_cases.rays(name)


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(origins, directions, closest_hit's t, normal and object, hit_surface's record) — computed once, shared, read-only"""
    o, d = rays(name, kind)
    g = gpu(name)
    t, nrm, obj = g.closest_hit(o, d)
    got = g.hit_surface(o, d)
    for a in (t, nrm, obj) + tuple(got.values()):
        a.setflags(write=False)
    return o, d, t, nrm, obj, got


@functools.lru_cache(maxsize=None)
def both_sets(name):
    """case(name, kind) over the scene's kinds, one after the other"""
    parts = [case(name, kind) for kind in kinds(name)]
    cat = lambda k: np.concatenate([p[k] for p in parts])
    got = {k: np.concatenate([p[5][k] for p in parts]) for k in parts[0][5]}
    return cat(0), cat(1), cat(2), cat(3), cat(4), got


def differing(got, want):
    return [k for k in want if k not in got or not same(got[k], want[k])] + [k for k in got if k not in want]


def test_the_box_rays_are_the_neighbours():
    for name in ("cornell", "coverage", "wine_glass", "nested_groups"):
        assert all(same(a, b) for a, b in zip(M.box_rays(name), occ.rays(name)[:2]))


# ---- 1. t and object are closest_hit's; a miss and a NaN record name nothing
@FLAGS
@pytest.mark.parametrize("name", SCENES)
def test_t_and_object_are_closest_hits(name, flags):
    g = gpu(name)
    for kind in kinds(name):
        o, d, t, _, obj, _ = case(name, kind)
        g.reset_stats()
        got = g.hit_surface(o, d, flags=flags)
        st = g.stats()
        assert sorted(got) == ["barycentric", "child", "object", "primitive", "t"]
        assert same(got["t"], t) and same(got["object"], obj)
        assert st.samples == 0 and st.extend_rays == 0 and st.shadow_rays == 0 and st.total_ms > 0.0
        assert st.kernel_launches[_abi.RPT_K_EXTEND] == 1
        miss = obj < 0
        assert (miss.any() or kind == "aimed") and np.isposinf(got["t"][miss]).all()
        nothing = miss | np.isnan(t)
        assert (got["child"][nothing] == -1).all() and (got["primitive"][nothing] == -1).all()
        assert (bits(got["barycentric"][got["primitive"] < 0]) == 0).all()
    if name == "monomial":
        assert (np.isnan(t) & (obj >= 0)).any()  # the NaN records are there


# ---- 2. the named triangle reproduces the record
@FLAGS
@pytest.mark.parametrize("name", MESH_SCENES)
def test_the_named_triangle_reproduces_the_record(name, flags):
    scene, g = scene_of(name), gpu(name)
    on_triangle = total = 0
    for kind in kinds(name):
        o, d, t, nrm, obj, _ = case(name, kind)
        got = g.hit_surface(o, d, flags=flags)
        prim, bary = got["primitive"], got["barycentric"]
        idx, plain, time, uvw, normal = M.restate(scene, o, d, obj, got["child"], prim)
        assert len(idx) == (prim >= 0).sum()  # (no mesh of these scenes lies deeper than a group's child)
        assert same(time, t[idx]), (kind, np.flatnonzero(bits(time) != bits(t[idx]))[:5])
        assert same(uvw, bary[idx]), kind
        assert (bary[idx] >= 0.0).all()
        assert same(normal, nrm[idx]), (kind, np.flatnonzero((bits(normal) != bits(nrm[idx])).any(axis=1))[:5])
        on_triangle += len(idx)
        total += len(o)
        if name in ("cornell", "wine_glass"):
            assert plain.any()   # an untransformed top-level mesh
        if name in ("coverage", "nested_groups", "fractal_teapots"):
            assert (~plain).any()  # a transformed mesh, a mesh inside a group
    assert on_triangle >= 0.10 * total, (on_triangle, total)


# ---- 3. primitive == -1 exactly where the hit shape is no triangle, child == -1 exactly where the object is no group
@FLAGS
@pytest.mark.parametrize("name", SCENES)
def test_primitive_and_child_say_what_the_scene_says(name, flags):
    scene, g = scene_of(name), gpu(name)
    groups = np.array([M.is_group(M.unwrap(ob.shape)[1]) for ob in scene.objects])
    for kind in kinds(name):
        o, d, t, _, obj, _ = case(name, kind)
        got = g.hit_surface(o, d, flags=flags)
        named = (obj >= 0) & ~np.isnan(t)
        in_group = named & groups[np.maximum(obj, 0)]
        assert ((got["child"] >= 0) == in_group).all()
        for i in np.flatnonzero(in_group):
            assert got["child"][i] < len(M.unwrap(scene.objects[obj[i]].shape)[1].objects)
        want_triangle = np.zeros(len(o), dtype=bool)
        for i in np.flatnonzero(named):
            shape = M.hit_shape(scene, int(obj[i]), int(got["child"][i]))[1]
            assert M.is_mesh(shape) or not M.contains_triangles(shape)  # (so the scene decides)
            want_triangle[i] = M.is_mesh(shape)
        assert ((got["primitive"] >= 0) == want_triangle).all()
        for i in np.flatnonzero(want_triangle):
            assert got["primitive"][i] < len(M.hit_shape(scene, int(obj[i]), int(got["child"][i]))[1].triangles)
        if name in GROUP_SCENES:
            assert in_group.sum() >= 10


# ---- 4. the named child
def restated(shape):
    """is the shape inside test_independent_pathtracer.intersect's closed set?"""
    core = M.unwrap(shape)[1]
    if isinstance(core, (S.Sphere, S.Cube)):
        return True
    if M.is_mesh(core):
        return True
    return False  # (a MonomialSurface, a group inside a group: the oracle's Shape::intersect stands in)


def holds_monomial(shape):
    core = M.unwrap(shape)[1]
    return isinstance(core, S.MonomialSurface) or (M.is_group(core) and any(holds_monomial(k) for k in core.objects))


def into(xf, o, d):
    """the ray in the space inside a Transformed, with numpy's inverse, as test_independent_pathtracer.intersect does it"""
    if xf is None:
        return o, d
    minv = np.linalg.inv(np.array(xf.transform_m).reshape(4, 4).T)
    return (minv @ np.append(o, 1.0))[:3], (minv @ np.append(d, 0.0))[:3]


def monomial_residuals(shape, o, d, t):
    """|y - height (x^2 + z^2)^2| at the ray's point at t, for every MonomialSurface inside `shape` whose disc holds it"""
    xf, core = M.unwrap(shape)
    o, d = into(xf, o, d)
    if M.is_group(core):
        return [r for k in core.objects for r in monomial_residuals(k, o, d, t)]
    if not isinstance(core, S.MonomialSurface):
        return []
    p = o + t * d
    s = p[0] * p[0] + p[2] * p[2]
    return [abs(p[1] - core.height * (s * s))] if s <= 1.0 + 1e-9 else []


def child_is_hit_at(outer, child, o, d, t):
    """does the child's own Shape::intersect for the world ray (o, d) give t, to test_independent_pathtracer.py's agreement
    for whole samples (1e-9 relative)?  That file's restatement where it covers the child; the oracle's Shape::intersect for
    a MonomialSurface or a group that holds one.  Such a child is the one shape whose answer depends on t_min beyond the
    guard — its bisection STARTS at t_min (monomial_surface.rs:50-104), and inside a group's tree a far child is entered with
    t_min = t_split (kdtree.rs:213-220) —, so where t_min = 1e-12 does not give t, the point at t must lie ON one of its
    monomial surfaces instead"""
    o, d = into(outer, o, d)
    tol = 1e-9 * max(1.0, abs(t))
    if restated(child):
        hit, tc, _ = P.intersect(child, o, d, EPSILON, INF)
        return hit and abs(tc - t) <= tol
    from oracle import oracle_ffi
    hit, tc, _ = oracle_ffi.shape_intersect(child, o, d, EPSILON, INF)
    if hit and abs(tc - t) <= tol:
        return True
    return any(r <= tol for r in monomial_residuals(child, o, d, t))


@pytest.mark.parametrize("name", GROUP_SCENES)
def test_the_named_child_is_hit_there(name):
    """test_independent_pathtracer.py's agreement for whole samples: 1e-9 relative"""
    scene = scene_of(name)
    checked = 0
    for kind in kinds(name):
        o, d, t, _, obj, got = case(name, kind)
        for i in np.flatnonzero(got["child"] >= 0)[:150]:
            outer, core = M.unwrap(scene.objects[obj[i]].shape)
            assert child_is_hit_at(outer, core.objects[got["child"][i]], o[i], d[i], t[i]), (kind, i, got["child"][i], t[i])
            checked += 1
    assert checked >= 10


@pytest.mark.parametrize("name", GROUP_SCENES)
def test_a_group_of_the_named_child_alone_gives_the_record(name):
    """(the children whose record does not depend on where the group's tree cut the ray: no MonomialSurface inside —
    child_is_hit_at says why)"""
    scene = scene_of(name)
    o, d, t, nrm, obj, got = both_sets(name)
    pairs, counts = np.unique(np.stack([obj, got["child"]], axis=1)[got["child"] >= 0], axis=0, return_counts=True)
    free = np.array([not holds_monomial(M.unwrap(scene.objects[ob].shape)[1].objects[ch]) for ob, ch in pairs])
    pairs, counts = pairs[free], counts[free]
    assert len(pairs) >= 2
    for ob, ch in pairs[np.argsort(-counts, kind="stable")][:8]:
        outer, core = M.unwrap(scene.objects[ob].shape)
        alone = KdTree([core.objects[ch]])
        lone = Scene()
        lone.add(Object(S.Transformed(alone, outer.transform_m) if outer is not None else alone))
        sel = np.flatnonzero((obj == ob) & (got["child"] == ch))
        h = GpuScene(lone, 0)
        t1, n1, o1 = h.closest_hit(o[sel], d[sel])
        s1 = h.hit_surface(o[sel], d[sel])
        h.close()
        assert (o1 == 0).all() and same(t1, t[sel]) and same(n1, nrm[sel]), (ob, ch)
        assert (s1["child"] == 0).all() and same(s1["primitive"], got["primitive"][sel]) and same(s1["barycentric"], got["barycentric"][sel])


# ---- 5. ties: the first tested wins
def flat_grid(nx, ny):
    """2 nx ny triangles tiling [0, nx] x [0, ny] in the plane z = 0, their normals +z"""
    tris = []
    for y in range(ny):
        for x in range(nx):
            a, b, c, e = (x, y, 0.0), (x + 1.0, y, 0.0), (x + 1.0, y + 1.0, 0.0), (x, y + 1.0, 0.0)
            tris += [Triangle.from_vertices(a, b, c), Triangle.from_vertices(a, c, e)]
    return tris


def tie_check(tris, o, d, expect=None):
    """hit_surface on a scene of one untransformed mesh; every ray must hit it, and test (2)'s check decides"""
    mesh = Mesh(tris)
    scene = Scene()
    scene.add(Object(mesh).material(Material.diffuse((0.5, 0.5, 0.5))))
    g = GpuScene(scene, 0)
    o, d = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)
    t, nrm, obj = g.closest_hit(o, d)
    both = [g.hit_surface(o, d), g.hit_surface(o, d, flags=GENERAL)]
    g.close()
    assert (obj == 0).all()
    assert differing(both[1], both[0]) == []
    got = both[0]
    assert same(got["t"], t) and (got["child"] == -1).all() and (got["primitive"] >= 0).all()
    idx, _, time, uvw, normal = M.restate(scene, o, d, obj, got["child"], got["primitive"])
    assert len(idx) == len(o) and same(time, t) and same(uvw, got["barycentric"]) and (uvw >= 0.0).all() and same(normal, nrm)
    if expect is not None:
        assert (got["primitive"] == expect).all(), got["primitive"]
    return got, mesh.triangles


def first_accepted(rows, o, d):
    """Triangle::intersect over `rows` in list order on one record (a one-leaf mesh: the leaf order is the list order)"""
    win = np.full(len(o), -1)
    for i in range(len(o)):
        rec = INF
        n = len(rows)
        time, uvw, _ = M.tri_records(rows, np.repeat(o[i:i + 1], n, 0), np.repeat(d[i:i + 1], n, 0))
        for k in range(n):
            if time[k] >= EPSILON and time[k] < rec and (uvw[k] >= 0.0).all():
                rec, win[i] = time[k], k
    return win


TILT_A, TILT_B = (0.3, 0.0, 1.0), (0.0, -0.4, 1.0)  # vertex normals that tell the two coincident triangles apart


def unit(v):
    v = np.array(v, dtype=np.float64)
    return tuple(v / np.sqrt((v * v).sum()))


@pytest.mark.parametrize("order", ["first", "last"])
def test_ties_coincident_triangles_with_distinct_normals(order):
    """two coincident triangles with different vertex normals inside a mesh of 34 triangles (a tree with inner nodes): both
    would be accepted at the final t, the first one tested wrote the record — the one whose normals closest_hit returned"""
    grid = flat_grid(4, 4)
    v = ((1.0, 1.0, 0.0), (2.0, 1.0, 0.0), (2.0, 2.0, 0.0))  # grid triangle 10, again
    a = Triangle(*v, unit(TILT_A), unit(TILT_A), unit(TILT_A))
    b = Triangle(*v, unit(TILT_B), unit(TILT_B), unit(TILT_B))
    rest = grid[:10] + grid[11:]  # (the flat original would tie too)
    tris = [a, b] + rest if order == "first" else rest + [b, a]
    assert len(tris) == 33
    o = [(1.75, 1.25, 2.0), (1.5, 1.25, 1.0), (1.875, 1.5, 3.0), (2.25, 0.75, 2.0)]
    d = [(0.0, 0.0, -1.0), (0.0, 0.0, -2.0), (0.0, 0.0, -0.5), (-0.25, 0.25, -1.0)]
    got, rows = tie_check(tris, o, d)
    pair = {0, 1} if order == "first" else {31, 32}
    assert set(got["primitive"].tolist()) <= pair


def test_ties_coincident_triangles_with_identical_normals_in_one_leaf():
    """... and with identical normals only the index tells: in a one-leaf mesh the leaf order is the list order, so the lower
    index wins"""
    grid = flat_grid(2, 2)  # 8 triangles: fewer than 16, node 0 is a leaf
    v = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 0.0))
    twin = Triangle.from_vertices(*v)
    tris = grid[:3] + [twin] + grid[3:] + [Triangle.from_vertices(*v)]  # grid triangle 0 again, at 3 and at 9
    o = [(0.75, 0.25, 2.0), (0.5, 0.25, 1.0), (1.5, 0.75, 2.0)]
    d = [(0.0, 0.0, -1.0), (0.0, 0.0, -3.0), (-0.375, -0.25, -1.0)]
    got, rows = tie_check(tris, o, d, expect=0)
    assert (first_accepted(rows, np.array(o), np.array(d)) == 0).all()


def test_ties_a_quad_hit_on_its_diagonal():
    """polygon()'s fan (shape.rs:307-313): both triangles of the quad accept a point of the shared diagonal at the same
    time; the first of the leaf, triangle 0, wrote the record"""
    quad = polygon([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 0.0)])
    tris = quad.triangles  # (n, 18) rows: Mesh takes them as they are
    s = np.array([0.125, 0.25, 0.5, 0.75, 0.875])
    o = np.stack([s, s, np.full(5, 2.0)], axis=1)
    d = np.tile(np.array([0.0, 0.0, -1.0]), (5, 1))
    got, rows = tie_check(tris, o, d, expect=0)
    assert (first_accepted(rows, o, d) == 0).all()
    assert (got["barycentric"][:, 1] == 0.0).all()  # on the edge v1-v3 of triangle 0: v2's weight is exactly zero


def test_ties_a_hit_on_a_shared_vertex():
    """a pyramid's apex, shared by its faces (distinct normals), in a one-leaf mesh and inside a tree with inner nodes"""
    apex = (2.0, 2.0, 1.0)
    ring = [(1.0, 1.0, 0.0), (3.0, 1.0, 0.0), (3.0, 3.0, 0.0), (1.0, 3.0, 0.0)]
    faces = [Triangle.from_vertices(apex, ring[k], ring[(k + 1) % 4]) for k in range(4)]
    o = [(2.0, 2.0, 3.0), (2.0, 2.0, 5.0)]
    d = [(0.0, 0.0, -1.0), (0.0, 0.0, -0.5)]
    got, rows = tie_check(faces, o, d)
    assert same(got["primitive"], first_accepted(rows, np.array(o), np.array(d)).astype(np.int32))
    below = [Triangle.from_vertices(*[(x, y, -1.0) for x, y, _ in (t.v1, t.v2, t.v3)]) for t in flat_grid(4, 4)]
    got, _ = tie_check(below + faces, o, d)  # 36 triangles
    assert (got["primitive"] >= 32).all()


# ---- 6. a ray's result depends on that ray and the scene and on nothing else
@pytest.mark.parametrize("name", SCENES)
def test_pieces_order_and_company_change_nothing(name, monkeypatch):
    o, d, _, _, _, want = case(name, kinds(name)[-1])
    g = gpu(name)
    monkeypatch.setenv("RPTGPU_SURFACE_PIECE", "256")  # three pieces, the last with 88 rays
    g.reset_stats()
    assert differing(g.hit_surface(o, d), want) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == 3
    assert differing(g.hit_surface(o[::-1], d[::-1]), {k: v[::-1] for k, v in want.items()}) == []
    sub = np.sort(np.random.RandomState(3).permutation(N)[:300])  # a subset: 256 + 44
    assert differing(g.hit_surface(o[sub], d[sub], flags=GENERAL), {k: v[sub] for k, v in want.items()}) == []
    monkeypatch.delenv("RPTGPU_SURFACE_PIECE")
    for i in np.flatnonzero(want["object"] >= 0)[:3]:  # alone
        assert differing(g.hit_surface(o[i:i + 1], d[i:i + 1]), {k: v[i:i + 1] for k, v in want.items()}) == []


def test_one_channel_of_a_host_caller_in_pieces_of_three(monkeypatch):
    """7 rays in pieces of 3 — the last holds one —, BARYCENTRIC alone (not the first channel, three components), against the
    same rays in one piece with every channel: a wrong staging offset, component count or row of the channel table shows"""
    o, d, _, _, _, want = case("cornell", "box")
    hit = want["primitive"] >= 0
    idx = np.sort(np.concatenate([np.flatnonzero(hit)[:4], np.flatnonzero(~hit)[:3]]))
    assert len(idx) == 7
    o, d = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    g = gpu("cornell")
    whole = g.hit_surface(o, d)
    monkeypatch.setenv("RPTGPU_SURFACE_PIECE", "3")
    g.reset_stats()
    assert differing(g.hit_surface(o, d, channels=_abi.RPT_SURFACE_BARYCENTRIC), {"barycentric": whole["barycentric"]}) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == 3
    assert differing(whole, {k: v[idx] for k, v in want.items()}) == []


# ---- 7. a channel that is not named is not written
@pytest.mark.parametrize("name", ["wine_glass", "fractal_spheres"])
def test_every_single_channel_and_nothing_else(name):
    o, d, _, _, _, want = case(name, "box")
    g = gpu(name)
    lib, PD = g.lib, _abi.C.POINTER(_abi.C.c_double)
    types = dict(_abi.RptSurfaceArrays._fields_)
    o, d = np.array(o), np.array(d)
    for only, bit in CHANNELS + (("primitive+barycentric", WALK),):
        names = only.split("+")
        assert differing(g.hit_surface(o, d, channels=bit), {k: want[k] for k in names}) == []
        # through the ABI with EVERY pointer set: the arrays of the other channels keep their sentinel
        outs = {k: np.full(want[k].shape, 7, dtype=want[k].dtype) for k, _ in CHANNELS}
        q, a = _abi.RptSurfaceQuery(), _abi.RptSurfaceArrays()
        q.struct_size, q.channels = _abi.C.sizeof(q), bit
        a.struct_size = _abi.C.sizeof(a)
        for k, v in outs.items():
            setattr(a, k, v.ctypes.data_as(types[k]))
        _abi.check(lib.rptgpu_hit_surface(g.handle, N, o.ctypes.data_as(PD), d.ctypes.data_as(PD), _abi.C.byref(q), _abi.C.byref(a)),
                   g.handle)
        assert all(same(outs[k], want[k]) for k in names), only
        assert all((v == 7).all() for k, v in outs.items() if k not in names), only


# ---- 8. device arrays
@pytest.mark.parametrize("name", routes_cases.DEVICE_FORMS + ("wine_glass",))
def test_device_arrays_give_the_host_calls_bits(name, monkeypatch):
    o, d, _, _, _, want = case(name, "box")
    g = gpu(name)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a writable, contiguous copy of the shared arrays)
    got = g.hit_surface(to(o), to(d))
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values())
    assert got["primitive"].dtype == torch.int32 and got["barycentric"].dtype == torch.float64
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, want) == []
    monkeypatch.setenv("RPTGPU_SURFACE_PIECE", "256")
    got = g.hit_surface(to(o), to(d), channels=WALK, flags=GENERAL)  # T and OBJECT in the handle's own pair
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, {k: want[k] for k in ("primitive", "barycentric")}) == []
    with torch.cuda.stream(torch.cuda.Stream(dev)):  # on a stream of the caller's own
        got = g.hit_surface(to(o), to(d), channels=_abi.RPT_SURFACE_CHILD | _abi.RPT_SURFACE_T)
        assert differing({k: v.cpu().numpy() for k, v in got.items()}, {k: want[k] for k in ("t", "child")}) == []
    with pytest.raises(ValueError):
        g.hit_surface(to(o), d)  # a host array beside a device tensor


# ---- 9. live updates
def test_after_set_mesh_the_results_are_a_fresh_handles():
    scene = scene_of("wine_glass")
    o, d, _, _, _, before = case("wine_glass", "aimed")
    g = GpuScene(scene, 0)
    assert differing(g.hit_surface(o, d), before) == []
    rows = np.array(M.unwrap(scene.objects[0].shape)[1].triangles)
    rows[:, 0:9:3] = rows[:, 0:9:3] * 1.15 + 0.1 * rows[:, 1:9:3]  # wider, and sheared along x with the height
    g.set_mesh(0, rows)
    got = g.hit_surface(o, d)
    moved = small_scenes.small("wine_glass")[0]
    moved.objects[0].shape = Mesh(rows)
    fresh = GpuScene(moved, 0)
    new = fresh.hit_surface(o, d)
    t, nrm, obj = fresh.closest_hit(o, d)
    fresh.close()
    g.close()
    assert differing(got, new) == []
    assert same(new["t"], t) and not same(new["primitive"], before["primitive"])  # (it did change)
    idx, _, time, uvw, normal = M.restate(moved, o, d, obj, new["child"], new["primitive"])
    assert len(idx) >= 60 and same(time, t[idx]) and same(uvw, new["barycentric"][idx]) and same(normal, nrm[idx])


def test_after_set_group_the_results_are_a_fresh_handles():
    scene = scene_of("fractal_spheres")
    o, d, _, _, _, before = case("fractal_spheres", "box")
    g = GpuScene(scene, 0)
    assert differing(g.hit_surface(o, d), before) == []
    kids = M.unwrap(scene.objects[2].shape)[1].objects  # 30 spheres: a tree with inner nodes, rebuilt on the device
    new_kids = [k.scale((1.2, 0.9, 1.1)).translate((0.01 * i, -0.01 * i, 0.02)) for i, k in enumerate(kids)][::-1]
    g.set_group(2, new_kids)
    got = g.hit_surface(o, d)
    moved = small_scenes.small("fractal_spheres")[0]
    moved.objects[2].shape = KdTree(new_kids)
    fresh = GpuScene(moved, 0)
    new = fresh.hit_surface(o, d)
    t, _, obj = fresh.closest_hit(o, d)
    fresh.close()
    g.close()
    assert differing(got, new) == []
    assert same(new["t"], t) and same(new["object"], obj) and (new["object"] == 2).sum() >= 10
    assert not same(new["child"], before["child"])  # (they did move)


# ---- 10. nothing to do, the refusals on a live handle, the stats
def test_nothing_to_do_refusals_and_stats_on_a_live_handle():
    g = gpu("cornell")
    o, d, _, _, _, want = case("cornell", "box")
    o, d = np.array(o), np.array(d)
    params = small_scenes.small("cornell")[2]
    camera = small_scenes.small("cornell")[1]
    frame = g.render_batch(camera, params)
    none = g.hit_surface(np.zeros((0, 3)), np.zeros((0, 3)))
    assert none["t"].shape == (0,) and none["barycentric"].shape == (0, 3) and none["primitive"].dtype == np.int32
    dev = torch.device("cuda", 0)
    none = g.hit_surface(torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros((0, 3), dtype=torch.float64, device=dev))
    assert none["barycentric"].shape == (0, 3)
    for kw, word in ((dict(flags=_abi.RPT_FLAG_PERSISTENT), "RPT_FLAG_PERSISTENT"), (dict(channels=0), "channels == 0"),
                     (dict(channels=32), "unknown RPT_SURFACE_")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            g.hit_surface(o, d, **kw)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
    # through the ABI: every refusal leaves the arrays untouched
    PD = _abi.C.POINTER(_abi.C.c_double)
    types = dict(_abi.RptSurfaceArrays._fields_)

    def call(q_kw=(), a_kw=(), drop=None, n=N, rays=True):
        outs = {k: np.full(want[k].shape, 7, dtype=want[k].dtype) for k, _ in CHANNELS}
        q, a = _abi.RptSurfaceQuery(), _abi.RptSurfaceArrays()
        q.struct_size, q.channels = _abi.C.sizeof(q), _abi.RPT_SURFACE_ALL
        a.struct_size = _abi.C.sizeof(a)
        for k, v in outs.items():
            if k != drop:
                setattr(a, k, v.ctypes.data_as(types[k]))
        for k, v in dict(q_kw).items():
            setattr(q, k, v)
        for k, v in dict(a_kw).items():
            setattr(a, k, v)
        rc = g.lib.rptgpu_hit_surface(g.handle, n, o.ctypes.data_as(PD) if rays else None, d.ctypes.data_as(PD), _abi.C.byref(q),
                                      _abi.C.byref(a))
        return rc, g.lib.rptgpu_last_error_detail(g.handle), outs

    refusals = [(dict(q_kw={"struct_size": 12}), b"RptSurfaceQuery: struct_size"), (dict(a_kw={"struct_size": 40}), b"RptSurfaceArrays: struct_size"),
                (dict(q_kw={"channels": 0}), b"channels == 0"), (dict(q_kw={"channels": 64}), b"unknown RPT_SURFACE_"),
                (dict(a_kw={"reserved": 1}), b"reserved != 0"), (dict(q_kw={"precision_mode": 1}), b"unknown precision_mode"),
                (dict(q_kw={"flags": _abi.RPT_FLAG_PERSISTENT}), b"RPT_FLAG_PERSISTENT"), (dict(rays=False), b"null argument")]
    refusals += [(dict(drop=k), ("RPT_SURFACE_%s is named but %s is NULL" % (k.upper(), k)).encode()) for k, _ in CHANNELS]
    g.reset_stats()
    for kw, word in refusals:
        rc, detail, outs = call(**kw)
        assert rc == _abi.RPTGPU_E_INVALID_ARGUMENT and word in detail, (kw, detail)
        assert all((v == 7).all() for v in outs.values()), kw
    rc, _, outs = call(n=0)
    assert rc == _abi.RPTGPU_OK and all((v == 7).all() for v in outs.values())
    st = g.stats()
    assert st.kernel_launches[_abi.RPT_K_EXTEND] == 0 and st.total_ms == 0.0  # none of them reached the device
    # the handle is as good as before: the same records, the same frame
    assert differing(g.hit_surface(o, d), want) == []
    st = g.stats()
    assert st.kernel_launches[_abi.RPT_K_EXTEND] == 1 and st.samples == 0 and st.extend_rays == 0 and st.shadow_rays == 0
    assert sum(st.kernel_launches) == 1  # rpt_hit_surface is counted under no RPT_K_* kind
    assert st.total_ms > 0.0
    g.hit_surface(o, d, channels=_abi.RPT_SURFACE_T, flags=_abi.RPT_FLAG_PROFILE_KERNELS)
    assert g.stats().kernel_ms[_abi.RPT_K_EXTEND] > 0.0
    assert same(g.render_batch(camera, params), frame)
