"""Scenes and ray populations aimed at the f32 leaf-box filter (kernels/shapes.inc boxray_make / box_window /
leaf_box_pass / kd_leaf_boxed and the group branch of kd_leaf), shared by tests/test_leaf_boxes.py (the numpy model, no
GPU) and tests/test_gpu_leaf_boxes.py (the device code against the oracle).  Everything is seeded.

Scenes (`build(name)`): `knot` and `knot_thin` (one mesh, plain and under a thin off-centre placement), `bundles` (the knot
plus stacks of k mutually overlapping triangles that the kd build must leave in ONE leaf: leaves of up to 100 entries),
`group` (about 200 spheres and cubes around quadric_too_small's threshold, under a non-uniform placement) and `nested` (a
group whose children are two meshes and spheres: rpt_nest_trace).  Populations (`population(scene, name)`): rays through
triangle interiors, edges and vertices, sphere silhouettes, nearly and exactly axis-parallel rays, far origins, and rays
through the bundles whose first hit is an entry in every position of its leaf."""
import math

import numpy as np

from rpt_amd import KdTree, Light, Material, Mesh, Object, Scene, cube, plane, scenes, sphere

GRID = 65529.0
BUNDLE_SIZES = (3, 8, 9, 16, 31, 32, 33, 64, 65, 100)
FAR_BANDS = ((0.0, 10.0), (10.0, 12.0), (12.0, 14.0), (14.0, 16.0))
LEAF_CLASSES = ((3, 8), (9, 16), (17, 32), (33, 64), (65, 1 << 30))
POSITION_CLASSES = ((0, 7), (8, 31), (32, 63), (64, 1 << 30))


def matrix(shape):
    """the 4x4 placement of a shape (row-major numpy); the identity if it is not Transformed"""
    m = getattr(shape, "transform_m", None)
    return np.eye(4) if m is None else np.array(m, dtype=np.float64).reshape(4, 4).T


def place(m, p):
    return p @ m[:3, :3].T + m[:3, 3]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _grey():
    return Material.diffuse((0.7, 0.7, 0.7))


# ---- scenes ---------------------------------------------------------------------------------------------------------
class Built:
    """scene: the rpt_amd.Scene; tris: (n, 9) world-space triangles to aim at; spheres / cubes: (n, 4, 4) world
    placements of the unit sphere / the cube [-0.5, 0.5]^3; lo, hi: the world bounds of all of these (not the floor)"""

    def __init__(self, scene, tris=None, spheres=None, cubes=None, **more):
        self.scene = scene
        self.tris = np.zeros((0, 9)) if tris is None else tris
        self.spheres = np.zeros((0, 4, 4)) if spheres is None else spheres
        self.cubes = np.zeros((0, 4, 4)) if cubes is None else cubes
        pts = [self.tris.reshape(-1, 3)]
        corners = np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
        for ms, half in ((self.spheres, 1.0), (self.cubes, 0.5)):
            for m in ms:
                pts.append(place(m, corners * half))
        pts = np.concatenate(pts)
        self.lo, self.hi = pts.min(axis=0), pts.max(axis=0)
        self.__dict__.update(more)


def _scene(shape, light=None):
    s = Scene()
    s.add(Object(plane((0.0, 1.0, 0.0), -1.0)).material(_grey()))
    s.add(Object(shape).material(_grey()))
    if light is not None:
        s.add(Light.Point((30.0, 30.0, 30.0), tuple(float(x) for x in light)))
    return s


def knot_rows():
    return scenes.knot_mesh(96, 12)     # 2 304 triangles


def knot(light=None, island=None):
    """island: a triangle index — its neighbours (centroids within 0.07) are left out, so that it stands alone in a hole of
    the tube and a light on either side of it reaches something"""
    rows = knot_rows()
    if island is not None:
        cen = rows[:, :9].reshape(-1, 3, 3).mean(axis=1)
        near = np.linalg.norm(cen - cen[island], axis=1) < 0.07
        near[island] = False
        rows = np.ascontiguousarray(rows[~near])
    return Built(_scene(Mesh(rows), light), tris=rows[:, :9].copy(), rows=rows)


def knot_thin(light=None):
    """thin, off-centre bounds; the ray in the mesh's space has a direction that is not unit length"""
    rows = knot_rows()
    shape = Mesh(rows).scale((1.5, 0.02, 40.0)).rotate_y(0.3).translate((3.0, 0.7, -20.0))
    tris = place(matrix(shape), rows[:, :9].reshape(-1, 3)).reshape(-1, 9)
    return Built(_scene(shape, light), tris=tris, rows=rows)


def id_normals(n):
    """n well separated unit vectors (a Fibonacci lattice on the sphere, one hemisphere: v and -v are never both used).
    A triangle whose three vertex normals are the same vector reports it as the hit's normal (mesh.rs:77), which tells
    WHICH of several coincident or nearly coincident triangles a ray hit."""
    i = np.arange(n) + 0.5
    z = i / n                                           # (0, 1): the upper hemisphere
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def bundle_rows(rs):
    """-> (rows (n, 18), bundle index of each row, the bundles' (centre, normal, e1, e2, layer heights)).  A bundle: k triangles in parallel planes, stacked along their normal with gaps from 1e-3 down to one
    ulp, each a little smaller or larger and turned in its plane (so a ray from outside meets a different one first), in
    shuffled index order; two of them exact duplicates of their neighbours below, and one a sliver (sin < 1e-5: the host
    gives it the whole grid as its box).  All their boxes contain the bundle's centre."""
    rows, which, frames = [], [], []
    for b, k in enumerate(BUNDLE_SIZES):
        ang = 2.0 * math.pi * b / len(BUNDLE_SIZES)
        c = np.array([3.0 * math.cos(ang), 0.4 + 0.1 * (b % 3), 3.0 * math.sin(ang)])
        while True:                                     # a normal off every axis and coordinate plane: boxes with volume
            n = _unit(rs.randn(3))
            if (np.abs(n) > 0.35).all():
                break
        while True:                                     # in-plane axes off every coordinate plane too (the sliver's box)
            e1 = _unit(np.cross(n, rs.randn(3)))
            e2 = np.cross(n, e1)
            if min(np.abs(e1).min(), np.abs(e2).min()) > 0.1:
                break
        gaps = 1e-3 * (4.5e-16 / 1e-3) ** (np.arange(k - 1) / max(k - 2, 1))
        h = np.concatenate([[0.0], np.cumsum(gaps)])
        h -= h[-1] / 2.0
        verts = np.zeros((k, 3, 3))
        for i in range(k):
            s, turn = rs.uniform(0.25, 0.4), rs.uniform(-0.3, 0.3)
            for j in range(3):
                a = turn + math.pi / 2.0 + j * 2.0 * math.pi / 3.0
                verts[i, j] = c + h[i] * n + s * (math.cos(a) * e1 + math.sin(a) * e2)
        dup = np.sort(rs.choice(np.arange(1, k - 1), 2, replace=False)) if k > 3 else np.array([1])
        verts[dup] = verts[dup - 1]                     # exact ties: the first in LEAF order must win
        sl = k - 1 if k == 3 else int(rs.randint(k))
        while sl in dup or sl + 1 in dup:
            sl = int(rs.randint(k))
        verts[sl] = [c + h[sl] * n - 0.3 * e1, c + h[sl] * n + 0.3 * e1, c + h[sl] * n + 0.1 * e1 + 2e-6 * e2]
        rows.append(verts[rs.permutation(k)].reshape(k, 9))     # index order is not height order
        which += [b] * k
        frames.append((c, n, e1, e2, h))
        box_lo, box_hi = verts.min(axis=1), verts.max(axis=1)
        assert (box_lo.max(axis=0) <= c).all() and (box_hi.min(axis=0) >= c).all(), k   # a common point: one leaf
    v = np.concatenate(rows)
    ids = id_normals(len(v))
    return np.concatenate([v, ids, ids, ids], axis=1), np.array(which), frames


def separate_row(n=41):
    """n small triangles in a row, none touching another: nothing straddles a median split, so the build halves them
    down to leaves of exactly 8 (the knot's own leaves, whose triangles share edges, hold 9 to 15)"""
    base = np.array([6.0, 0.2, 1.0]) + np.arange(n)[:, None] * np.array([0.25, 0.02, 0.03])
    v1, v2, v3 = base, base + [0.1, 0.05, 0.0], base + [0.0, 0.05, 0.1]
    nrm = _unit(np.cross(v2 - v1, v3 - v1))
    return np.concatenate([v1, v2, v3, nrm, nrm, nrm], axis=1)


def bundles(light=None):
    rs = np.random.RandomState(41)
    krows = knot_rows()
    brows, which, frames = bundle_rows(rs)
    rows = np.ascontiguousarray(np.concatenate([krows, brows, separate_row()]))
    return Built(_scene(Mesh(rows), light), tris=rows[:, :9].copy(), rows=rows, n_knot=len(krows), which=which, frames=frames)


def mesh_tree(rows):
    """the kd-tree the library builds over these triangles (host build: no GPU)"""
    from rpt_amd.device import kdtree_build
    v = rows[:, :9].reshape(-1, 3, 3)
    return kdtree_build(np.concatenate([v.min(axis=1), v.max(axis=1)], axis=1))


def tree_leaves(tree):
    """-> list of the leaves' reference arrays"""
    leaf = np.flatnonzero(tree["info"] == 3)
    return [tree["refs"][tree["a"][i]:tree["a"][i] + tree["b"][i]] for i in leaf]


def leaf_class_counts(tree):
    sizes = np.array([len(r) for r in tree_leaves(tree)])
    return [int(((sizes >= a) & (sizes <= b)).sum()) for a, b in LEAF_CLASSES]


def winner_positions(built, tree, o, d, t, nrm):
    """For rays that hit a bundle triangle: the position of the winning triangle in the leaf that holds the hit point
    (-1 for the other rays).  The triangle is read off the hit's normal (id_normals)."""
    ids = built.rows[built.n_knot:built.n_knot + len(built.which), 9:12]
    pos = np.full(len(t), -1)
    hit = np.isfinite(t) & np.isfinite(nrm).all(axis=1)
    idx = np.flatnonzero(hit)
    dots = np.abs(nrm[idx] @ ids.T)
    tri = dots.argmax(axis=1)
    sure = dots[np.arange(len(idx)), tri] > 1.0 - 1e-9
    idx, tri = idx[sure], tri[sure] + built.n_knot
    p = o[idx] + t[idx, None] * d[idx]
    info, split, a = tree["info"], tree["split"], tree["a"]
    where = {}
    for j, r in enumerate(tree_leaves(tree)):
        for q, g in enumerate(r):
            where.setdefault(int(g), []).append((j, q))
    leaf_of_node = {int(nd): j for j, nd in enumerate(np.flatnonzero(info == 3))}
    for i, g, pt in zip(idx, tri, p):
        node = 0
        while info[node] != 3:
            node = a[node] if pt[info[node]] < split[node] else a[node] + 1
        j = leaf_of_node[int(node)]
        cand = [q for (jj, q) in where[int(g)] if jj == j]
        pos[i] = cand[0] if cand else min(q for (_, q) in where[int(g)])
    return pos


def group_children(rs):
    """-> (shapes, kinds) of the `group` scene: spheres and cubes in a box of about 10 x 6 x 8, sizes around
    quadric_too_small's 64 grid steps, plus one cluster of 40 children around a common point (a leaf of more than 32)"""
    step = 10.0 / GRID
    kids, kinds = [], []

    def one(centre, steps):
        kind = rs.randint(3)
        if kind == 0:       # a sphere: r_min = r / sqrt(3) by the rule's Frobenius bound
            r = steps * step * math.sqrt(3.0)
            kids.append(sphere().scale((r, r, r)).translate(tuple(centre)))
        elif kind == 1:     # an ellipsoid, turned
            r = steps * step * math.sqrt(3.0)
            kids.append(sphere().scale((r, r * rs.uniform(1.0, 3.0), r * rs.uniform(1.0, 2.0))).rotate_y(rs.uniform(0, 3.0))
                        .rotate_x(rs.uniform(0, 3.0)).translate(tuple(centre)))
        else:
            e = steps * step * 2.0
            kids.append(cube().scale((e, e * rs.uniform(0.5, 2.0), e)).rotate_z(rs.uniform(0, 3.0)).rotate_y(rs.uniform(0, 3.0))
                        .translate(tuple(centre)))
        kinds.append(0 if kind < 2 else 1)

    for i in range(160):
        # near a curve through the box, so that neighbours share leaves and rays see several of them
        s = i / 159.0
        centre = np.array([-5.0 + 10.0 * s, 3.0 * math.sin(7.0 * s), 4.0 * math.cos(5.0 * s)]) + rs.randn(3) * 0.02
        one(centre, rs.uniform(30.0, 130.0))
    hub = np.array([1.0, -2.0, -3.0])
    for i in range(40):
        steps = rs.uniform(30.0, 130.0)
        one(hub + _unit(rs.randn(3)) * steps * step * 0.3, steps)
    return kids, np.array(kinds)


def too_small(m_child, qscale):
    """shape_records.h quadric_too_small for a sphere placed by the 4x4 m_child (in the group's space)"""
    inv = np.linalg.inv(m_child[:3, :3])
    r_min = 1.0 / math.sqrt((inv * inv).sum())
    return not (r_min >= 64.0 * qscale.max())


def group():
    rs = np.random.RandomState(43)
    kids, kinds = group_children(rs)
    shape = KdTree(kids).scale((1.3, 0.6, 2.0)).rotate_y(0.4).translate((0.5, 2.5, -1.0))
    g = matrix(shape)
    local = np.array([matrix(k) for k in kids])
    world = np.array([g @ m for m in local])
    b = Built(_scene(shape), spheres=world[kinds == 0], cubes=world[kinds == 1])
    # the group's own grid (mesh_records.h grid_over over the children's boxes, shape.rs:153-176) and the rule
    corners = np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
    pts = np.concatenate([place(m, corners * (1.0 if kd == 0 else 0.5)) for m, kd in zip(local, kinds)])
    b.qscale = (pts.max(axis=0) - pts.min(axis=0)) / GRID
    b.small = np.array([too_small(m, b.qscale) for m in local[kinds == 0]])
    return b


def nested():
    """a group with TREE children: the knot squashed to a sheet, a second knot, and 20 spheres"""
    rs = np.random.RandomState(47)
    rows1, rows2 = knot_rows(), scenes.knot_mesh(48, 8, seed=0x9E57)
    k1 = Mesh(rows1).scale((1e3, 1.0, 1e-3))
    k2 = Mesh(rows2).rotate_x(0.4).scale((40.0, 30.0, 25.0)).translate((100.0, 30.0, 20.0))
    # (the spheres at the far end in x: from 1e8 radii away Sphere::intersect accepts lines that miss by far, at the time of
    # the closest approach — rays that travel towards +x meet the meshes first, so that a mesh hit still wins, far_along_x)
    balls = [sphere().scale((r, r, r)).translate((rs.uniform(300.0, 480.0), rs.uniform(5.0, 30.0), rs.uniform(-20.0, 20.0)))
             for r in np.exp(rs.uniform(math.log(0.3), math.log(8.0), 20))]
    tris = np.concatenate([place(matrix(k), r[:, :9].reshape(-1, 3)).reshape(-1, 9) for k, r in ((k1, rows1), (k2, rows2))])
    return Built(_scene(KdTree([k1, k2] + balls)), tris=tris, spheres=np.array([matrix(s) for s in balls]))


SCENES = {"knot": knot, "knot_thin": knot_thin, "bundles": bundles, "group": group, "nested": nested}
_built = {}


def build(name):
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]


# ---- ray populations ------------------------------------------------------------------------------------------------
def barycentrics(rs, n, kind):
    if kind == "interior":
        return rs.dirichlet((1, 1, 1), n)
    if kind == "edge":
        a = rs.rand(n)
        bary = np.stack([a, 1.0 - a, np.zeros(n)], axis=1)
        return np.take_along_axis(bary, np.argsort(rs.rand(n, 3), axis=1), axis=1)
    return np.eye(3)[rs.randint(0, 3, n)]


def _points(bary, tris):
    return (bary[:, :, None] * tris.reshape(-1, 3, 3)).sum(axis=1)


def mesh_aimed(b, rs, n):
    """interior, edge and vertex, from 0.05, 1 and 50 units away"""
    from test_leaf_boxes import aimed_rays
    per = max(n // 9, 1)
    os_, ds = [], []
    for kind in ("interior", "edge", "vertex"):
        for dist in (0.05, 1.0, 50.0):
            tris = b.tris[rs.randint(0, len(b.tris), per)]
            o, d = aimed_rays(rs, tris, barycentrics(rs, per, kind), dist)
            os_.append(o)
            ds.append(d)
    return np.concatenate(os_), np.concatenate(ds)


def sphere_silhouette(b, rs, n):
    """rays aimed at the contour of a sphere as seen from the origin (discriminant ~ 0), scaled by 1 +- 1e-9"""
    m = b.spheres[rs.randint(0, len(b.spheres), n)]
    radius = np.linalg.norm(m[:, :3, 0], axis=1)[:, None]
    o = m[:, :3, 3] + _unit(rs.randn(n, 3)) * radius * 10.0 ** rs.uniform(0.3, 2.5, (n, 1))
    ol = np.einsum("nij,nj->ni", np.linalg.inv(m[:, :3, :3]), o - m[:, :3, 3])       # the origin in object space
    q = (ol * ol).sum(axis=1, keepdims=True)
    w = np.cross(ol, rs.randn(n, 3))
    p = ol / q + np.sqrt(np.maximum(1.0 - 1.0 / q, 0.0)) * _unit(w)                  # p . ol = 1, |p| = 1
    p *= 1.0 + rs.choice([-1e-9, 1e-9, -1e-6, 0.0], n)[:, None]
    pw = np.einsum("nij,nj->ni", m[:, :3, :3], p) + m[:, :3, 3]
    return o, _unit(pw - o)


def cube_features(b, rs, n):
    """rays aimed at corners, edges and faces of placed cubes"""
    m = b.cubes[rs.randint(0, len(b.cubes), n)]
    p = rs.choice([-0.5, 0.5], (n, 3))
    free = rs.randint(0, 3, n)                                                       # 0: a corner; 1: an edge; 2: a face
    for k in range(1, 3):
        rows = np.flatnonzero(free >= k)
        p[rows, (rs.randint(0, 3, len(rows)) + k) % 3] = rs.uniform(-0.5, 0.5, len(rows))
    pw = np.einsum("nij,nj->ni", m[:, :3, :3], p) + m[:, :3, 3]
    size = np.linalg.norm(m[:, :3, 0], axis=1)[:, None]
    o = pw + _unit(rs.randn(n, 3)) * size * 10.0 ** rs.uniform(0.0, 2.5, (n, 1))
    return o, _unit(pw - o)


def target_points(b, rs, n, feature=False):
    """points ON the scene's surfaces: of triangles (interior, or vertices if `feature`), spheres and cubes"""
    parts = []
    kinds = [k for k, have in (("tris", len(b.tris)), ("spheres", len(b.spheres)), ("cubes", len(b.cubes))) if have]
    per = n // len(kinds)
    for kind in kinds:
        if kind == "tris":
            tris = b.tris[rs.randint(0, len(b.tris), per)]
            parts.append(_points(barycentrics(rs, per, "vertex" if feature else "interior"), tris))
        elif kind == "spheres":
            m = b.spheres[rs.randint(0, len(b.spheres), per)]
            p = _unit(rs.randn(per, 3)) * (0.0 if feature else 1.0)                  # feature: the centre
            parts.append(np.einsum("nij,nj->ni", m[:, :3, :3], p) + m[:, :3, 3])
        else:
            m = b.cubes[rs.randint(0, len(b.cubes), per)]
            p = rs.choice([-0.5, 0.5], (per, 3))
            if not feature:
                p[np.arange(per), rs.randint(0, 3, per)] = rs.uniform(-0.5, 0.5, per)
                p[np.arange(per), rs.randint(0, 3, per)] = rs.uniform(-0.5, 0.5, per)
            parts.append(np.einsum("nij,nj->ni", m[:, :3, :3], p) + m[:, :3, 3])
    return np.concatenate(parts)


def near_axis(b, rs, n):
    """nearly axis-parallel: two components of about 1e-9"""
    p = target_points(b, rs, n)
    n = len(p)
    d = rs.randn(n, 3) * 1e-9
    d[np.arange(n), rs.randint(0, 3, n)] = rs.choice([-1.0, 1.0], n)
    d = _unit(d)
    ext = np.linalg.norm(b.hi - b.lo)
    return p - d * ext * 10.0 ** rs.uniform(-3.0, 1.0, (n, 1)), d


def axis_through_feature(b, rs, n):
    """exactly axis-parallel (one or two zero components) through a vertex / a corner / a centre: on the zero axes the
    origin's coordinate EQUALS the feature's"""
    p = target_points(b, rs, n, feature=True)
    n = len(p)
    d = rs.randn(n, 3)
    ax = rs.randint(0, 3, n)
    d[np.arange(n), ax] = 0.0
    two = np.flatnonzero(rs.rand(n) < 0.4)
    d[two, (ax[two] + 1) % 3] = 0.0
    d = _unit(d)
    ext = np.linalg.norm(b.hi - b.lo)
    o = p - d * ext * 10.0 ** rs.uniform(-3.0, 1.0, (n, 1))
    return np.where(d == 0.0, p, o), d


def far(b, rs, n, u_lo=0.0, u_hi=16.0, along=None):
    """interior-aimed rays from 10^u extents away -> (o, d, u); along: the directions gather around this one"""
    p = target_points(b, rs, n)
    n = len(p)
    d = _unit(rs.randn(n, 3) if along is None else rs.randn(n, 3) * 0.4 + np.asarray(along))
    u = rs.uniform(u_lo, u_hi, n)
    return p - d * (10.0 ** u * np.linalg.norm(b.hi - b.lo))[:, None], d, u


def far_pairs(per_triangle=60, seed=1):
    """the far population as (triangle, ray) PAIRS for the numpy model of tests/test_leaf_boxes.py: every triangle of the
    knot with `per_triangle` interior-aimed rays from 10^u extents away -> (tris (n, 9), o, d, u, lo, hi)"""
    from test_leaf_boxes import aimed_rays
    tris = knot_rows()[:, :9]
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    rs = np.random.RandomState(seed)
    rep = np.repeat(tris, per_triangle, axis=0)
    bary = rs.dirichlet((1, 1, 1), len(rep))
    _, d = aimed_rays(rs, rep, bary, 1.0)
    u = rs.uniform(0.0, 16.0, len(rep))
    o = _points(bary, rep) - d * (10.0 ** u * np.linalg.norm(hi - lo))[:, None]
    return rep, o, d, u, lo, hi


def bundle_pairs():
    """every other ray through the bundles, paired with every triangle of the bundle it is aimed at
    -> (tris (n, 9), o, d, lo, hi) with the bounds of the whole mesh"""
    b = build("bundles")
    o, d, k = (a[::2] for a in population("bundles", "through"))
    first = np.concatenate([[0], np.cumsum(BUNDLE_SIZES)]) + b.n_knot
    ray = np.concatenate([np.repeat(np.flatnonzero(k == j), size) for j, size in enumerate(BUNDLE_SIZES)])
    tri = np.concatenate([np.tile(np.arange(first[j], first[j] + size), int((k == j).sum())) for j, size in enumerate(BUNDLE_SIZES)])
    return b.tris[tri], o[ray], d[ray], b.tris.reshape(-1, 3).min(axis=0), b.tris.reshape(-1, 3).max(axis=0)


def far_along_x(b, rs, n):
    return far(b, rs, n, along=(1.5, 0.0, 0.0))


def far_group(b, rs, n):
    """the group's far population: 10^u extents with u in [-1, 4.5] crosses the quadric filter's 1e7-step limit"""
    return far(b, rs, n, -1.0, 4.5)


def through_bundles(b, rs, n):
    """rays along a bundle's normal and at 80 degrees to it, either way, aimed at random points of the stack — from
    outside it and from between its layers — plus a few at each bundle's sliver and its duplicates"""
    k = rs.randint(0, len(b.frames), n)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    first = np.concatenate([[0], np.cumsum(BUNDLE_SIZES)])
    btris = b.tris[b.n_knot:b.n_knot + len(b.which)].reshape(-1, 3, 3)
    for i in range(n):
        c, nrm, e1, e2, h = b.frames[k[i]]
        size = BUNDLE_SIZES[k[i]]
        mode = i % 8
        layer = rs.randint(size)
        if mode == 7:       # a triangle's own centroid (slivers and duplicates included), straight on
            p = btris[first[k[i]] + layer].mean(axis=0)
        else:
            ang = rs.uniform(0.0, 2.0 * math.pi)
            p = c + rs.uniform(0.0, 0.12) * (math.cos(ang) * e1 + math.sin(ang) * e2) + h[layer] * nrm
        tilt = 0.0 if mode % 2 == 0 else math.radians(80.0)
        ang = rs.uniform(0.0, 2.0 * math.pi)
        dirn = rs.choice([-1.0, 1.0]) * (math.cos(tilt) * nrm + math.sin(tilt) * (math.cos(ang) * e1 + math.sin(ang) * e2))
        if mode < 4 or mode == 7:   # from outside the stack
            back = rs.uniform(0.5, 3.0)
        else:                        # from between the layers: half a gap before the aimed layer, whichever way the ray goes
            j = layer - 1 if (dirn @ nrm) > 0 else layer + 1
            gap = abs(h[layer] - h[j]) if 0 <= j < size else 1e-3
            back = 0.5 * gap / max(abs(dirn @ nrm), 1e-3)
        o[i], d[i] = p - back * dirn, dirn
    return o, d, k


POPULATIONS = {
    # scene -> {population: (builder, rays)}
    "knot": {"aimed": (mesh_aimed, 90000), "near_axis": (near_axis, 60000), "axis_vertex": (axis_through_feature, 60000),
             "far": (far, 120000)},
    "knot_thin": {"aimed": (mesh_aimed, 90000), "near_axis": (near_axis, 60000), "axis_vertex": (axis_through_feature, 60000),
                  "far": (far, 120000)},
    "bundles": {"through": (through_bundles, 40000), "aimed": (mesh_aimed, 90000)},
    "group": {"silhouette": (sphere_silhouette, 80000), "cube_features": (cube_features, 80000), "near_axis": (near_axis, 60000),
              "axis_vertex": (axis_through_feature, 60000), "far": (far_group, 120000)},
    "nested": {"aimed": (mesh_aimed, 90000), "silhouette": (sphere_silhouette, 60000), "near_axis": (near_axis, 60000),
               "far": (far_along_x, 120000)},
}
PAIRS = [(s, p) for s in POPULATIONS for p in POPULATIONS[s]]
_rays = {}


def population(scene, name):
    """-> (o, d, tag): tag is log10 of the distance in extents for the far populations, the bundle aimed at for the
    rays through the bundles, else None"""
    key = (scene, name)
    if key not in _rays:
        fn, n = POPULATIONS[scene][name]
        rs = np.random.RandomState(1000 + 37 * sorted(SCENES).index(scene) + sorted(POPULATIONS[scene]).index(name))
        out = fn(build(scene), rs, n)
        _rays[key] = (out[0], out[1], out[2] if len(out) > 2 else None)
        assert len(out[0]) <= 200000 and np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    return _rays[key]
