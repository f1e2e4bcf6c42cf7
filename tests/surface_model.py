"""What tests/test_gpu_hit_surface.py and tests/test_hit_surface_host.py share: Triangle::intersect (mesh.rs:50-73) restated in
numpy f64 in the operation order the library's records use (rpt_amd/csrc/mesh_records.h fill_trix, kernels/shapes.inc tri_plane /
tri_bary), the host mirror's Transformed arithmetic (rpt_amd/glm.py's matrices, nalgebra's sums), and what the Python scene says
about the shape behind an (object, child) pair.  A helper, not a test.

The restatement is a YARDSTICK for rptgpu_hit_surface: given the triangle a ray is said to have hit, it must reproduce the
record rptgpu_closest_hit returned — time and shading normal, bit for bit — with all three weights >= 0.  It is itself held to
the oracle without a GPU (test_hit_surface_host.py)."""
import functools

import numpy as np

from rpt_amd import shape as S

import aov_model
import test_gpu_occlusion as occ

bits = aov_model.bits
N_RAYS = occ.N_RAYS


def same(a, b):
    """the raw bits: -0.0 != +0.0, a NaN equals the same NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def box_rays(name):
    """test_gpu_occlusion.rays' origins and directions for a scene without special rows, made without a GPU: the same
    generator, the same two draws (the GPU test holds them equal)"""
    assert name != "monomial"
    rs = np.random.RandomState(sum(map(ord, name)) + 1)
    lo, hi = occ.BOXES[name]
    o = rs.uniform(lo, hi, (N_RAYS, 3))
    d = rs.standard_normal((N_RAYS, 3)) * rs.uniform(0.25, 4.0, (N_RAYS, 1))
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def d3(a, b):
    """nalgebra's 3-vector dot: the products summed left to right"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(a):
    with np.errstate(all="ignore"):
        return a / np.sqrt(d3(a, a))[..., None]


def tri_records(rows, o, d):
    """Triangle::intersect for row k of `rows` ((n, 18): v1 v2 v3 n1 n2 n3) and ray k, in the mesh's space ->
    (time, (u, v, w) as an (n, 3) array, the normalised interpolated normal).  fill_trix's precomputed values, then
    tri_plane and tri_bary, operation for operation."""
    rows = np.asarray(rows, dtype=np.float64)
    v1, v2, v3, n1, n2, n3 = (rows[:, 3 * k:3 * k + 3] for k in range(6))
    with np.errstate(all="ignore"):
        d0, d1 = v2 - v1, v3 - v1
        c = np.stack([d0[:, 1] * d1[:, 2] - d0[:, 2] * d1[:, 1], d0[:, 2] * d1[:, 0] - d0[:, 0] * d1[:, 2],
                      d0[:, 0] * d1[:, 1] - d0[:, 1] * d1[:, 0]], axis=1)
        pn = c / np.sqrt(d3(c, c))[:, None]
        d00, d01, d11 = d3(d0, d0), d3(d0, d1), d3(d1, d1)
        denom = d00 * d11 - d01 * d01
        cosine = d3(pn, d)
        time = d3(pn, v1 - o) / cosine
        p2 = (o + time[:, None] * d) - v1
        d20, d21 = d3(p2, d0), d3(p2, d1)
        v = (d11 * d20 - d01 * d21) / denom
        w = (d00 * d21 - d01 * d20) / denom
        u = 1.0 - v - w
        nrm = normalize(u[:, None] * n1 + v[:, None] * n2 + w[:, None] * n3)
    return time, np.stack([u, v, w], axis=1), nrm


def local_rays(xf, o, d):
    """Ray::apply_transform (shape.rs:64-71) with the host mirror's inverse_transform (column-major), nalgebra's sums: what
    the library computes from the matrices the mirror hands it"""
    m = np.asarray(xf.inverse_transform, dtype=np.float64)
    lo = np.stack([((m[r] * o[:, 0] + m[4 + r] * o[:, 1]) + m[8 + r] * o[:, 2]) + m[12 + r] * 1.0 for r in range(3)], axis=1)
    ld = np.stack([((m[r] * d[:, 0] + m[4 + r] * d[:, 1]) + m[8 + r] * d[:, 2]) + m[12 + r] * 0.0 for r in range(3)], axis=1)
    return lo, ld


def world_normals(xf, n):
    """shape.rs:131-132: normalize(normal_transform * n), the mirror's matrix (column-major 3 x 3)"""
    m = np.asarray(xf.normal_transform, dtype=np.float64)
    return normalize(np.stack([(m[r] * n[:, 0] + m[3 + r] * n[:, 1]) + m[6 + r] * n[:, 2] for r in range(3)], axis=1))


def unwrap(shape):
    """-> (the Transformed wrapper or None, the shape inside)"""
    return (shape, shape.shape) if isinstance(shape, S.Transformed) else (None, shape)


def is_mesh(core):
    return isinstance(core, S.KdTree) and core.triangles is not None


def is_group(core):
    return isinstance(core, S.KdTree) and core.triangles is None


def contains_triangles(shape):
    core = unwrap(shape)[1]
    return is_mesh(core) or (is_group(core) and any(contains_triangles(k) for k in core.objects))


def hit_shape(scene, obj, child):
    """what the scene says stands behind (object, child): -> (the chain of Transformed wrappers outermost first — None
    where a level has none —, the innermost shape named: a mesh, another group, or a primitive)"""
    outer, core = unwrap(scene.objects[obj].shape)
    if not is_group(core):
        return [outer], core
    inner, kid = unwrap(core.objects[child])
    return [outer, inner], kid


def restate(scene, o, d, obj, child, primitive):
    """Triangle::intersect for every ray with primitive >= 0 whose mesh is the hit object or a direct child of it ->
    (the rays' indices, whether the ray reaches the mesh's space untransformed, time, (u, v, w), the world-space normal)"""
    idx, plain, time, bary, nrm = [], [], [], [], []
    for i in np.flatnonzero(primitive >= 0):
        chain, mesh = hit_shape(scene, int(obj[i]), int(child[i]))
        if not is_mesh(mesh):
            continue  # (a mesh nested deeper: PRIMITIVE names the innermost triangle, CHILD only the first level)
        lo, ld = o[i:i + 1], d[i:i + 1]
        for xf in chain:
            if xf is not None:
                lo, ld = local_rays(xf, lo, ld)
        t, b, n = tri_records(mesh.triangles[int(primitive[i])][None, :], lo, ld)
        for xf in reversed(chain):
            if xf is not None:
                n = world_normals(xf, n)
        idx.append(i)
        plain.append(all(xf is None for xf in chain))
        time.append(t[0]); bary.append(b[0]); nrm.append(n[0])
    if not idx:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3))
    return np.array(idx), np.array(plain), np.array(time), np.array(bary), np.array(nrm)


def meshes_of(scene):
    """every mesh that is a top-level object or a direct child of a top-level group: (object, child or -1, chain, mesh)"""
    out = []
    for i, ob in enumerate(scene.objects):
        outer, core = unwrap(ob.shape)
        if is_mesh(core):
            out.append((i, -1, [outer], core))
        elif is_group(core):
            for k, kid in enumerate(core.objects):
                inner, shape = unwrap(kid)
                if is_mesh(shape):
                    out.append((i, k, [outer, inner], shape))
    return out


def aimed_rays(scene, box, seed, n=N_RAYS):
    """n rays from inside `box` towards random points of random triangles of the scene's meshes (meshes_of), their
    directions no unit vectors: the box rays of the scenes whose meshes are small seldom land on a triangle, these mostly do"""
    rs = np.random.RandomState(seed)
    found = meshes_of(scene)
    lo, hi = box
    o = rs.uniform(lo, hi, (n, 3))
    d = np.empty((n, 3))
    for i in range(n):
        _, _, chain, mesh = found[rs.randint(len(found))]
        row = mesh.triangles[rs.randint(len(mesh.triangles))]
        w = rs.dirichlet((1.0, 1.0, 1.0))
        p = w[0] * row[0:3] + w[1] * row[3:6] + w[2] * row[6:9]
        for xf in reversed(chain):  # the innermost placement first
            if xf is not None:
                m = np.asarray(xf.transform_m, dtype=np.float64).reshape(4, 4).T
                p = (m @ np.append(p, 1.0))[:3]
        d[i] = (p - o[i]) * rs.uniform(0.25, 4.0)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d
