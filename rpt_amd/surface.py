"""What a caller does next with GpuScene.hit_surface's `primitive` and `barycentric`: interpolate a per-vertex attribute
at the hits (include/rpt_gpu_hit_surface.h).  numpy only."""
import numpy as np


def interpolate(values, primitive, barycentric):
    """values: (n_tris, 3, k) — attribute vectors a1, a2, a3 of every triangle's v1, v2, v3, in the mesh's triangle order
    (what hit_surface's `primitive` counts in); a (n_tris, 3) array is k = 1 without the last axis.  primitive: (n,) ints,
    barycentric: (n, 3) (u, v, w).  Returns (n, k) — or (n,) — float64: u*a1 + v*a2 + w*a3 where primitive >= 0, in that
    order of operations (Triangle::intersect's for the normal, mesh.rs:74), and 0 elsewhere."""
    values = np.asarray(values, dtype=np.float64)
    primitive = np.asarray(primitive)
    barycentric = np.asarray(barycentric, dtype=np.float64)
    if values.ndim not in (2, 3) or values.shape[1] != 3:
        raise ValueError("interpolate: values must be an (n_tris, 3, k) or (n_tris, 3) array")
    if primitive.ndim != 1 or primitive.dtype.kind not in "iu":
        raise ValueError("interpolate: primitive must be an (n,) integer array")
    if barycentric.shape != (len(primitive), 3):
        raise ValueError("interpolate: barycentric must be an (n, 3) array, one row per primitive")
    hit = primitive >= 0
    if hit.any() and int(primitive.max()) >= len(values):
        raise ValueError("interpolate: primitive %d of a mesh of %d triangles" % (int(primitive.max()), len(values)))
    scalar = values.ndim == 2
    v = values[:, :, None] if scalar else values
    out = np.zeros((len(primitive), v.shape[2]))
    a = v[primitive[hit]]
    b = barycentric[hit]
    out[hit] = b[:, 0, None] * a[:, 0] + b[:, 1, None] * a[:, 1] + b[:, 2, None] * a[:, 2]
    return out[:, 0] if scalar else out
