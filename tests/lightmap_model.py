"""The contract of include/rpt_gpu_lightmap.h restated in numpy f64, from the header's text: texel space, the edge function,
coverage, the owner rule, barycentrics, the gather point and the normal, and the dilation.  Every expression is a chain of
separate ufunc calls in the header's order (no einsum, no dot: nothing fuses or reorders).  A helper, not a test:
tests/test_lightmap_host.py holds it to closed forms without a GPU, tests/test_gpu_lightmap.py holds the kernels to it."""
import numpy as np

import aov_model

bits = aov_model.bits


def same(a, b):
    """the raw bits: -0.0 != +0.0, a NaN equals the same NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def edge(px, py, qx, qy, cx, cy):
    """e(P, Q, c) = (Q.x - P.x) * (c.y - P.y) - (Q.y - P.y) * (c.x - P.x)"""
    return (qx - px) * (cy - py) - (qy - py) * (cx - px)


def centres(width, height):
    """-> (cx, cy), each (H, W): texel (x, y)'s centre (x + 0.5, y + 0.5)"""
    cx = np.broadcast_to(np.arange(width, dtype=np.float64) + 0.5, (height, width))
    cy = np.broadcast_to((np.arange(height, dtype=np.float64) + 0.5)[:, None], (height, width))
    return cx, cy


def coverage(uvs, width, height):
    """-> (covers (n, H, W) bool, e (n, 3, H, W), area (n,)): which texel centres each triangle covers, and e1, e2, e3 there"""
    uvs = np.asarray(uvs, dtype=np.float64).reshape(-1, 3, 2)
    n = len(uvs)
    cx, cy = centres(width, height)
    covers = np.zeros((n, height, width), dtype=bool)
    e = np.zeros((n, 3, height, width))
    area = np.zeros(n)
    with np.errstate(all="ignore"):
        ax = uvs[:, :, 0] * float(width)
        ay = uvs[:, :, 1] * float(height)
        for j in range(n):
            (x1, x2, x3), (y1, y2, y3) = ax[j], ay[j]
            area[j] = edge(x1, y1, x2, y2, x3, y3)
            e[j, 0] = edge(x2, y2, x3, y3, cx, cy)
            e[j, 1] = edge(x3, y3, x1, y1, cx, cy)
            e[j, 2] = edge(x1, y1, x2, y2, cx, cy)
            if not (np.isfinite(ax[j]).all() and np.isfinite(ay[j]).all() and np.isfinite(area[j])) or area[j] == 0.0:
                continue
            if area[j] > 0.0:
                covers[j] = (e[j, 0] >= 0.0) & (e[j, 1] >= 0.0) & (e[j, 2] >= 0.0)
            else:
                covers[j] = (e[j, 0] <= 0.0) & (e[j, 1] <= 0.0) & (e[j, 2] <= 0.0)
    return covers, e, area


def raster(uvs, width, height):
    """-> (owner (H, W) int32: the lowest covering index or -1, barycentric (H, W, 3): e / area of the owner, +0.0 unowned)"""
    covers, e, area = coverage(uvs, width, height)
    owner = np.full((height, width), -1, dtype=np.int32)
    bary = np.zeros((height, width, 3))
    for j in range(len(covers) - 1, -1, -1):  # the lowest index is written last
        m = covers[j]
        owner[m] = j
        with np.errstate(all="ignore"):
            for k in range(3):
                bary[m, k] = (e[j, k] / area[j])[m]
    return owner, bary


def cross(a, b):
    """Triangle::from_vertices' (mesh.rs:27) cross product"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def surface(owner, bary, positions, normals, offset):
    """-> (G (H, W, 3), n (H, W, 3)) of the owned texels, +0.0 elsewhere"""
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3, 3)
    g = np.zeros(owner.shape + (3,))
    nrm = np.zeros(owner.shape + (3,))
    m = owner >= 0
    if not m.any():
        return g, nrm
    o = owner[m]
    b1, b2, b3 = (bary[m][:, k, None] for k in range(3))
    p = positions[o]
    with np.errstate(all="ignore"):
        pos = (b1 * p[:, 0] + b2 * p[:, 1]) + b3 * p[:, 2]
        if normals is not None:
            q = np.asarray(normals, dtype=np.float64).reshape(-1, 3, 3)[o]
            mm = (b1 * q[:, 0] + b2 * q[:, 1]) + b3 * q[:, 2]
        else:
            mm = cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        length = np.sqrt((mm[:, 0] * mm[:, 0] + mm[:, 1] * mm[:, 1]) + mm[:, 2] * mm[:, 2])
        unit = mm / length[:, None]
        g[m] = pos + float(offset) * unit
        nrm[m] = unit
    return g, nrm


def raw(positions, normals, uvs, width, height, offset=0.0):
    """the four raw channels of a call -> {"owner", "barycentric", "position", "normal"}"""
    owner, bary = raster(uvs, width, height)
    g, nrm = surface(owner, bary, positions, normals, offset)
    return {"owner": owner, "barycentric": bary, "position": g, "normal": nrm}


def dilate(values, filled, rounds):
    """`rounds` rounds over values (H, W) or (H, W, C) with filled (H, W) bool -> (values, filled) afterwards.  A round reads
    the previous round's state only: an unfilled texel with filled neighbours takes acc / count, acc from +0.0 in the order
    dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner)"""
    values = np.array(values, dtype=np.float64)
    filled = np.array(filled, dtype=bool)
    flat = values.ndim == 2
    if flat:
        values = values[:, :, None]
    h, w = filled.shape
    for _ in range(int(rounds)):
        acc = np.zeros_like(values)
        count = np.zeros((h, w), dtype=np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nf = np.zeros((h, w), dtype=bool)       # is the neighbour at (x + dx, y + dy) in the map and filled?
                nv = np.zeros_like(values)
                ys, yd = (slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0)))
                xs, xd = (slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0)))
                nf[yd, xd] = filled[ys, xs]
                nv[yd, xd] = values[ys, xs]
                acc = np.where(nf[:, :, None], acc + nv, acc)
                count = count + nf
        take = ~filled & (count > 0)
        with np.errstate(all="ignore"):
            mean = acc / count.astype(np.float64)[:, :, None]
        values = np.where(take[:, :, None], mean, values)
        filled = filled | take
    return (values[:, :, 0] if flat else values), filled
