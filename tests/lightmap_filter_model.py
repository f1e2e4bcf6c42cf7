"""rptgpu_filter_lightmap restated in numpy from the contract in include/rpt_gpu_lightmap_filter.h alone.  Test helper, not a
test.

Every operation is element-wise over the map (IEEE f64, one rounding each, never contracted) and the TAPS are walked by plain
Python loops in the contract's order — dx outer, dy inner, ascending — so every running sum adds in the order the contract
fixes; no np.sum anywhere.  A skipped tap adds nothing: the sums are updated through np.where, never by adding a zero weight
(0 * NaN would be NaN).  exp is include/rpt_math.h's, through the oracle; the dilation is lightmap_model's."""
import numpy as np

from oracle import oracle_ffi as O

import lightmap_model

K = {-2: 0.0625, -1: 0.25, 0: 0.375, 1: 0.25, 2: 0.0625}
G = {-1: 0.25, 0: 0.5, 1: 0.25}
INF = float("inf")


def rpt_exp(x):
    """rpt_exp of include/rpt_math.h (oracle_math_eval fn 0), any shape"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return O.math_eval(0, x.reshape(-1)).reshape(x.shape)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm2(d):
    """|d|^2: dot(d, d) for 3 words, d * d for 1 (d: (..., words))"""
    return dot(d, d) if d.shape[-1] == 3 else d[..., 0] * d[..., 0]


def regions(h, w, ox, oy):
    """the texels p whose tap q = p + (ox, oy) lies in the map, and those taps: two (rows, columns) slice pairs, or None
    when there is no such texel"""
    x0, x1 = max(0, -ox), min(w, w - ox)
    y0, y1 = max(0, -oy), min(h, h - oy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def prefilter(variance, valid):
    """v: the 3 x 3 prefilter over the valid neighbours for a valid texel, variance_p for any other"""
    h, w = valid.shape
    a, s = np.zeros((h, w)), np.zeros((h, w))
    with np.errstate(all="ignore"):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                r = regions(h, w, dx, dy)
                if r is None:
                    continue
                p, q = r
                g = G[dx] * G[dy]
                ok = valid[q]
                a[p] = np.where(ok, a[p] + g * variance[q], a[p])
                s[p] = np.where(ok, s[p] + g, s[p])
        return np.where(valid, a / s, variance)


def level(c, v, valid, N, P, step, sigma_normal, sigma_plane, sigma_distance, sigma_color, exp=rpt_exp):
    """one a-trous pass -> (c', v').  c: (H, W, words); v: (H, W) or None"""
    h, w = valid.shape
    C, W = np.zeros(c.shape), np.zeros((h, w))
    V = np.zeros((h, w)) if v is not None else None
    sd = sigma_distance * float(step)
    with np.errstate(all="ignore"):
        for dx in range(-2, 3):
            for dy in range(-2, 3):
                r = regions(h, w, dx * step, dy * step)
                if r is None:
                    continue
                p, q = r
                w0 = K[dx] * K[dy]
                cq = c[q]
                ok = valid[q]
                if dx == 0 and dy == 0:
                    wt = np.full(ok.shape, w0)
                else:
                    ok = ok & (np.abs(cq) < INF).all(axis=-1)
                    D = P[q] - P[p]
                    t = 1.0 - dot(N[p], N[q])
                    en = np.where(t > 0.0, t, 0.0) / sigma_normal
                    ez = np.abs(dot(N[p], D)) / sigma_plane
                    ed = dot(D, D) / (sd * sd)
                    e = (en + ez) + ed
                    if v is not None:
                        d = cq - c[p]
                        e = e + norm2(d) / ((sigma_color * sigma_color) * (v[p] + v[q]) + 1e-12)
                    ok = ok & (e >= 0.0) & (e < INF)
                    wt = w0 * exp(-np.where(ok, e, 0.0))
                C[p] = np.where(ok[..., None], C[p] + wt[..., None] * cq, C[p])
                W[p] = np.where(ok, W[p] + wt, W[p])
                if v is not None:
                    V[p] = np.where(ok, V[p] + (wt * wt) * v[q], V[p])
        c1 = np.where(valid[..., None], C / W[..., None], c)
        v1 = np.where(valid, V / (W * W), v) if v is not None else None
    return c1, v1


def filter_lightmap(values, owner, position, normal, *, sigma_distance, sigma_plane, sigma_normal=0.1, levels=3, variance=None,
                    sigma_color=2.0, dilate=0, exp=rpt_exp):
    """out of rptgpu_filter_lightmap, shaped like values ((H, W) or (H, W, 3)) — or (out, out_variance) with a variance"""
    values = np.asarray(values, dtype=np.float64)
    flat = values.ndim == 2
    c = values[..., None] if flat else values
    valid = np.asarray(owner) >= 0
    h, w = valid.shape
    P, N = np.asarray(position, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    v = prefilter(np.asarray(variance, dtype=np.float64), valid) if variance is not None else None
    for l in range(int(levels)):
        c, v = level(c, v, valid, N, P, 1 << l, sigma_normal, sigma_plane, sigma_distance, sigma_color, exp)
    out, _ = lightmap_model.dilate(c, valid, min(int(dilate), max(w, h)))
    out = out[..., 0] if flat else out
    return (out, v) if variance is not None else out
