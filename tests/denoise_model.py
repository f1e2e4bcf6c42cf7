"""rptgpu_buffer_denoise restated in numpy from the contract in include/rpt_gpu.h alone.  Test helper, not a test.

Every operation is element-wise over the frame (IEEE f64, one rounding each, never contracted) and the TAPS are walked by
plain Python loops in the contract's order — dx outer, dy inner, ascending — so every running sum adds in the order the
contract fixes; no np.sum anywhere (its pairwise order differs).  A skipped tap adds nothing: the sums are updated through
np.where, never by adding a zero weight (0 * NaN would be NaN).  exp is include/rpt_math.h's, through the oracle."""
import numpy as np

from oracle import oracle_ffi as O

DEFAULTS = dict(levels=3, sigma_color=2.0, sigma_normal=0.1, sigma_depth=0.01, sigma_albedo=0.1)
K = {-2: 0.0625, -1: 0.25, 0: 0.375, 1: 0.25, 2: 0.0625}
G = {-1: 0.25, 0: 0.5, 1: 0.25}
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rpt_exp(x):
    """rpt_exp of include/rpt_math.h (oracle_math_eval fn 0), any shape"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return O.math_eval(0, x.reshape(-1)).reshape(x.shape)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def regions(h, w, ox, oy):
    """the pixels p whose tap q = p + (ox, oy) lies in the frame, and those taps: two (rows, columns) slice pairs, or
    None when there is no such pixel"""
    x0, x1 = max(0, -ox), min(w, w - ox)
    y0, y1 = max(0, -oy), min(h, h - oy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def welford(frames, counts=None):
    """The buffer's per-pixel state from its batches: frames[k] (H, W, 3) is batch k for every pixel and pixel p holds
    the first counts[p] of them (default: all).  -> total (H, W, 3), counts (H, W), M2 (H, W)"""
    h, w = frames[0].shape[:2]
    counts = np.full((h, w), len(frames), dtype=np.int64) if counts is None else np.asarray(counts).reshape(h, w).astype(np.int64)
    total, m, M2 = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
    with np.errstate(all="ignore"):
        for k, F in enumerate(frames):
            sel = counts > k
            x = np.asarray(F, dtype=np.float64).reshape(h, w, 3)
            d = x - m
            m1 = m + d / np.float64(k + 1)
            total = np.where(sel[..., None], total + x, total)
            M2 = np.where(sel, M2 + dot(d, x - m1), M2)
            m = np.where(sel[..., None], m1, m)
    return total, counts, M2


def inputs(total, counts, M2, feats):
    """the contract's inputs per pixel -> c, v (prefiltered), hit, N, P, Z, A"""
    h, w = counts.shape
    with np.errstate(all="ignore"):
        n = counts.astype(np.float64)
        c = total / n[..., None]
        u = (M2 / (n - 1.0)) / n
        a, s = np.zeros((h, w)), np.zeros((h, w))
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                r = regions(h, w, dx, dy)
                if r is None:
                    continue
                p, q = r
                g = G[dx] * G[dy]
                a[p] = a[p] + g * u[q]
                s[p] = s[p] + g
        v = a / s
        hits = np.asarray(feats["hits"]).reshape(h, w)
        hit = hits > 0
        hd = np.where(hit, hits, 1).astype(np.float64)
        N = np.where(hit[..., None], np.asarray(feats["normal"]).reshape(h, w, 3) / hd[..., None], 0.0)
        P = np.where(hit[..., None], np.asarray(feats["position"]).reshape(h, w, 3) / hd[..., None], 0.0)
        A = np.where(hit[..., None], np.asarray(feats["albedo"]).reshape(h, w, 3) / hd[..., None], 0.0)
        Z = np.where(hit, np.asarray(feats["depth"]).reshape(h, w) / hd, 0.0)
    return c, v, hit, N, P, Z, A


def level(c, v, hit, N, P, Z, A, step, sigma_color, sigma_normal, sigma_depth, sigma_albedo, exp=rpt_exp, weights=None):
    """one a-trous pass -> (c', v').  weights: a list that receives (dx, dy, w, used) per tap, for the tests of the model"""
    h, w = v.shape
    C, W, V = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    with np.errstate(all="ignore"):
        for dx in range(-2, 3):
            for dy in range(-2, 3):
                r = regions(h, w, dx * step, dy * step)
                if r is None:
                    continue
                p, q = r
                w0 = K[dx] * K[dy]
                cq, vq = c[q], v[q]
                if dx == 0 and dy == 0:
                    wt = np.full(vq.shape, w0)
                    ok = np.ones(vq.shape, dtype=bool)
                else:
                    d = cq - c[p]
                    e = dot(d, d) / (sigma_color * sigma_color * (v[p] + vq) + 1e-12)
                    t = 1.0 - dot(N[p], N[q])
                    en = np.where(t > 0.0, t, 0.0) / sigma_normal
                    ez = np.abs(dot(N[p], P[q] - P[p])) / (sigma_depth * Z[p] + 1e-12)
                    D = A[q] - A[p]
                    ea = dot(D, D) / (sigma_albedo * sigma_albedo)
                    e = np.where(hit[p], e + ((en + ez) + ea), e)
                    ok = (hit[p] == hit[q]) & (e >= 0.0) & (e < INF)
                    wt = w0 * exp(-np.where(ok, e, 0.0))
                if weights is not None:
                    weights.append((dx, dy, p, wt, ok))
                C[p] = np.where(ok[..., None], C[p] + wt[..., None] * cq, C[p])
                W[p] = np.where(ok, W[p] + wt, W[p])
                V[p] = np.where(ok, V[p] + (wt * wt) * vq, V[p])
        return C / W[..., None], V / (W * W)


def denoise(total, counts, M2, feats, levels=3, sigma_color=2.0, sigma_normal=0.1, sigma_depth=0.01, sigma_albedo=0.1,
            exp=rpt_exp):
    """out_linear of rptgpu_buffer_denoise -> (H, W, 3)"""
    c, v, hit, N, P, Z, A = inputs(total, counts, M2, feats)
    for l in range(levels):
        c, v = level(c, v, hit, N, P, Z, A, 1 << l, sigma_color, sigma_normal, sigma_depth, sigma_albedo, exp)
    return c
