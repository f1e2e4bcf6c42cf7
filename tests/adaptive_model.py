"""The adaptive device Buffer restated in numpy: per-pixel Welford statistics over the batch values, the
stopping rule, and buffer.rs:59-93 with per-pixel sample lists.  IEEE f64, the C ABI's order of operations."""
import numpy as np


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def stays_active(n, m, M2, min_batches, abs_tol, rel_tol):
    nn = n.astype(np.float64)
    with np.errstate(all="ignore"):
        e = (M2 / (nn - 1.0)) / nn
        t = abs_tol + rel_tol * ((m[:, 0] + m[:, 1]) + m[:, 2])
        return ~((n >= min_batches) & (e <= t * t))


def run(frames, min_batches, abs_tol, rel_tol):
    """frames[k]: (P, 3) batch values of round k for EVERY pixel (a plain full-frame render at that round's base).
    -> dict(counts, mean, M2, active (list of active counts after each round), totals, last_e)"""
    P = len(frames[0])
    n = np.zeros(P, dtype=np.int64)
    m = np.zeros((P, 3))
    M2 = np.zeros(P)
    total = np.zeros((P, 3))
    active = np.ones(P, dtype=bool)
    left = []
    for F in frames:
        idx = np.nonzero(active)[0]
        if len(idx):
            x = F[idx]
            total[idx] = total[idx] + x
            n[idx] += 1
            d = x - m[idx]
            m[idx] = m[idx] + d / n[idx].astype(np.float64)[:, None]
            M2[idx] = M2[idx] + dot(d, x - m[idx])
            keep = stays_active(n[idx], m[idx], M2[idx], min_batches, abs_tol, rel_tol)
            active[idx[~keep]] = False
        left.append(int(active.sum()))
    return dict(counts=n, mean=m, M2=M2, active=left, totals=total)


def masked_totals(frames, counts):
    """sum_{k < n_p} F_k[p], in round order"""
    total = np.zeros_like(frames[0])
    for k, F in enumerate(frames):
        sel = counts > k
        total[sel] = total[sel] + F[sel]
    return total


def pixel_lists(frames, counts):
    """per pixel, its samples as Python tuples: samples[index] of the reference's Buffer"""
    return [[tuple(float(v) for v in frames[k][p]) for k in range(int(counts[p]))] for p in range(len(counts))]


def ref_filtered(pix, w, h, radius):
    """get_filtered_color (buffer.rs:75-93), pixel by pixel in Python floats"""
    out = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            color = [0.0, 0.0, 0.0]
            count = 0
            for i in range(max(0, x - radius), x + radius + 1):
                for j in range(max(0, y - radius), y + radius + 1):
                    if i < w and j < h:
                        s = [0.0, 0.0, 0.0]
                        for c in pix[j * w + i]:
                            s = [s[0] + c[0], s[1] + c[1], s[2] + c[2]]
                        color = [color[0] + s[0], color[1] + s[1], color[2] + s[2]]
                        count += len(pix[j * w + i])
            assert count != 0, "Pixel found with no samples"
            out[y, x] = [color[0] / count, color[1] / count, color[2] / count]
    return out


def ref_variance(pix):
    """Buffer::variance (buffer.rs:59-73) in Python floats"""
    variance, count = 0.0, 0.0
    for samples in pix:
        s = [0.0, 0.0, 0.0]
        for c in samples:
            s = [s[0] + c[0], s[1] + c[1], s[2] + c[2]]
        n = float(len(samples))
        mean = [v / n if n else float("nan") for v in s]
        ss = 0.0
        for c in samples:
            d = [c[0] - mean[0], c[1] - mean[1], c[2] - mean[2]]
            ss += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        variance += ss / (n - 1.0) if n != 1.0 else float("nan")
        count += 1.0
    return variance / count
