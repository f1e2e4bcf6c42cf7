"""The adaptive device Buffer restated in numpy: per-pixel Welford statistics over the batch values, the
stopping rule, and buffer.rs:59-93 with per-pixel sample lists.  IEEE f64, the C ABI's order of operations."""
import numpy as np

from rpt_amd.color import color_bytes


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


def filtered_color(totals, counts, w, h, radius):
    """get_filtered_color (buffer.rs:75-93) for every pixel at once: totals (w*h, 3) the per-pixel sample sums, counts
    (w*h,) their lengths -> (h, w, 3).  Per pixel the neighbours are added in the reference's order, column i outer and
    row j inner.  The frame is padded with zeros, so an out-of-frame neighbour adds +0.0: the running sum starts at +0.0
    and can never become -0.0, hence x + 0.0 == x and the padding changes no bit.  Offsets beyond the frame only ever
    reach the padding and are left out."""
    tot = np.asarray(totals, dtype=np.float64).reshape(h, w, 3)
    cnt = np.asarray(counts, dtype=np.int64).reshape(h, w)
    rx, ry = min(radius, w - 1), min(radius, h - 1)
    tp = np.zeros((h + 2 * ry, w + 2 * rx, 3))
    tp[ry:ry + h, rx:rx + w] = tot
    cp = np.zeros((h + 2 * ry, w + 2 * rx), dtype=np.int64)
    cp[ry:ry + h, rx:rx + w] = cnt
    color = np.zeros((h, w, 3))
    count = np.zeros((h, w), dtype=np.int64)
    for i in range(-rx, rx + 1):  # column offset: outer
        for j in range(-ry, ry + 1):  # row offset: inner
            color = color + tp[ry + j:ry + j + h, rx + i:rx + i + w]
            count = count + cp[ry + j:ry + j + h, rx + i:rx + i + w]
    assert (count != 0).all(), "Pixel found with no samples"
    return color / count.astype(np.float64)[:, :, None]


def filtered_image(totals, counts, w, h, radius):
    """Buffer::image (buffer.rs:43-56) with per-pixel counts -> (h, w, 3) uint8"""
    return color_bytes(filtered_color(totals, counts, w, h, radius))


def variance(frames, counts):
    """Buffer::variance (buffer.rs:59-73) over per-pixel sample lists (pixel p holds frames[k][p] for k < counts[p]),
    vectorised over pixels: mean = total / n, ss summed over the pixel's samples in order as ((dx*dx + dy*dy) + dz*dz),
    ss / (n - 1), then a SEQUENTIAL sum over the pixels in index order (np.cumsum; np.sum would add pairwise)."""
    counts = np.asarray(counts)
    n = counts.astype(np.float64)
    with np.errstate(all="ignore"):  # n = 1: ss / 0 = 0/0 = NaN, as the reference computes
        mean = masked_totals(frames, counts) / n[:, None]
        ss = np.zeros(len(n))
        for k, F in enumerate(frames):
            d = F - mean
            # a pixel without a k-th sample adds +0.0 to an ss that started at +0.0: no bit changes
            ss = ss + np.where(counts > k, dot(d, d), 0.0)
        per_pixel = ss / (n - 1.0)
    return float(np.cumsum(per_pixel)[-1]) / float(len(per_pixel))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_against(dev, left, frames, r):
    """a DeviceBuffer after adaptive rounds over `frames` (left: what each round returned) against the model's run r:
    per-pixel counts, the active counts, the batches recorded and the totals' bits -> the counts"""
    counts = dev.sample_counts().ravel()
    assert np.array_equal(counts, r["counts"])
    assert left == r["active"]
    assert dev.num_batches() == sum(1 for k in range(len(frames)) if k == 0 or r["active"][k - 1] > 0)
    assert np.array_equal(bits(dev.totals().reshape(-1, 3)), bits(masked_totals(frames, counts)))
    return counts


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
