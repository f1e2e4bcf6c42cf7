"""include/rpt_gpu_probe_volume.h restated in numpy, operation for operation: the rule that reads a grid of SH9
probes at a point — the cell per axis, the eight taps and their weights, the sums in the header's order, one division per
channel —, the ray form's facing of the normal, and the irradiance rptgpu_render_views_probe_lit gives a hit.  Every sum is
written out tap by tap and coefficient by coefficient; numpy only evaluates each step for all points at once, which changes no
bit: + - * / floor fmin fmax are IEEE per element, and nothing here is contracted.  No GPU, no library."""
import numpy as np

from rpt_amd.probes import sh9_basis

A = (3.141592653589793, 2.0943951023931953, 2.0943951023931953, 2.0943951023931953, 0.7853981633974483,
     0.7853981633974483, 0.7853981633974483, 0.7853981633974483, 0.7853981633974483)


def cell(q, o, h, n):
    """step 2 for one axis -> (f, i0, i1, inside)"""
    with np.errstate(all="ignore"):
        g = (q - o) / h
        top = float(n - 1)
        s = np.fmin(np.fmax(g, 0.0), top)   # a NaN g takes the fmax's other argument
        i0f = np.floor(s)
        f = s - i0f
        i0 = i0f.astype(np.int64)
        i1 = np.minimum(i0 + 1, n - 1)      # after f is formed
        inside = (g >= 0.0) & (g <= top)
    return f, i0, i1, inside


def rule(volume, P, N, normal_bias):
    """steps 1 to 8 at the points P (n, 3) with the directions N (n, 3), used as given -> (E (n, 3), covered (n,) bool, inside
    (n,) bool); E is meaningful where covered.  volume: origin, spacing, counts, coeffs, valid (rpt_amd.probes.ProbeVolume's)"""
    P, N = np.asarray(P, dtype=np.float64), np.asarray(N, dtype=np.float64)
    nx, ny, nz = volume.counts
    count = nx * ny * nz
    C = np.asarray(volume.coeffs, dtype=np.float64).reshape(count, 9, 3)
    valid = None if volume.valid is None else np.asarray(volume.valid).reshape(count) != 0
    with np.errstate(all="ignore"):
        Q = [P[:, a] + normal_bias * N[:, a] for a in range(3)]
        fx, i0, i1, in_x = cell(Q[0], volume.origin[0], volume.spacing[0], nx)
        fy, j0, j1, in_y = cell(Q[1], volume.origin[1], volume.spacing[1], ny)
        fz, k0, k1, in_z = cell(Q[2], volume.origin[2], volume.spacing[2], nz)
        X, Y, Z = (1.0 - fx, fx), (1.0 - fy, fy), (1.0 - fz, fz)
        I, J, K = (i0, i1), (j0, j1), (k0, k1)
        p, w = [], []
        for t in range(8):
            a, b, c = t & 1, (t >> 1) & 1, t >> 2
            pt = (K[c] * ny + J[b]) * nx + I[a]
            wt = (X[a] * Y[b]) * Z[c]
            if valid is not None:
                wt = np.where(valid[pt], wt, 0.0)
            p.append(pt)
            w.append(wt)
        ws = w[0] + w[1]
        for t in range(2, 8):
            ws = ws + w[t]
        Yn = sh9_basis(N)
        M = [None, None, None]
        for j in range(9):
            B = A[j] * Yn[:, j]
            for c in range(3):
                S = w[0] * C[p[0], j, c]
                for t in range(1, 8):
                    S = S + w[t] * C[p[t], j, c]
                M[c] = B * S if j == 0 else M[c] + B * S
        E = np.stack([M[c] / ws for c in range(3)], axis=1)
        finite = np.isfinite(Q[0]) & np.isfinite(Q[1]) & np.isfinite(Q[2]) & np.isfinite(N).all(axis=1)
        covered = finite & (ws > 0.0)
    return E, covered, in_x & in_y & in_z


def sample(volume, positions, normals, normal_bias=0.0, fallback=(0.0, 0.0, 0.0)):
    """rptgpu_sample_probe_volume -> {"value", "covered", "inside"}"""
    E, covered, inside = rule(volume, positions, normals, normal_bias)
    value = np.where(covered[:, None], E, np.asarray(fallback, dtype=np.float64)[None, :])
    return {"value": value, "covered": covered.astype(np.uint8), "inside": inside.astype(np.uint8)}


def face(normal, dirs):
    """the ray form's N: first_hits' normal, negated where it looks along the ray"""
    n, d = np.asarray(normal, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    with np.errstate(all="ignore"):
        dot = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    return np.where((dot > 0.0)[:, None], -n, n)


def lookup(volume, dirs, hits, normal_bias=0.0, fallback=(0.0, 0.0, 0.0)):
    """rptgpu_lookup_probe_volume from first_hits' t, object, normal, position for the rays -> all seven channels"""
    obj = np.asarray(hits["object"])
    hit = obj >= 0
    N = np.where(hit[:, None], face(hits["normal"], dirs), 0.0)
    P = np.where(hit[:, None], hits["position"], 0.0)
    E, covered, inside = rule(volume, P, N, normal_bias)
    covered, inside = covered & hit, inside & hit
    value = np.where(covered[:, None], E, np.asarray(fallback, dtype=np.float64)[None, :])
    return {"t": np.asarray(hits["t"]), "object": obj, "position": P, "normal": N, "value": value,
            "covered": covered.astype(np.uint8), "inside": inside.astype(np.uint8)}


def irradiance(lightmap_covered, lightmap_value, volume_covered, volume_value):
    """rptgpu_render_views_probe_lit's I as (covered, value) for lightmap_lookup_model.shade, which takes unbound_irradiance
    where covered is 0: the lightmap's value where it covers, else the volume's E cut at zero where that covers.  -> also the
    branch of each index: 0 lightmap, 1 volume, 2 neither"""
    lc, vc = np.asarray(lightmap_covered) != 0, np.asarray(volume_covered) != 0
    E = np.asarray(volume_value, dtype=np.float64)
    with np.errstate(all="ignore"):
        cut = np.where(E < 0.0, 0.0, E)
    value = np.where(lc[:, None], lightmap_value, cut)
    return (lc | vc).astype(np.uint8), value, np.where(lc, 0, np.where(vc, 1, 2))
