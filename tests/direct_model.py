"""rptgpu_bake_direct restated in numpy from the text of include/rpt_gpu_direct.h — the fold, the project's dot and
normalize, and Light::illuminate for the two kinds that take no draw (light.rs:23-47).  A Light::Object's sample needs the
Philox stream and Shape::sample, which this module does not restate: the caller brings it (`sample_object`; the tests bring
the oracle's).  The closest-hit query is the caller's too (`closest_t`): the header defines t by rptgpu_closest_hit."""
import numpy as np

from rpt_amd import _abi

DBL_MAX = 1.7976931348623157e308
INF = float("inf")


def dot(a, b):
    """the project's dot: the three products summed left to right"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return v / np.sqrt(dot(v, v))[..., None]


def illuminate(light, pos, seed, stream, sample, draw, sample_object=None):
    """Light::illuminate(pos, rng) with the stream at `draw` -> (I, wi, dist, the draw behind it)"""
    pos = np.asarray(pos, dtype=np.float64)
    if light.kind == _abi.RPT_LIGHT_POINT:
        disp = np.array(tuple(light.vec), dtype=np.float64) - pos
        length = np.sqrt(dot(disp, disp))
        with np.errstate(all="ignore"):
            return np.array(tuple(light.color), dtype=np.float64) / (length * length), disp / length, float(length), draw
    if light.kind == _abi.RPT_LIGHT_DIRECTIONAL:
        return np.array(tuple(light.color), dtype=np.float64), -normalize(np.array(tuple(light.vec), dtype=np.float64)), INF, draw
    if light.kind == _abi.RPT_LIGHT_OBJECT:
        return sample_object(light, pos, seed, stream, sample, draw)
    raise ValueError("Light::Ambient has no illuminate in this sum")


def chain(lights, pos, seed, stream, sample, illuminate=illuminate, **kw):
    """one sample of one point: every light of the scene in scene order on one stream from draw 0 -> a list with None for
    an ambient light (skipped, no draw) and (I, wi, dist) for every other"""
    draw, out = 0, []
    for light in lights:
        if light.kind == _abi.RPT_LIGHT_AMBIENT:
            out.append(None)
            continue
        I, wi, dist, draw = illuminate(light, pos, seed, stream, sample, draw, **kw)
        out.append((np.asarray(I, dtype=np.float64), np.asarray(wi, dtype=np.float64), float(dist)))
    return out


def direct(lights, positions, normals, samples, seed, closest_t, sample_index_base=0, streams=None, illuminate=illuminate,
           details=False, **kw):
    """out [n][3] as the header defines it.  closest_t(origins (m, 3), dirs (m, 3)) -> t (m,), rptgpu_closest_hit's.
    details: also the (point, sample, light) triples as arrays — cosv, t, stop — for a test's own conditions"""
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    nn = normalize(np.asarray(normals, dtype=np.float64).reshape(-1, 3))
    n = len(positions)
    ids = np.arange(n) if streams is None else np.asarray(streams)
    rows = []  # (i, k, l, I, wi, dist) in the header's order: i, then k ascending, then l in scene order
    for i in range(n):
        for k in range(samples):
            for l, s in enumerate(chain(lights, positions[i], seed, int(ids[i]), sample_index_base + k, illuminate, **kw)):
                if s is not None:
                    rows.append((i, k, l) + s)
    out = np.zeros((n, 3))
    if not rows:
        return (out, None) if details else out
    idx = np.array([r[0] for r in rows])
    I = np.array([r[3] for r in rows])
    wi = np.array([r[4] for r in rows])
    stop = np.fmin(np.array([r[5] for r in rows]), DBL_MAX)
    t = np.asarray(closest_t(positions[idx], wi), dtype=np.float64)
    with np.errstate(all="ignore"):
        cosv = dot(wi, nn[idx])
        c = I * cosv[:, None]
        adds = (cosv > 0.0) & (t > stop)  # both false for NaN
    acc = np.zeros((n, 3))
    for j in range(len(rows)):  # ascending: the header's order
        if adds[j]:
            acc[idx[j]] = acc[idx[j]] + c[j]
    out = acc / float(samples)
    if details:
        return out, {"point": idx, "light": np.array([r[2] for r in rows]), "cosv": cosv, "t": t, "stop": stop, "adds": adds, "c": c}
    return out
