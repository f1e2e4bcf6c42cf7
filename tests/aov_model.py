"""The expected first-hit feature buffers (rptgpu_render_aov) from the oracle alone: oracle_camera_ray per
pixel and sample, ONE oracle_closest_hit over all of them, then the fold of the contract as a plain loop in ascending
sample order (not np.sum: its pairwise order differs).  Test helper, not a test."""
import numpy as np

from oracle import oracle_ffi as O

CHANNELS = ("depth", "normal", "albedo", "position")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def owned(params):
    """(H, W) bool: the pixels of the call's part (RptRenderParams' tile partition)."""
    w, h = params.width, params.height
    tw, th = params.tile_width or 32, params.tile_height or 8
    pc = params.part_count or 1
    pi = params.part_index if params.part_count else 0
    y, x = np.mgrid[0:h, 0:w]
    tile = (y // th) * ((w + tw - 1) // tw) + x // tw
    return (tile % pc) == pi if pc > 1 else np.ones((h, w), dtype=bool)


def rays(camera, params, pixels):
    """-> origins, dirs of shape (len(pixels), iterations, 3): sample s of pixel (x, y) at [k, s - base]"""
    n, it = len(pixels), params.iterations
    o = np.empty((n, it, 3))
    d = np.empty((n, it, 3))
    for k, (x, y) in enumerate(pixels):
        for s in range(it):
            o[k, s], d[k, s] = O.camera_ray(camera, params, int(x), int(y), params.sample_index_base + s)
    return o, d


def colors(scene):
    """objects[i].material.color as the library receives it (Material.lower)"""
    return np.array([list(ob._material.lower().color) for ob in scene.objects], dtype=np.float64).reshape(-1, 3)


def fold(o, d, t, nrm, obj, albedo_of):
    """The contract's steps 3 and 4 for ONE pixel: its samples' rays and hits in ascending sample order."""
    hits = 0
    depth = np.float64(0.0)
    normal, albedo, position = np.zeros(3), np.zeros(3), np.zeros(3)
    for s in range(len(t)):
        if obj[s] < 0:
            continue
        hits += 1
        depth = depth + t[s]
        for c in range(3):
            normal[c] = normal[c] + nrm[s, c]
            albedo[c] = albedo[c] + albedo_of[obj[s], c]
            position[c] = position[c] + (o[s, c] + t[s] * d[s, c])  # one multiply, then one add
    return hits, depth, normal, albedo, position, int(obj[0])


def expected(scene, camera, params, pixels=None, oracle_scene=None):
    """The buffers of the listed pixels ((x, y) pairs; default: every pixel the call owns, row-major) -> dict of arrays
    over the list: hits (n,) u32, depth (n,), normal / albedo / position (n, 3), object (n,) i32; plus 'pixels'."""
    if pixels is None:
        ys, xs = np.nonzero(owned(params))
        pixels = list(zip(xs.tolist(), ys.tolist()))
    osc = oracle_scene or O.OracleScene(scene)
    o, d = rays(camera, params, pixels)
    n, it = len(pixels), params.iterations
    t, nrm, obj = osc.closest_hit(o.reshape(-1, 3), d.reshape(-1, 3))
    t, nrm, obj = t.reshape(n, it), nrm.reshape(n, it, 3), obj.reshape(n, it)
    col = colors(scene)
    out = {"pixels": pixels, "hits": np.zeros(n, dtype=np.uint32), "depth": np.zeros(n), "normal": np.zeros((n, 3)),
           "albedo": np.zeros((n, 3)), "position": np.zeros((n, 3)), "object": np.full(n, -1, dtype=np.int32),
           "rays": (o, d)}
    with np.errstate(all="ignore"):
        for k in range(n):
            h, de, no, al, po, ob = fold(o[k], d[k], t[k], nrm[k], obj[k], col)
            out["hits"][k], out["depth"][k], out["normal"][k], out["albedo"][k], out["position"][k] = h, de, no, al, po
            out["object"][k] = ob
    return out


def full_frame(exp, params):
    """expected() over the owned pixels as full-frame arrays: 0 (object: -1) outside the part."""
    h, w = params.height, params.width
    f = {"hits": np.zeros((h, w), dtype=np.uint32), "depth": np.zeros((h, w)), "normal": np.zeros((h, w, 3)),
         "albedo": np.zeros((h, w, 3)), "position": np.zeros((h, w, 3)), "object": np.full((h, w), -1, dtype=np.int32)}
    for k, (x, y) in enumerate(exp["pixels"]):
        for name in f:
            f[name][y, x] = exp[name][k]
    return f


def mismatches(got, want):
    """names of the arrays whose raw bits differ (f64 compared as uint64: -0.0 != +0.0, NaN payloads count)"""
    bad = []
    for name in ("hits", "object") + CHANNELS:
        if name not in got and name not in want:
            continue
        a, b = got[name], want[name]
        same = a.shape == b.shape and (np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b))
        if not same:
            bad.append(name)
    return bad
