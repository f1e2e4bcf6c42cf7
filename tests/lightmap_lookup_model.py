"""rptgpu_lookup_lightmap's rule restated in numpy from the text of include/rpt_gpu_lightmap_lookup.h: plain f64, every
expression in the order the header writes it, so that the kernel can be held to it to the bit (tests/test_gpu_lightmap_lookup.py)
and the rule itself to closed forms without a GPU (tests/test_lightmap_lookup_host.py).  A helper, not a test.

lookup(object, primitive, barycentric, bindings, filter, fallback): the inputs are rptgpu_hit_surface's arrays for the rays and
the caller's bindings (anything with .object, .uvs, .map, .valid: rpt_amd.lightmap.Binding); -> a dict with `binding`,
`covered`, `uv`, `value` as the call's channels of those names."""
import numpy as np

NEAREST, BILINEAR = "nearest", "bilinear"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _texels(b):
    """-> (map as (H, W, 3) — a scalar map three times —, valid as (H, W) bool)"""
    tex = np.asarray(b.map, dtype=np.float64)
    if tex.ndim == 2:
        tex = np.repeat(tex[:, :, None], 3, axis=2)
    valid = np.ones(tex.shape[:2], dtype=bool) if b.valid is None else np.asarray(b.valid) != 0
    return tex, valid


def interpolate_uv(uvs, primitive, barycentric):
    """U = (u * uv1.x + v * uv2.x) + w * uv3.x, V likewise: (m, 2)"""
    t = np.asarray(uvs, dtype=np.float64)[primitive]          # (m, 3, 2)
    u, v, w = (barycentric[:, k, None] for k in range(3))
    return (u * t[:, 0] + v * t[:, 1]) + w * t[:, 2]


def _axis(c, size):
    """one axis of the bilinear rule: the coordinate c = U or V, the map's size -> (i0, i1 clamped, f, g)"""
    s = np.fmin(np.fmax(c * np.float64(size) - 0.5, -1.0), np.float64(size))
    f0 = np.floor(s)
    f = s - f0
    i0 = f0.astype(np.int64)
    i1 = i0 + 1
    return np.clip(i0, 0, size - 1), np.clip(i1, 0, size - 1), f, 1.0 - f


def valid_taps(b, uv):
    """how many of the bilinear rule's four taps are valid, per ray: (m,) int"""
    _, valid = _texels(b)
    H, W = valid.shape
    with np.errstate(all="ignore"):
        x0, x1, _, _ = _axis(uv[:, 0], W)
        y0, y1, _, _ = _axis(uv[:, 1], H)
    return valid[y0, x0].astype(int) + valid[y0, x1] + valid[y1, x0] + valid[y1, x1]


def fetch(b, uv, filter):
    """the rule for the rays bound to b, uv (m, 2) -> (covered (m,), value (m, 3) — meaningful where covered)"""
    tex, valid = _texels(b)
    H, W = valid.shape
    U, V = uv[:, 0], uv[:, 1]
    finite = np.isfinite(U) & np.isfinite(V)
    with np.errstate(all="ignore"):
        if filter == NEAREST:
            x = np.fmin(np.fmax(np.floor(U * np.float64(W)), 0.0), np.float64(W - 1)).astype(np.int64)
            y = np.fmin(np.fmax(np.floor(V * np.float64(H)), 0.0), np.float64(H - 1)).astype(np.int64)
            return finite & valid[y, x], tex[y, x]
        assert filter == BILINEAR
        x0, x1, fx, gx = _axis(U, W)
        y0, y1, fy, gy = _axis(V, H)
        zero = np.float64(0.0)
        w00 = np.where(valid[y0, x0], gx * gy, zero)
        w10 = np.where(valid[y0, x1], fx * gy, zero)
        w01 = np.where(valid[y1, x0], gx * fy, zero)
        w11 = np.where(valid[y1, x1], fx * fy, zero)
        ws = ((w00 + w10) + w01) + w11
        m00, m10, m01, m11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
        value = (((w00[:, None] * m00 + w10[:, None] * m10) + w01[:, None] * m01) + w11[:, None] * m11) / ws[:, None]
    return finite & (ws > 0.0), value


def lookup(object, primitive, barycentric, bindings, filter=BILINEAR, fallback=(0.0, 0.0, 0.0)):
    object, primitive = np.asarray(object), np.asarray(primitive)
    barycentric = np.asarray(barycentric, dtype=np.float64)
    n = len(object)
    binding = np.full(n, -1, dtype=np.int32)
    covered = np.zeros(n, dtype=np.uint8)
    uv = np.zeros((n, 2))
    value = np.tile(np.asarray(fallback, dtype=np.float64), (n, 1))
    for k, b in enumerate(bindings):
        at = np.flatnonzero((object == int(b.object)) & (primitive >= 0))
        if not len(at):
            continue
        binding[at] = k
        with np.errstate(all="ignore"):
            uv[at] = interpolate_uv(b.uvs, primitive[at], barycentric[at])
        ok, val = fetch(b, uv[at], filter)
        covered[at] = ok
        value[at[ok]] = val[ok]
    return {"binding": binding, "covered": covered, "uv": uv, "value": value}


# ---- the round trip's case, shared by the host test (which holds the rays to the cap with the oracle) and the GPU test
ROUND_TRIP_SIZE = 64
ROUND_TRIP_RAYS = 600


def round_trip_case():
    """cornell's floor (object 0, two triangles, untransformed) under a planar chart that lays its bounding rectangle over
    [1/16, 15/16]^2 of a 64 x 64 map, and rays from inside the box aimed at random points of it -> (object, rows (2, 18), uvs
    (2, 3, 2), origins, dirs, extent = the floor's largest |coordinate|)"""
    import small_scenes
    import surface_model
    scene = small_scenes.small("cornell")[0]
    rows = next(np.ascontiguousarray(mesh.triangles) for ob, child, chain, mesh in surface_model.meshes_of(scene)
                if ob == 0 and child < 0 and chain == [None])
    v = rows[:, :9].reshape(-1, 3, 3)
    flat = v.reshape(-1, 3)
    ext = flat.max(axis=0) - flat.min(axis=0)
    ax = np.sort(np.argsort(ext)[1:])
    uvs = np.ascontiguousarray(1.0 / 16.0 + (14.0 / 16.0) * (v[:, :, ax] - flat.min(axis=0)[ax]) / ext[ax])
    rs = np.random.RandomState(2511)
    o = rs.uniform((60.0, 120.0, 60.0), (500.0, 500.0, 500.0), (ROUND_TRIP_RAYS, 3))
    w = rs.dirichlet((1.0, 1.0, 1.0), ROUND_TRIP_RAYS)
    tri = v[rs.randint(len(v), size=ROUND_TRIP_RAYS)]
    p = w[:, 0, None] * tri[:, 0] + w[:, 1, None] * tri[:, 1] + w[:, 2, None] * tri[:, 2]
    d = np.ascontiguousarray((p - o) * rs.uniform(0.25, 4.0, (ROUND_TRIP_RAYS, 1)))
    return 0, rows, uvs, o, d, float(np.abs(flat).max())


# ---- rptgpu_render_views_lightmapped: the shading of a sample and the fold of a pixel's samples, as the header writes them
PI = 3.141592653589793


def shade(hit, environment, albedo, emittance, covered, value, unbound_irradiance):
    """one sample of every index -> L (n, 3).  hit (n,) bool; environment (n, 3): the environment's colour for the ray
    (read where the ray misses); albedo (n, 3) and emittance (n,): the hit object's material; covered, value: the lookup's"""
    irradiance = np.where(np.asarray(covered)[:, None] != 0, value, np.asarray(unbound_irradiance, dtype=np.float64)[None, :])
    e = np.asarray(emittance, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        lit = e * albedo + (albedo / PI) * irradiance
    return np.where(np.asarray(hit)[:, None], lit, environment)


def fold(samples, exposure_value=0.0):
    """out = (the sum over the samples in order, from +0.0, of L) / iterations * 2^exposure_value"""
    acc = np.zeros_like(samples[0])
    for L in samples:
        acc = acc + L
    return acc / float(len(samples)) * 2.0 ** float(exposure_value)
