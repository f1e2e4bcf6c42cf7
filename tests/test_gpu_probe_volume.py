"""The probe volume on a real MI355X (include/rpt_gpu_probe_volume.h): rptgpu_sample_probe_volume,
rptgpu_lookup_probe_volume and rptgpu_render_views_probe_lit against the numpy restatement of the header
(tests/probe_volume_model.py), bit for bit unless a test says otherwise.

1. The point form: grids of 3 x 2 x 2, 1 x 1 x 1 and 4 x 1 x 3 probes with random coefficients, 257 points — every probe's own
   position, faces and corners of the grid, points far outside, NaN and infinite points and normals, a normal that is no unit
   vector —, normal_bias 0 and 0.35, a NaN and an infinite coefficient (the grids of more than one probe), valid masks that
   take some taps out, all of them, and none.  Each channel named alone with sentinels behind and beside it; pieces of 64 and
   of 3 points; torch tensors on the device.
2. The ray form on cornell (the flat route) and wine_glass (the per-tree route), and under RPT_FLAG_GENERAL_TRAVERSAL: rays from
   the scene's camera, rays aimed at its meshes from inside, rays that leave it — against first_hits' own arrays with the
   facing rule and the model applied in numpy.
3. The views form: three views of 16 x 9, one per projection, 2 samples, seed_stride 1, tests/views_model.py's rays, the
   lightmap term from tests/lightmap_lookup_model.py and the volume's from the model — without bindings, with one binding,
   and with a volume whose mask leaves hits uncovered, so that all three branches of the irradiance occur.
4. The meaning: ProbeVolume.bake is bake_probes at positions(), and a lookup at a probe's own position is sh9_irradiance of
   its coefficients."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import Camera, GpuScene, ProbeVolume, _abi, sh9_irradiance

import lightmap_lookup_model as L
import probe_volume_model as PV
import small_scenes
import surface_model as M
import test_gpu_lightmap_lookup as LK
import test_gpu_occlusion as occ
import views_model

pytestmark = pytest.mark.gpu

GENERAL = _abi.RPT_FLAG_GENERAL_TRAVERSAL
FALLBACK = (-1.5, 0.25, 7.0)
POINT_NAMES = ("value", "covered", "inside")
RAY_NAMES = ("t", "object", "position", "normal", "value", "covered", "inside")
N_POINTS = 257
GRIDS = ((3, 2, 2), (1, 1, 1), (4, 1, 3))
ORIGIN, SPACING = (-1.0, 0.5, 2.0), (0.7, 1.3, 0.45)


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(small_scenes.small(name)[0], 0)


def same(a, b):
    """the raw bits — but a NaN equals any NaN: which payload a sum of NaNs keeps is no part of the contract"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    return bool(((M.bits(a) == M.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def differing(got, want, names):
    return [k for k in names if k not in got or not same(got[k], want[k])]


# ---- 1. the point form
@functools.lru_cache(maxsize=None)
def volume(counts, mask):
    """random coefficients in [-4, 4]; with more than one probe a NaN in probe 0 and an infinity in the last one.  mask:
    "some" (each probe valid with probability 0.6), "none" (every probe invalid: all eight taps out everywhere), None"""
    nx, ny, nz = counts
    n = nx * ny * nz
    rs = np.random.RandomState(100 * nx + 10 * ny + nz)
    coeffs = rs.uniform(-4.0, 4.0, (nz, ny, nx, 9, 3))
    if n > 1:
        coeffs.reshape(n, 9, 3)[0, 2, 1] = np.nan
        coeffs.reshape(n, 9, 3)[n - 1, 5, 0] = np.inf
    valid = {None: None, "none": np.zeros((nz, ny, nx), dtype=np.uint8), "some": (rs.uniform(size=(nz, ny, nx)) < 0.6).astype(np.uint8)}[mask]
    coeffs.setflags(write=False)
    return ProbeVolume(ORIGIN, SPACING, counts, coeffs, valid)


@functools.lru_cache(maxsize=None)
def points(counts):
    """257 points and directions for a grid -> (positions, normals), read-only"""
    rs = np.random.RandomState(sum(counts))
    o, h, c = np.array(ORIGIN), np.array(SPACING), np.array(counts)
    top = o + (c - 1) * h
    own = ProbeVolume.positions(ORIGIN, SPACING, counts)                       # every probe's own position
    span = np.maximum(top - o, h)
    rand = o - 0.3 * span + rs.uniform(size=(N_POINTS, 3)) * 1.6 * span        # inside and a little outside
    pos = rand.copy()
    pos[:len(own)] = own
    k = len(own)
    pos[k], pos[k + 1] = o, top                                                # two corners
    pos[k + 2, 0], pos[k + 3, 1], pos[k + 4, 2] = o[0], top[1], o[2]           # on three faces
    pos[k + 5], pos[k + 6] = o - 100.0 * span, top + 1e9 * span                # far outside
    pos[k + 7, 1], pos[k + 8, 2], pos[k + 9, 0] = np.nan, np.inf, -np.inf
    nrm = rs.normal(size=(N_POINTS, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[k + 10] *= 2.5                                                         # no unit vector: used as given
    nrm[k + 11, 0], nrm[k + 12, 2] = np.nan, np.inf
    nrm[k + 13] = 0.0
    for a in (pos, nrm):
        a.setflags(write=False)
    return pos, nrm


@pytest.mark.parametrize("bias", [0.0, 0.35])
@pytest.mark.parametrize("mask", [None, "some", "none"])
@pytest.mark.parametrize("counts", GRIDS, ids=["3x2x2", "1x1x1", "4x1x3"])
def test_the_point_form_is_the_model(counts, mask, bias):
    pos, nrm = points(counts)
    vol = volume(counts, mask)
    want = PV.sample(vol, pos, nrm, bias, FALLBACK)
    got = gpu("cornell").sample_probe_volume(pos, nrm, vol, normal_bias=bias, fallback=FALLBACK)
    assert got["value"].shape == (N_POINTS, 3) and got["covered"].dtype == np.uint8 and got["inside"].dtype == np.uint8
    assert differing(got, want, POINT_NAMES) == []
    # the case says something
    assert not want["inside"].all()
    if min(counts) > 1 or bias == 0.0:                     # (one probe along an axis: inside are the points ON its plane alone)
        assert want["inside"].any()
    assert not want["covered"].all()                                          # the NaN and infinite points and normals
    if mask == "none":
        assert not want["covered"].any() and same(want["value"], np.tile(FALLBACK, (N_POINTS, 1)))
    else:
        assert want["covered"].sum() >= 100
    if mask is None and counts != (1, 1, 1):
        assert np.isnan(want["value"][want["covered"] != 0]).any()             # the NaN coefficient is seen
        assert np.isfinite(want["value"][want["covered"] != 0]).any()


def test_each_channel_alone_leaves_everything_else_untouched():
    counts, n, tail = (3, 2, 2), N_POINTS, 8
    pos, nrm = (np.array(a) for a in points(counts))
    vol = volume(counts, "some")
    want = PV.sample(vol, pos, nrm, 0.35, FALLBACK)
    g = gpu("cornell")
    rec, keep = g._lower_volume(rpt_amd._marshal.HOST, vol, "test")
    types = dict(_abi.RptVolumeArrays._fields_)
    shapes = {"t": ((n + tail,), np.float64), "object": ((n + tail,), np.int32), "position": ((n + tail, 3), np.float64),
              "normal": ((n + tail, 3), np.float64), "value": ((n + tail, 3), np.float64), "covered": ((n + tail,), np.uint8),
              "inside": ((n + tail,), np.uint8)}
    bit = {"value": _abi.RPT_VOLUME_VALUE, "covered": _abi.RPT_VOLUME_COVERED, "inside": _abi.RPT_VOLUME_INSIDE}
    PD = C.POINTER(C.c_double)
    for named in (("value",), ("covered",), ("inside",), ("covered", "inside")):
        outs = {k: np.full(s, 7, dtype=dt) for k, (s, dt) in shapes.items()}
        a = _abi.RptVolumeArrays()
        a.struct_size = C.sizeof(a)
        for k, arr in outs.items():
            setattr(a, k, arr.ctypes.data_as(types[k]))
        q = _abi.RptVolumeQuery()
        q.struct_size, q.channels, q.normal_bias = C.sizeof(q), sum(bit[k] for k in named), 0.35
        q.fallback = _abi.V3(*FALLBACK)
        p2, n2 = pos.copy(), nrm.copy()
        _abi.check(g.lib.rptgpu_sample_probe_volume(g.handle, n, p2.ctypes.data_as(PD), n2.ctypes.data_as(PD), C.byref(rec),
                                                    C.byref(q), C.byref(a)), g.handle)
        assert differing({k: outs[k][:n] for k in named}, want, named) == []
        assert all((outs[k][n:] == 7).all() for k in named)                    # the tail behind every output
        assert all((outs[k] == 7).all() for k in shapes if k not in named)     # the arrays that are not named
        assert same(p2, pos) and same(n2, nrm)                                 # the inputs
    del keep


@pytest.mark.parametrize("piece", [64, 3])
def test_pieces_do_not_change_a_bit(piece, monkeypatch):
    counts = (4, 1, 3)
    pos, nrm = points(counts)
    vol = volume(counts, "some")
    monkeypatch.setenv("RPTGPU_VOLUME_PIECE", str(piece))
    got = gpu("cornell").sample_probe_volume(pos, nrm, vol, normal_bias=0.35, fallback=FALLBACK)
    assert differing(got, PV.sample(vol, pos, nrm, 0.35, FALLBACK), POINT_NAMES) == []


def on_device(vol):
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a writable, contiguous copy of the shared arrays)
    return ProbeVolume(vol.origin, vol.spacing, vol.counts, to(vol.coeffs), None if vol.valid is None else to(vol.valid)), to, dev


@pytest.mark.parametrize("mask", [None, "some"])
def test_device_tensors_give_the_host_forms_bits(mask):
    counts = (3, 2, 2)
    pos, nrm = points(counts)
    vol = volume(counts, mask)
    g = gpu("cornell")
    dvol, to, dev = on_device(vol)
    host = g.sample_probe_volume(pos, nrm, vol, normal_bias=0.35, fallback=FALLBACK)
    got = g.sample_probe_volume(to(pos), to(nrm), dvol, normal_bias=0.35, fallback=FALLBACK)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values())
    assert got["value"].dtype == torch.float64 and got["covered"].dtype == torch.uint8
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, host, POINT_NAMES) == []
    with torch.cuda.stream(torch.cuda.Stream(dev)):  # on a stream of the caller's own
        got = g.sample_probe_volume(to(pos), to(nrm), dvol, normal_bias=0.35, fallback=FALLBACK, channels=_abi.RPT_VOLUME_VALUE)
        assert same(got["value"].cpu().numpy(), host["value"])
    with pytest.raises(ValueError):  # tensors and numpy arrays do not mix
        g.sample_probe_volume(to(pos), to(nrm), vol)


# ---- 2. the ray form
RAY_SCENES = ("cornell", "wine_glass")
HIT_CHANNELS = _abi.RPT_HIT_T | _abi.RPT_HIT_NORMAL | _abi.RPT_HIT_OBJECT | _abi.RPT_HIT_POSITION


@functools.lru_cache(maxsize=None)
def scene_volume(name, mask=None):
    """a 4 x 3 x 4 grid over the middle 60 % of the scene's box (so hits lie inside and outside it), finite coefficients.
    mask "half": the probes of the two upper x layers are invalid, so a hit beyond them has all eight taps out"""
    lo, hi = (np.array(x) for x in occ.BOXES[name])
    counts = (4, 3, 4)
    origin = lo + 0.2 * (hi - lo)
    spacing = 0.6 * (hi - lo) / (np.array(counts) - 1)
    rs = np.random.RandomState(len(name) + 7)
    coeffs = rs.uniform(-1.0, 1.0, (counts[2], counts[1], counts[0], 9, 3))
    coeffs[..., 0, :] += 4.0  # (mostly positive irradiance, some ringing below zero)
    valid = None
    if mask == "half":
        valid = np.ones((counts[2], counts[1], counts[0]), dtype=np.uint8)
        valid[:, :, 2:] = 0
    return ProbeVolume(origin, spacing, counts, coeffs, valid)


@functools.lru_cache(maxsize=None)
def rays(name):
    """320 rays through a 20 x 16 grid of the scene's camera, 200 aimed at its meshes from inside its box, 60 that leave it;
    the directions are no unit vectors -> (origins, dirs, first_hits' arrays for them), read-only"""
    scene, cam = small_scenes.small(name)[:2]
    eye, fwd, up = (np.array([float(x) for x in v]) for v in (cam.eye, cam.direction, cam.up))
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    half = math.tan(float(cam.fov) / 2.0)
    xs, ys = np.meshgrid((np.arange(20) + 0.5) / 10.0 - 1.0, (np.arange(16) + 0.5) / 8.0 - 1.0)
    d_cam = fwd[None, :] + half * (xs.reshape(-1, 1) * right[None, :] * 1.25 + ys.reshape(-1, 1) * upv[None, :])
    o_cam = np.tile(eye, (len(d_cam), 1))
    o_in, d_in = M.aimed_rays(scene, occ.BOXES[name], 77 + len(name), 200)
    rs = np.random.RandomState(len(name))
    lo, hi = (np.array(x) for x in occ.BOXES[name])
    o_far = hi + (hi - lo) * rs.uniform(2.0, 3.0, (60, 3))
    d_far = rs.uniform(0.1, 1.0, (60, 3)) * (hi - lo)
    o = np.ascontiguousarray(np.concatenate([o_cam, o_in, o_far]))
    d = np.ascontiguousarray(np.concatenate([d_cam * 1.7, d_in, d_far]))
    hits = gpu(name).first_hits(o, d, channels=HIT_CHANNELS)
    for a in (o, d) + tuple(hits.values()):
        a.setflags(write=False)
    return o, d, hits


@pytest.mark.parametrize("flags", [0, GENERAL], ids=["default-route", "general"])
@pytest.mark.parametrize("name", RAY_SCENES)
def test_the_ray_form_is_first_hits_faced_and_the_model(name, flags):
    o, d, hits = rays(name)
    vol, bias = scene_volume(name), 0.01 * float(np.linalg.norm(np.array(occ.BOXES[name][1]) - np.array(occ.BOXES[name][0])))
    want = PV.lookup(vol, d, hits, bias, FALLBACK)
    got = gpu(name).lookup_probe_volume(o, d, vol, normal_bias=bias, fallback=FALLBACK, flags=flags)
    assert differing(got, want, RAY_NAMES) == []
    # the rays hold a hit, a miss and a normal that was turned to face its ray; hits inside and outside the grid
    hit = hits["object"] >= 0
    n = hits["normal"]
    turned = hit & (((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) > 0.0)
    assert hit.sum() >= 100 and (~hit).sum() >= 50 and turned.sum() >= 1
    assert same(want["normal"][turned], -n[turned]) and same(want["normal"][hit & ~turned], n[hit & ~turned])
    assert want["inside"][hit].any() and not want["inside"][hit].all() and want["covered"][hit].all()
    assert not want["covered"][~hit].any() and same(want["value"][~hit], np.tile(FALLBACK, (int((~hit).sum()), 1)))
    assert same(want["position"][~hit], np.zeros((int((~hit).sum()), 3)))


@pytest.mark.parametrize("name", RAY_SCENES)
def test_the_ray_forms_pieces_subsets_and_device_form(name, monkeypatch):
    o, d, hits = rays(name)
    vol, bias = scene_volume(name, "half"), 0.5
    want = PV.lookup(vol, d, hits, bias, FALLBACK)
    assert (want["covered"][hits["object"] >= 0] == 0).any()                   # the mask leaves hits uncovered
    g = gpu(name)
    monkeypatch.setenv("RPTGPU_VOLUME_PIECE", "64")
    g.reset_stats()
    assert differing(g.lookup_probe_volume(o, d, vol, normal_bias=bias, fallback=FALLBACK), want, RAY_NAMES) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == -(-len(o) // 64)
    monkeypatch.delenv("RPTGPU_VOLUME_PIECE")
    sub = g.lookup_probe_volume(o, d, vol, normal_bias=bias, fallback=FALLBACK, channels=_abi.RPT_VOLUME_NORMAL | _abi.RPT_VOLUME_COVERED)
    assert sorted(sub) == ["covered", "normal"] and differing(sub, want, ("normal", "covered")) == []
    dvol, to, dev = on_device(vol)
    got = g.lookup_probe_volume(to(o), to(d), dvol, normal_bias=bias, fallback=FALLBACK)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values())
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, want, RAY_NAMES) == []
    got = g.lookup_probe_volume(to(o), to(d), dvol, normal_bias=bias, fallback=FALLBACK, channels=_abi.RPT_VOLUME_VALUE | _abi.RPT_VOLUME_T)
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, want, ("t", "value")) == []


def test_one_channel_of_a_host_caller_in_pieces_of_three(monkeypatch):
    """7 rays in pieces of 3 — the last holds one —, NORMAL alone (not the first channel, three components), against the same
    rays in one piece with every channel: a wrong staging offset, component count or row of the channel table shows"""
    name = "cornell"
    o, d, hits = rays(name)
    hit = hits["object"] >= 0
    idx = np.sort(np.concatenate([np.flatnonzero(hit)[:4], np.flatnonzero(~hit)[:3]]))
    assert len(idx) == 7
    o, d = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    vol, g = scene_volume(name, "half"), gpu(name)
    whole = g.lookup_probe_volume(o, d, vol, normal_bias=0.5, fallback=FALLBACK)
    monkeypatch.setenv("RPTGPU_VOLUME_PIECE", "3")
    g.reset_stats()
    got = g.lookup_probe_volume(o, d, vol, normal_bias=0.5, fallback=FALLBACK, channels=_abi.RPT_VOLUME_NORMAL)
    assert sorted(got) == ["normal"] and differing(got, whole, ("normal",)) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == 3
    assert differing(whole, PV.lookup(vol, d, {k: v[idx] for k, v in hits.items()}, 0.5, FALLBACK), RAY_NAMES) == []


def test_empty_calls_and_refusals_on_a_live_handle():
    g = gpu("cornell")
    vol = volume((3, 2, 2), None)
    none = g.sample_probe_volume(np.zeros((0, 3)), np.zeros((0, 3)), vol)
    assert none["value"].shape == (0, 3) and none["covered"].shape == (0,)
    none = g.lookup_probe_volume(np.zeros((0, 3)), np.zeros((0, 3)), vol)
    assert none["normal"].shape == (0, 3) and none["object"].dtype == np.int32
    pos, nrm = points((3, 2, 2))
    with pytest.raises(rpt_amd.RptGpuError, match="RPT_FLAG_PERSISTENT"):
        g.lookup_probe_volume(pos, nrm, vol, flags=_abi.RPT_FLAG_PERSISTENT)
    with pytest.raises(rpt_amd.RptGpuError, match="a point has VALUE, COVERED and INSIDE only"):
        g.sample_probe_volume(pos, nrm, vol, channels=_abi.RPT_VOLUME_ALL)
    with pytest.raises(rpt_amd.RptGpuError, match="normal_bias is not finite"):
        g.sample_probe_volume(pos, nrm, vol, normal_bias=float("nan"))


# ---- 3. the views form
VIEW_SEED, VIEW_BASE, W, H, SPP = 0x5056, 2, 16, 9, 2
UNBOUND = (0.5, 0.25, 2.0)
VIEW_BIAS = 3.0


def model_frames(oracle, name, binds, vol, ev):
    """the two models fed with views_model's rays, first_hits, hit_surface, the scene's own emittance and
    trace_rays(max_bounces = 0) on the misses -> ((3, H, W, 3), the set of the irradiance's branches at the hits)"""
    g, scene = gpu(name), small_scenes.small(name)[0]
    emit = np.array([ob._material.emittance for ob in scene.objects])
    frames, branches = [], set()
    for v, view in enumerate(LK.the_views(name)):
        samples = []
        for s in range(VIEW_BASE, VIEW_BASE + SPP):
            o, d = (np.ascontiguousarray(a) for a in LK.view_rays(oracle, g, view, VIEW_SEED + v, W, H, s))
            hits = g.first_hits(o, d, channels=HIT_CHANNELS | _abi.RPT_HIT_ALBEDO)
            surf = g.hit_surface(o, d)
            look = L.lookup(surf["object"], surf["primitive"], surf["barycentric"], binds, L.BILINEAR)
            pv = PV.lookup(vol, d, hits, VIEW_BIAS)
            covered, value, branch = PV.irradiance(look["covered"], look["value"], pv["covered"], pv["value"])
            hit = hits["object"] >= 0
            branches |= set(np.unique(branch[hit]).tolist())
            env = np.zeros((W * H, 3))
            if (~hit).any():
                env[~hit] = g.trace_rays(np.ascontiguousarray(o[~hit]), np.ascontiguousarray(d[~hit]), 0, samples=1, seed=1)
            samples.append(L.shade(hit, env, hits["albedo"], emit[np.maximum(hits["object"], 0)], covered, value, UNBOUND))
        frames.append(L.fold(samples, ev))
    return np.stack(frames).reshape(3, H, W, 3), branches


def render(g, name, binds, vol, ev, **kw):
    return g.render_views_probe_lit(LK.the_views(name), W, H, binds, vol, samples=SPP, seed=VIEW_SEED, seed_stride=1,
                                    sample_index_base=VIEW_BASE, exposure_value=ev, normal_bias=VIEW_BIAS,
                                    unbound_irradiance=UNBOUND, **kw)


@pytest.mark.parametrize("case", ["no-bindings", "one-binding", "one-binding-masked-volume"])
def test_the_views_form_is_the_two_models_over_the_header_rays(case, oracle, monkeypatch):
    name, ev = "cornell", 0.5
    binds = [] if case == "no-bindings" else [LK.bindings(name, "large")[0]]
    vol = scene_volume(name, "half" if case.endswith("masked-volume") else None)
    want, branches = model_frames(oracle, name, binds, vol, ev)
    assert branches == {"no-bindings": {1}, "one-binding": {0, 1}, "one-binding-masked-volume": {0, 1, 2}}[case]
    g = gpu(name)
    got = render(g, name, binds, vol, ev)
    assert got.shape == (3, H, W, 3) and got.dtype == np.float64
    for v in range(3):
        assert same(got[v], want[v]), "view %d: %d pixels differ" % (v, (M.bits(got[v]) != M.bits(want[v])).any(axis=-1).sum())
    assert not same(got[0], got[1])
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "31")     # cuts inside a view
    assert same(render(g, name, binds, vol, ev), want)
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    assert same(render(g, name, binds, vol, ev, flags=GENERAL), want)
    dvol, to, dev = on_device(vol)
    dbinds = [rpt_amd.lightmap.Binding(b.object, to(b.uvs), to(b.map), None if b.valid is None else to(b.valid)) for b in binds]
    out = render(g, name, dbinds, dvol, ev)
    assert isinstance(out, torch.Tensor) and out.device == dev and same(out.cpu().numpy(), want)


def test_a_perspective_view_without_bindings_is_the_ray_form_folded_by_hand(oracle):
    name = "cornell"
    g, scene = gpu(name), small_scenes.small(name)[0]
    vol = scene_volume(name, "half")
    cam = LK.the_views(name)[0]
    assert isinstance(cam, Camera)
    emit = np.array([ob._material.emittance for ob in scene.objects])
    samples = []
    for s in range(VIEW_BASE, VIEW_BASE + SPP):
        o, d = (np.ascontiguousarray(a) for a in views_model.perspective_rays(oracle, cam, VIEW_SEED, W, H, s))
        got = g.lookup_probe_volume(o, d, vol, normal_bias=VIEW_BIAS)
        albedo = g.first_hits(o, d, channels=_abi.RPT_HIT_ALBEDO)["albedo"]
        hit = got["object"] >= 0
        env = np.zeros((W * H, 3))
        if (~hit).any():
            env[~hit] = g.trace_rays(np.ascontiguousarray(o[~hit]), np.ascontiguousarray(d[~hit]), 0, samples=1, seed=1)
        value = np.where(got["value"] < 0.0, 0.0, got["value"])
        samples.append(L.shade(hit, env, albedo, emit[np.maximum(got["object"], 0)], got["covered"], value, UNBOUND))
    want = L.fold(samples, 0.0).reshape(H, W, 3)
    frame = g.render_views_probe_lit([cam], W, H, [], vol, samples=SPP, seed=VIEW_SEED, sample_index_base=VIEW_BASE,
                                     normal_bias=VIEW_BIAS, unbound_irradiance=UNBOUND)
    assert frame.shape == (1, H, W, 3) and same(frame[0], want)
    assert not (frame == frame[0, 0, 0]).all()


# ---- 4. the meaning
def test_a_baked_volume_is_bake_probes_and_reads_back_as_sh9_irradiance():
    """At a probe's own position the probe's weight is 1 and the others' 0 up to the rounding of (o + i * h - o) / h, a few
    1e-16, so the call's value is the sum over j of (A_j * Y_j) * c_j in the header's order up to that much of a neighbour's
    coefficients, and sh9_irradiance's is numpy's einsum of the same nine terms: a few 1e-15 of the terms' absolute sum
    between them.  The issue's bound is 1e-12 relative; the scale it is taken against here is the absolute sum of the nine terms
    |A_j Y_j c_j|, NOT the value: where the terms cancel, the two orders of summation differ by roundings of the terms, not of
    what is left of them (DESIGN.md §26 says the same)."""
    name = "cornell"
    g = gpu(name)
    lo, hi = (np.array(x) for x in occ.BOXES[name])
    counts = (3, 3, 3)
    origin, spacing = lo + 0.25 * (hi - lo), 0.25 * (hi - lo)
    vol = ProbeVolume.bake(g, origin, spacing, counts, samples=16, max_bounces=2, seed=0xB0B)
    pos = ProbeVolume.positions(origin, spacing, counts)
    assert pos.shape == (27, 3) and same(pos[(1 * 3 + 2) * 3 + 1], origin + np.array([1.0, 2.0, 1.0]) * spacing)
    direct = g.bake_probes(pos, kind=_abi.RPT_PROBE_SH9, samples=16, max_bounces=2, seed=0xB0B)
    assert vol.coeffs.shape == (27, 9, 3) and same(vol.coeffs, direct) and np.abs(direct).max() > 0.0
    on_dev = ProbeVolume.bake(g, origin, spacing, counts, samples=16, max_bounces=2, seed=0xB0B, device=True)
    assert isinstance(on_dev.coeffs, torch.Tensor) and same(on_dev.coeffs.cpu().numpy(), direct)
    rs = np.random.RandomState(5)
    nrm = rs.normal(size=(27, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    got = g.sample_probe_volume(pos, nrm, vol)
    assert got["covered"].all() and got["inside"].all()
    want = sh9_irradiance(direct, nrm)
    terms = np.abs(rpt_amd.sh9_basis(nrm)[:, :, None] * np.array(PV.A)[None, :, None] * direct).sum(axis=1)
    error = np.abs(got["value"] - want)
    print("read back: max |value - sh9_irradiance| / sum |terms| = %.3e (bound 1e-12), %d of 81 sums are zero"
          % ((error[terms > 0.0] / terms[terms > 0.0]).max(), int((terms == 0.0).sum())))
    assert (terms > 0.0).sum() >= 40 and (error <= 1e-12 * terms).all()        # (a probe inside a box is black: 0 == 0)
    lit = g.render_views_probe_lit([LK.the_views(name)[0]], W, H, [], on_dev, samples=1, seed=1)   # a device volume: a tensor back
    assert isinstance(lit, torch.Tensor) and torch.isfinite(lit).all() and float(lit.max()) > 0.0
