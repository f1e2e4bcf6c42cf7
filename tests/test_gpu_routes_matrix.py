"""The entry points added since the renders, on the routes and the build their own GPU tests do not reach, on a real MI355X:
trace_rays, first_hits, occluded, bake_ao, bake_probes, trace_vertices, render_views (seed stride, seeds, pieces,
RPT_FLAG_VIEWS_PERSISTENT), render_views_aov, render_views_denoised, the device Buffer and the _device forms, each on one small
scene per route (tests/routes_cases.py says which, and why; tests/test_routes_matrix_host.py holds each scene to its route with
the oracle and the scene planner alone).

Every result is held to the chain of truths its own test file uses, by that file's helpers: the oracle's frame for the oracle's
camera rays anchors trace_rays; the header's rays through trace_rays give the probes and the two other projections; closest_hit
— itself the oracle's on the 600 loose rays — and its arithmetic give first_hits, occluded, bake_ao and the feature buffers;
render_views and render_views_aov through tests/denoise_model.py give the denoised views; the oracle's batches through
denoise_model, aov_model and adaptive_model give the device Buffer.  Tolerance 0: arrays are compared on their bytes (a NaN
equals the same NaN, -0.0 differs from +0.0).  One exception, the suite's own (tests/test_gpu_parity.py): where a DEVICE array
stands against an ORACLE array that may hold a NaN — closest_hit's t and normal on monomial's vertical rays — a NaN equals any
NaN, since x86 and gfx950 make different quiet NaNs; every other value is compared on its bits.

What RptStats says about the route is asserted after the calls that run the wavefront pipeline (a render's counters; first_hits
and occluded count one bracket per piece on any route): no per-tree launch on monomial and fractal_spheres, whose re-order
bracket (RPT_K_TREE_SORT) runs; per-tree launches (RPT_K_TREE_TRACE) on fractal_teapots, nested_groups and deep_nest."""
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import DeviceBuffer, GpuScene, _abi
from rpt_amd.color import color_bytes

import adaptive_model
import aov_model
import denoise_model
import routes_cases as RC
import test_gpu_first_hits as FH
import test_gpu_occlusion as occ
import test_gpu_probes as PT
import test_gpu_trace_rays as R
import test_gpu_vertices as VX
import test_gpu_views_denoised as VD
import views_model

pytestmark = pytest.mark.gpu

GENERAL, FLAGGED = _abi.RPT_FLAG_GENERAL_TRAVERSAL, _abi.RPT_FLAG_VIEWS_PERSISTENT
W, H, SPP, BASE, SEEDS = RC.W, RC.H, RC.SPP, RC.BASE, RC.SEEDS
SEEDINGS = {"stride": dict(seed=RC.STRIDE_SEED, seed_stride=RC.STRIDE), "seeds": dict(seeds=SEEDS)}
VIEW_SEEDS = {"stride": tuple(RC.STRIDE_SEED + v * RC.STRIDE for v in range(3)), "seeds": SEEDS}
_handles = {}


def gpu(name, mp):
    """the scene's handle, made once under the environment the scene is in the matrix with"""
    if name not in _handles:
        env = RC.CREATE_ENV.get(name, {})
        for k, v in env.items():
            mp.setenv(k, v)
        _handles[name] = GpuScene(RC.scene(name)[0], 0)
        for k in env:
            mp.delenv(k)
    return _handles[name]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_or_both_nan(device, oracle):
    """a device array against an oracle array: the bits, or a NaN on both sides"""
    device, oracle = np.ascontiguousarray(device), np.ascontiguousarray(oracle)
    if device.shape != oracle.shape or device.dtype != oracle.dtype:
        return False
    return bool(((device.view(np.uint64) == oracle.view(np.uint64)) | (np.isnan(device) & np.isnan(oracle))).all())


def counted(g, call):
    """-> (call's result, RptStats of the call alone)"""
    g.reset_stats()
    out = call()
    return out, g.stats()


def launches(st, kind):
    return int(st.kernel_launches[kind])


def assert_route(name, st, what):
    """the proof RptStats gives after a call through the wavefront pipeline"""
    said = (name, what, [int(x) for x in st.kernel_launches])
    assert launches(st, _abi.RPT_K_RAYGEN) >= 1 and launches(st, _abi.RPT_K_PATHS) == 0, said
    if name in RC.PER_TREE:
        assert launches(st, _abi.RPT_K_TREE_TRACE) > 0, said
    else:
        assert launches(st, _abi.RPT_K_TREE_TRACE) == 0, said
    if name == "fractal_spheres":
        assert launches(st, _abi.RPT_K_TREE_SORT) > 0, said


def pieces(mp, family):
    key, value = RC.PIECES[family]
    mp.setenv(key, value)
    return key


# ---- 1. trace_rays: the anchor
@pytest.mark.parametrize("s", [0, BASE])
@pytest.mark.parametrize("name", RC.SCENES)
def test_trace_rays_gives_the_oracles_frame_for_the_oracles_rays(name, s, monkeypatch):
    p, o, d, streams, draws, want = RC.camera_case(name, s)
    assert (draws == 2).all() and len(o) == W * H
    g = gpu(name, monkeypatch)
    got, st = counted(g, lambda: R.trace(g, p, o, d, streams=streams))
    assert same(got, want), "%s, sample %d: %d of %d rays differ" % (name, s, (got != want).any(axis=1).sum(), len(want))
    assert st.samples == len(o) and st.extend_rays >= len(o)
    assert_route(name, st, "trace_rays")
    if s == 0:
        assert same(R.trace(g, p, o, d, streams=streams, flags=GENERAL), want), name + " under RPT_FLAG_GENERAL_TRAVERSAL"
        perm = np.random.RandomState(77).permutation(len(o))
        assert same(R.trace(g, p, o[perm], d[perm], streams=streams[perm]), want[perm]), name + ", permuted"


# ---- 2. first_hits, occluded, bake_ao
@pytest.mark.parametrize("name", RC.QUERIED)
def test_first_hits_occluded_and_bake_ao(name, monkeypatch):
    scene = RC.scene(name)[0]
    o, d = RC.rays(name)
    g = gpu(name, monkeypatch)
    t, nrm, obj = g.closest_hit(o, d)
    t0, n0, obj0 = RC.oracle_scene(name).closest_hit(o, d)
    assert np.array_equal(obj, obj0) and same_or_both_nan(t, t0) and same_or_both_nan(nrm, n0)
    hit = obj >= 0
    assert hit.mean() >= 0.10 and (~hit).mean() >= 0.10, hit.mean()
    if name == "monomial":
        assert np.isnan(t).any() and hit[np.isnan(t)].all()  # the NaN records are there
    want = FH.model(g, scene, o, d)
    for flags in (0, GENERAL):
        got, st = counted(g, lambda: g.first_hits(o, d, flags=flags))
        assert FH.differing(got, want) == [], (name, flags)
        assert launches(st, _abi.RPT_K_EXTEND) == 1 and launches(st, _abi.RPT_K_PATHS) == 0 and st.samples == 0
    max_t = RC.max_t(name, t)
    with np.errstate(invalid="ignore"):
        stops = (~(t > np.fmin(max_t, occ.DBL_MAX))).astype(np.uint8)
        any_hit = (~(t > occ.DBL_MAX)).astype(np.uint8)
    assert stops.mean() >= 0.10 and (1 - stops).mean() >= 0.10, stops.mean()
    for flags in (0, GENERAL):
        got, st = counted(g, lambda: g.occluded(o, d, max_t, flags=flags))
        assert same(got, stops), (name, flags, np.flatnonzero(got != stops)[:8])
        assert st.shadow_rays == RC.N_RAYS and launches(st, _abi.RPT_K_SHADOW) >= 1 and launches(st, _abi.RPT_K_PATHS) == 0
        assert same(g.occluded(o, d, flags=flags), any_hit), (name, flags)
    # ambient occlusion: the directions of RPT_PROBE_IRRADIANCE through closest_hit, folded in the header's order
    pos, normals, ids = RC.points(name)
    S = RC.AO_SAMPLES
    dirs, _ = PT.directions(PT.IRR, normals, ids, occ.SEED, S, 0)
    ts = g.closest_hit(np.repeat(pos, S, axis=0), dirs.reshape(-1, 3))[0].reshape(RC.N_POINTS, S)
    folds = {far: occ.fold(dirs, ts, far) for far in (math.inf, RC.half_diagonal(name))}
    assert not (folds[math.inf][0] == 0.0).all() and not (folds[math.inf][0] == 1.0).all()
    bake = lambda far, **kw: g.bake_ao(pos, normals, samples=S, seed=occ.SEED, max_distance=far, streams=ids, bent_normals=True, **kw)
    for far, (want_ao, want_bent) in folds.items():
        for flags in (0, GENERAL):
            ao, bent = bake(far, flags=flags)
            assert same(ao, want_ao) and same(bent, want_bent), (name, far, flags)
    # in pieces: three of the 600 rays, the last with 88
    key = pieces(monkeypatch, "hits")
    got, st = counted(g, lambda: g.first_hits(o, d))
    assert FH.differing(got, want) == [] and launches(st, _abi.RPT_K_EXTEND) == 3, name
    monkeypatch.delenv(key)
    key = pieces(monkeypatch, "occlusion")
    assert same(g.occluded(o, d, max_t), stops), name
    ao, bent = bake(RC.half_diagonal(name))
    assert same(ao, folds[RC.half_diagonal(name)][0]) and same(bent, folds[RC.half_diagonal(name)][1]), name
    monkeypatch.delenv(key)


# ---- 3. bake_probes
@pytest.mark.parametrize("kind_name", sorted(PT.KINDS))
@pytest.mark.parametrize("name", RC.QUERIED)
def test_bake_probes_are_the_headers_rays_through_trace_rays(name, kind_name, monkeypatch):
    kind = PT.KINDS[kind_name]
    _, _, bounces, seed = RC.scene(name)
    pos, normals, ids = RC.points(name)
    g = gpu(name, monkeypatch)
    want, _, draws = PT.restated(g, kind, pos, normals, ids, bounces, seed, RC.PROBE_SAMPLES)
    assert len(set(draws.ravel().tolist())) >= 2 and np.isfinite(want).all() and (want != 0.0).any()
    bake = lambda: g.bake_probes(pos, normals if kind == PT.IRR else None, kind=kind, samples=RC.PROBE_SAMPLES, max_bounces=bounces,
                                 seed=seed, streams=ids)
    got, st = counted(g, bake)
    assert same(got, want), "%s, %s: %d of %d probes differ" % (name, kind_name, (got != want).reshape(RC.N_POINTS, -1).any(axis=1).sum(), RC.N_POINTS)
    assert st.samples == RC.N_POINTS * RC.PROBE_SAMPLES
    assert_route(name, st, "bake_probes")
    key = pieces(monkeypatch, "probes")  # six pieces, the last of one probe
    got, st = counted(g, bake)
    monkeypatch.delenv(key)
    assert same(got, want) and launches(st, _abi.RPT_K_RAYGEN) >= (RC.N_POINTS + 2) // 3, name


# ---- 4. trace_vertices
@pytest.mark.parametrize("name", RC.SCENES)
def test_trace_vertices_every_channel(name, monkeypatch):
    p, o, d, streams, draws, frame = RC.camera_case(name, BASE)
    bounces = p.max_bounces
    g = gpu(name, monkeypatch)
    kw = dict(samples=SPP, seed=p.seed, sample_index_base=BASE, streams=streams, first_draw=2)
    v, st = counted(g, lambda: g.trace_vertices(o, d, bounces, **kw))
    assert st.samples == len(o) * SPP
    assert_route(name, st, "trace_vertices")
    # rgb is trace_rays', and one sample of it the oracle's frame
    assert same(v.rgb, g.trace_rays(o, d, bounces, **kw)), name
    one = g.trace_vertices(o, d, bounces, channels=_abi.RPT_VERTEX_RGB | _abi.RPT_VERTEX_LENGTH, **dict(kw, samples=1))
    assert same(one.rgb, frame) and same(one.length, np.ascontiguousarray(v.length[:, :1])), name
    # the header's fold of the exported factors is rgb
    n, S, V = v.t.shape
    assert (S, V) == (SPP, bounces + 1) and v.length.dtype == np.uint32 and v.length.min() >= 1 and v.length.max() <= V
    assert (v.length >= 3).any(), name  # paths go past the first hit
    L, acc = VX.fold(v)
    assert same(acc / SPP * 2.0 ** 0.0, v.rgb), "%s: %d rays differ" % (name, (acc / SPP != v.rgb).any(axis=1).sum())
    # every vertex is first_hits of the ray that ends there, and that ray starts where the vertex before it lies
    depth = np.arange(V)[None, None, :]
    valid = depth < v.length[:, :, None]
    assert (v.draw[:, :, 0] == 2).all() and same(v.direction[:, :, 0], np.broadcast_to(d[:, None, :], (n, S, 3)).copy())
    origin = np.concatenate([np.broadcast_to(o[:, None, None, :], (n, S, 1, 3)), v.position[:, :, :-1]], axis=2)
    assert (v.object[valid & (depth < v.length[:, :, None] - 1)] >= 0).all()
    hit = g.first_hits(origin[valid], v.direction[valid],
                       channels=_abi.RPT_HIT_T | _abi.RPT_HIT_NORMAL | _abi.RPT_HIT_OBJECT | _abi.RPT_HIT_POSITION)
    got = {k: getattr(v, k)[valid] for k in ("t", "normal", "object", "position")}
    assert VX.differing(got, hit) == [], "%s: of %d vertices" % (name, valid.sum())
    reached = np.isin(got["object"], RC.COUNTED[name])
    assert reached.mean() >= 0.5 * RC.SHARE, reached.mean()  # (vertices on the objects the scene is here for)
    # behind a path's last vertex: +0.0, draw 0, object -1; at the last vertex the three factors are +0.0
    behind = ~valid
    assert behind.any()
    for k in VX.PER_VERTEX:
        a = getattr(v, k)[behind]
        assert (a == -1).all() if k == "object" else not VX.bits(a).any(), (name, k)
    last = depth == v.length[:, :, None] - 1
    for k in ("bsdf", "inv_pdf", "abs_cos"):
        assert not VX.bits(getattr(v, k)[last]).any(), (name, k)
    assert VX.differing(g.trace_vertices(o, d, bounces, flags=GENERAL, **kw), v) == [], name


# ---- 5. render_views: seed stride, seeds, pieces, RPT_FLAG_VIEWS_PERSISTENT
def headers_rays(oracle, g, view, seed, s):
    if view.projection == _abi.RPT_VIEW_ORTHOGRAPHIC:
        return views_model.orthographic_rays(oracle, view.camera, view.ortho_scale, seed, W, H, s)
    return views_model.panorama_rays(oracle, view.camera.eye, seed, W, H, s, views_model.device_sincos(g))[:2]


@pytest.mark.parametrize("seeding", sorted(SEEDINGS))
@pytest.mark.parametrize("name", RC.SCENES)
def test_render_views_every_projection(name, seeding, oracle, monkeypatch):
    _, _, bounces, _ = RC.scene(name)
    views = RC.views(name)
    g = gpu(name, monkeypatch)
    kw = dict(samples=SPP, sample_index_base=BASE, **SEEDINGS[seeding])
    got, st = counted(g, lambda: g.render_views(views, W, H, bounces, **kw))
    assert got.shape == (3, H, W, 3) and got.dtype == np.float64 and st.samples == 3 * W * H * SPP
    assert_route(name, st, "render_views")
    seeds = VIEW_SEEDS[seeding]
    # the perspective view (under a lens) is the oracle's frame of its camera
    want = RC.view_frame(name, seeds[0])
    assert same(got[0].reshape(-1, 3), want), "%s, %s: %d pixels of view 0 differ" % (name, seeding, (got[0].reshape(-1, 3) != want).any(axis=1).sum())
    # the orthographic view and the panorama are the header's rays through trace_rays, folded in sample order
    pixels = np.arange(W * H, dtype=np.uint32)
    for v in (1, 2):
        acc = np.zeros((W * H, 3))
        for s in range(BASE, BASE + SPP):
            ro, rd = headers_rays(oracle, g, views[v], seeds[v], s)
            acc = acc + g.trace_rays(ro, rd, bounces, samples=1, seed=seeds[v], sample_index_base=s, streams=pixels, first_draw=2,
                                     exposure_value=0.0)
        want = acc / float(SPP)
        assert same(got[v].reshape(-1, 3), want), "%s, %s: %d pixels of view %d differ" % (name, seeding, (got[v].reshape(-1, 3) != want).any(axis=1).sum(), v)
        assert not (acc == acc[0]).all()  # (it does see something)
    # in pieces of 500 indices: the second ends inside view 1, which has another seed than view 0
    key = pieces(monkeypatch, "views")
    in_pieces, st = counted(g, lambda: g.render_views(views, W, H, bounces, **kw))
    monkeypatch.delenv(key)
    assert same(in_pieces, got) and launches(st, _abi.RPT_K_RAYGEN) >= (3 * W * H + 499) // 500, (name, seeding)
    # on request in the persistent path kernel — which a scene with a group of trees cannot honour (api_views.cpp): the same bytes
    flagged, st = counted(g, lambda: g.render_views(views, W, H, bounces, flags=FLAGGED, **kw))
    assert same(flagged, got), "%s, %s, flagged: %s pixels differ" % (name, seeding, [int((flagged[v] != got[v]).any(axis=-1).sum()) for v in range(3)])
    said = (name, seeding, [int(x) for x in st.kernel_launches])
    if name in RC.PER_TREE:
        assert launches(st, _abi.RPT_K_PATHS) == 0 and launches(st, _abi.RPT_K_TREE_TRACE) > 0, said
    else:
        assert launches(st, _abi.RPT_K_PATHS) > 0 and launches(st, _abi.RPT_K_RAYGEN) == 0, said
    assert st.samples == 3 * W * H * SPP
    assert same(g.render_views(views, W, H, bounces, flags=GENERAL, **kw), got), (name, seeding)


# ---- 6. render_views_aov
@pytest.mark.parametrize("seeding", sorted(SEEDINGS))
@pytest.mark.parametrize("name", RC.QUERIED)
def test_render_views_aov_every_projection(name, seeding, oracle, monkeypatch):
    scene = RC.scene(name)[0]
    views = RC.views(name)
    g = gpu(name, monkeypatch)
    kw = dict(samples=SPP, sample_index_base=BASE, **SEEDINGS[seeding])
    got = g.render_views_aov(views, W, H, **kw)
    seeds = VIEW_SEEDS[seeding]
    assert got["hits"].shape == (3, H, W) and got["hits"].max() == SPP and (got["hits"] < SPP).any()
    # the perspective view: the oracle's camera rays and closest hits, folded (tests/aov_model.py)
    p = RC.view_params(name, seeds[0])
    want = aov_model.full_frame(aov_model.expected(scene, views[0], p, oracle_scene=RC.oracle_scene(name)), p)
    assert aov_model.mismatches({k: a[0] for k, a in got.items()}, want) == [], (name, seeding)
    # the two other projections: the header's rays through closest_hit, folded per pixel in ascending sample order
    col = aov_model.colors(scene)
    n = W * H
    for v in (1, 2):
        o, d = np.empty((n, SPP, 3)), np.empty((n, SPP, 3))
        for k, s in enumerate(range(BASE, BASE + SPP)):
            o[:, k], d[:, k] = headers_rays(oracle, g, views[v], seeds[v], s)
        t, nrm, obj = g.closest_hit(o.reshape(-1, 3), d.reshape(-1, 3))
        t, nrm, obj = t.reshape(n, SPP), nrm.reshape(n, SPP, 3), obj.reshape(n, SPP)
        want = {"hits": np.zeros(n, dtype=np.uint32), "depth": np.zeros(n), "normal": np.zeros((n, 3)), "albedo": np.zeros((n, 3)),
                "position": np.zeros((n, 3)), "object": np.zeros(n, dtype=np.int32)}
        with np.errstate(all="ignore"):
            for j in range(n):
                (want["hits"][j], want["depth"][j], want["normal"][j], want["albedo"][j], want["position"][j],
                 want["object"][j]) = aov_model.fold(o[j], d[j], t[j], nrm[j], obj[j], col)
        mine = {k: a[v].reshape(want[k].shape) for k, a in got.items()}
        assert aov_model.mismatches(mine, want) == [], (name, seeding, v)
        assert 0 < want["hits"].sum() and np.isin(want["object"], RC.COUNTED[name]).any()
    key = pieces(monkeypatch, "views")
    assert aov_model.mismatches(g.render_views_aov(views, W, H, **kw), got) == [], (name, seeding)
    monkeypatch.delenv(key)
    assert aov_model.mismatches(g.render_views_aov(views, W, H, flags=GENERAL, **kw), got) == [], (name, seeding)


# ---- 7. render_views_denoised
@pytest.mark.parametrize("name", RC.QUERIED)
def test_render_views_denoised_is_the_model(name, monkeypatch):
    assert (VD.SPP, VD.BATCHES, VD.BASE, VD.FSPP, VD.FBASE, VD.SEEDS) == (SPP, RC.BATCHES, BASE, RC.FSPP, RC.FBASE, SEEDS)
    monkeypatch.setattr(VD, "BOUNCES", RC.scene(name)[2])  # that file's call and model, at the scene's own max_bounces
    views = RC.views(name)
    g = gpu(name, monkeypatch)
    got = VD.call(g, views, W, H, seeds=SEEDS, levels=RC.LEVELS, want=VD.ALL)
    want = VD.model(g, views, W, H, SEEDS, levels=RC.LEVELS)
    for k in ("mean", "variance", "denoised"):
        for v in range(3):
            assert VD.same(got[k][v], want[k][v]), "%s: %s of view %d: %d values differ" % (name, k, v, (denoise_model.bits(got[k][v]) != denoise_model.bits(want[k][v])).sum())
    assert got["rgb8"].dtype == np.uint8 and np.array_equal(got["rgb8"], color_bytes(got["denoised"]))
    assert not VD.same(got["denoised"], got["mean"]) and np.isfinite(got["denoised"]).all()
    key = pieces(monkeypatch, "views")
    assert VD.same_all(VD.call(g, views, W, H, seeds=SEEDS, levels=RC.LEVELS, want=VD.ALL), got), name
    monkeypatch.delenv(key)


# ---- 8. the device Buffer
@pytest.mark.parametrize("name", RC.BUFFERED)
def test_the_device_buffer_is_the_host_buffer_of_the_oracles_batches(name, monkeypatch):
    scene = RC.scene(name)[0]
    lens = RC.views(name)[0]
    seed = SEEDS[0]
    frames = [RC.view_frame(name, seed, BASE + b * SPP) for b in range(RC.BATCHES)]  # the oracle's
    g = gpu(name, monkeypatch)
    buf = DeviceBuffer(g, W, H)
    host = rpt_amd.Buffer(W, H, rpt_amd.Filter.Box(0))
    for b in range(2):
        buf.sample(lens, RC.view_params(name, seed, BASE + b * SPP))
        for pix in range(W * H):
            host.add_sample(pix % W, pix // W, frames[b][pix])
    total, counts, M2 = denoise_model.welford([f.reshape(H, W, 3) for f in frames[:2]])
    assert same(buf.totals(), total) and (buf.sample_counts() == 2).all() and buf.num_batches() == 2, name
    assert np.array_equal(buf.image(), host.image()), name
    # the features are the oracle's first hits, folded
    fp = RC.view_params(name, seed, RC.FBASE, RC.FSPP)
    buf.features(lens, fp)
    feats = buf.feature_sums()
    model = aov_model.full_frame(aov_model.expected(scene, lens, fp, oracle_scene=RC.oracle_scene(name)), fp)
    assert feats["hits"].sum() > 0 and aov_model.mismatches(feats, {k: model[k] for k in feats}) == [], name
    # the filter is the model's on the oracle's state
    want = denoise_model.denoise(total, counts, M2, {k: model[k] for k in feats}, levels=RC.LEVELS)
    got = buf.denoise(levels=RC.LEVELS)
    assert same(got, want), "%s: %d values differ" % (name, (denoise_model.bits(got) != denoise_model.bits(want)).sum())
    assert np.array_equal(buf.denoised_image(levels=RC.LEVELS), color_bytes(want)) and not same(got, total / 2.0)
    # one adaptive round on top of the two plain batches: every pixel gets the third batch, then the rule speaks (n = 3)
    left = buf.sample_adaptive(lens, RC.view_params(name, seed, BASE + 2 * SPP), min_batches=2, abs_tol=0.0, rel_tol=RC.ADAPTIVE_REL_TOL)
    r = adaptive_model.run(frames, 3, 0.0, RC.ADAPTIVE_REL_TOL)
    print("%s: %d of %d pixels stay active after the adaptive round" % (name, left, W * H))
    adaptive_model.check_against(buf, [W * H, W * H, left], frames, r)
    assert 0 < r["active"][-1] < W * H  # (tests/test_routes_matrix_host.py: a mix)
    buf.close()


# ---- 9. the _device forms
@pytest.mark.parametrize("name", RC.DEVICE_FORMS)
def test_device_forms_give_the_host_forms_bytes(name, monkeypatch):
    g = gpu(name, monkeypatch)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a writable, contiguous copy of the shared arrays)
    p, o, d, streams, draws, frame = RC.camera_case(name, 0)
    got = R.trace(g, p, to(o), to(d), streams=to(streams.astype(np.int32)))
    assert isinstance(got, torch.Tensor) and got.device == dev and same(got.cpu().numpy(), frame), name
    ro, rd = RC.rays(name)
    host = g.first_hits(ro, rd)
    for flags in (0, GENERAL):
        got = g.first_hits(to(ro), to(rd), flags=flags)
        assert all(isinstance(a, torch.Tensor) and a.device == dev for a in got.values())
        assert FH.differing({k: a.cpu().numpy() for k, a in got.items()}, host) == [], (name, flags)
    monkeypatch.setattr(VD, "BOUNCES", RC.scene(name)[2])
    views = RC.views(name)
    host = VD.call(g, views, W, H, seeds=SEEDS, levels=RC.LEVELS, want=VD.ALL)
    got = VD.call(g, views, W, H, seeds=SEEDS, levels=RC.LEVELS, want=VD.ALL, out="torch")
    assert all(a.is_cuda for a in got.values()) and VD.same_all({k: a.cpu().numpy() for k, a in got.items()}, host), name


# ---- the per-depth path re-order, really sorting, is scheduling only
def test_the_path_sort_changes_no_byte(monkeypatch):
    """fractal_spheres with the sort on from one path up against a handle made with RPTGPU_PATH_REORDER=0: trace_rays, both
    kinds of probes, every channel of trace_vertices and the seeded views — whose seeds_out and ids_out stand beside the
    permuted rows — give the same bytes, with and without the re-order's bracket in RptStats"""
    name = "fractal_spheres"
    _, _, bounces, seed = RC.scene(name)
    g = gpu(name, monkeypatch)
    for k, v in RC.UNSORTED_ENV.items():
        monkeypatch.setenv(k, v)
    plain = GpuScene(RC.scene(name)[0], 0)
    for k in RC.UNSORTED_ENV:
        monkeypatch.delenv(k)
    p, o, d, streams, draws, frame = RC.camera_case(name, 0)
    pos, normals, ids = RC.points(name)
    views = RC.views(name)
    vkw = dict(samples=SPP, seed=p.seed, sample_index_base=BASE, streams=streams, first_draw=2)
    calls = {
        "trace_rays": lambda h: {"rgb": R.trace(h, p, o, d, streams=streams)},
        "bake_probes sh9": lambda h: {"sh": h.bake_probes(pos, kind=PT.SH9, samples=RC.PROBE_SAMPLES, max_bounces=bounces, seed=seed, streams=ids)},
        "bake_probes irradiance": lambda h: {"e": h.bake_probes(pos, normals, kind=PT.IRR, samples=RC.PROBE_SAMPLES, max_bounces=bounces, seed=seed, streams=ids)},
        "trace_vertices": lambda h: h.trace_vertices(o, d, bounces, **vkw).arrays(),
        "render_views, seeds": lambda h: {"frames": h.render_views(views, W, H, bounces, samples=SPP, sample_index_base=BASE, seeds=SEEDS)},
        "render_views, stride": lambda h: {"frames": h.render_views(views, W, H, bounces, samples=SPP, sample_index_base=BASE, **SEEDINGS["stride"])},
    }
    try:
        for what, call in calls.items():
            sorted_, st = counted(g, lambda: call(g))
            unsorted, st0 = counted(plain, lambda: call(plain))
            assert launches(st, _abi.RPT_K_TREE_SORT) > 0 and launches(st0, _abi.RPT_K_TREE_SORT) == 0, what
            assert launches(st, _abi.RPT_K_TREE_TRACE) == 0 and launches(st0, _abi.RPT_K_TREE_TRACE) == 0, what
            assert VX.differing(sorted_, unsorted) == [], what
    finally:
        plain.close()
