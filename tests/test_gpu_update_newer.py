"""The entry points added since tests/test_gpu_update_matrix.py was written — hit_surface, bake_lightmap (irradiance, AO,
the raw channels), filter_lightmap, bake_direct, bake_lightmap_direct, bake_probes, trace_rays, trace_vertices, their _device
forms, and the three requests for the persistent path kernel (RPT_FLAG_RAYS_PERSISTENT for rays and probes,
RPT_FLAG_VIEWS_PERSISTENT, RPT_FLAG_VERTICES_PERSISTENT) — on a handle that has been UPDATED, on a real MI355X.  The contract
is DESIGN.md §9's: after set_objects, set_lights, update, set_mesh or set_group every result is, bit for bit, that of a fresh
handle of the updated scene.

One test per case of tests/update_cases.py, on one handle g, as in the matrix:
  1. warm: every call on g at the final sizes, on the scene as it is BEFORE any update — rpt_hit_surface's columns, the
     lightmap's compacted arrays, the shadow queues and the persistent kernel's buffers are the creation's;
  2. per step: the step's update, every call on g again and on f, a fresh handle of the step's scene with g's options: every
     array equal on its bytes (tolerance 0; a NaN equals the same NaN, -0.0 differs from +0.0).  On g itself: hit_surface's t
     and object are closest_hit's and the triangle a ray names reproduces t and the weights (surface_model.restate on the
     step's scene); the lightmap's raw channels are tests/lightmap_model.py's, its dilated maps the model's dilation of its
     undilated ones; filter_lightmap is tests/lightmap_filter_model.py's of the same arrays; bake_lightmap_direct at the
     owned texels is bake_direct at the bake's own position and normal channels; a flagged call's bytes are the unflagged
     call's, a _device form's the host form's, RPT_FLAG_GENERAL_TRAVERSAL's the default route's;
  3. the update is seen, by the shares tests/test_update_cases_host.py measures with the oracle: hit_surface's t differs from
     the warm one on at least half the oracle's share where the case moves geometry; for lights and materials hit_surface
     and the lightmap's geometry channels and AO keep the warm bytes, and for lights irradiance, probes and trace_rays differ;
     bake_direct differs or not as update_cases.DIRECT_CHANGES says; the lightmap's four raw channels keep the warm bytes at
     every step of every case (they do not read the scene);
  4. the last step returns to the creation's scene: every result has the warm bytes.

The route of each flagged call, from RptStats: RPT_K_PATHS launches are equal on g and on f at every step, and more than
none wherever the scene has no object for the per-tree pipeline only (tree_kids) — every case's creation, and every step but
one: no group here holds a tree (GU.ROUTES' two routes differ in how G itself is walked, and use_wavefront reads tree_kids
alone), and only mesh_past_fast_stacks' `clustered` rebuilds a tree beyond fast_max_depth.  There reroute_object raises
tree_kids: a flagged call that ran rpt_paths_* before the step runs none after it, on g as on f — RPT_K_TREE_TRACE counts the
wavefront pipeline's per-tree launches instead —, the request dropped, not refused, the bytes still the fresh handle's."""
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

from rpt_amd import GpuScene, _abi

import lightmap_filter_model as F
import lightmap_model as LM
import surface_model as SM
import update_cases as C
from test_gpu_update_matrix import differing, put, same

pytestmark = pytest.mark.gpu

GENERAL = _abi.RPT_FLAG_GENERAL_TRAVERSAL
RAYS_P, VIEWS_P, VERTICES_P = _abi.RPT_FLAG_RAYS_PERSISTENT, _abi.RPT_FLAG_VIEWS_PERSISTENT, _abi.RPT_FLAG_VERTICES_PERSISTENT
PATHS, TREE_TRACE = _abi.RPT_K_PATHS, _abi.RPT_K_TREE_TRACE
SH9, IRR = _abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE
ALL = _abi.RPT_LIGHTMAP_ALL
W, H, BOUNCES, SPP, BASE, SEEDS, SEED = C.W, C.H, C.BOUNCES, C.SPP, C.BASE, C.SEEDS, C.NEWER_SEED
RAW_NAMES = ("owner", "barycentric", "position", "normal")
ROUTES = (("default", 0), ("general", GENERAL))
FLAGGED = ("probes/sh9", "probes/irradiance", "rays", "views", "vertices")
assert _abi.rays_persistent_supported() and _abi.views_persistent_supported() and _abi.vertices_persistent_supported()


def counted(h, routes, key, call):
    """the call's result; routes[key] = its (RPT_K_PATHS, RPT_K_TREE_TRACE) launches"""
    h.reset_stats()
    result = call()
    k = h.stats().kernel_launches
    routes[key] = (int(k[PATHS]), int(k[TREE_TRACE]))
    return result


def filter_kw(name):
    """2 levels; a tap a texel away weighs about exp(-1/4) on every chart (their texels are 1/11 of the aim box wide)"""
    lo, hi = C.cases()[name].aim[0]
    return dict(sigma_distance=2.0 * (hi[0] - lo[0]) / 11.0, sigma_plane=C.points(name)[3], levels=2)


def calls(h, c, mp):
    """every call of the docstring on handle h -> ({name: array}, {flagged call: (RPT_K_PATHS, RPT_K_TREE_TRACE) launches})"""
    out, routes = {}, {}
    o, d, _ = C.rays(c.name)
    pos, nrm, ids, half = C.points(c.name)
    ray_ids, lm_base = C.streams(c.name)
    tris, uvs, w, h_, offset = C.chart(c.name)
    views = C.views(c.name)
    lm = dict(channels=ALL, samples=C.LM_SAMPLES, max_bounces=BOUNCES, seed=SEED, offset=offset, stream_base=lm_base, sample_index_base=BASE)
    dk = dict(samples=C.DIRECT_SAMPLES, seed=SEED, sample_index_base=BASE)
    for word, flags in ROUTES:
        put(out, "surface/%s" % word, h.hit_surface(o, d, flags=flags))
        for reach, far in (("inf", math.inf), ("half", half)):
            put(out, "lightmap/%s/%s" % (word, reach), h.bake_lightmap(tris, uvs, w, h_, dilate=2, max_distance=far, flags=flags, **lm))
        out["direct/%s" % word] = h.bake_direct(pos, nrm, streams=ids, flags=flags, **dk)
        out["lightmap_direct/%s" % word] = h.bake_lightmap_direct(tris, uvs, w, h_, offset=offset, dilate=2, stream_base=lm_base, flags=flags, **dk)
    mp.setenv("RPTGPU_SURFACE_PIECE", "256")  # three pieces, the last with 88 rays
    put(out, "surface/pieces", h.hit_surface(o, d))
    mp.delenv("RPTGPU_SURFACE_PIECE")
    plain = h.bake_lightmap(tris, uvs, w, h_, dilate=0, **lm)
    put(out, "lightmap/undilated", plain)
    out["filter"] = h.filter_lightmap(plain["irradiance"], plain["owner"], plain["position"], plain["normal"], **filter_kw(c.name))
    pk = dict(samples=C.PROBE_SAMPLES, max_bounces=BOUNCES, seed=SEED, sample_index_base=BASE, streams=ids)
    for word, kind, normals in (("sh9", SH9, None), ("irradiance", IRR, nrm)):
        for route, flags in ROUTES:
            out["probes/%s/%s" % (word, route)] = h.bake_probes(pos, normals, kind=kind, flags=flags, **pk)
        out["probes/%s/persistent" % word] = counted(h, routes, "probes/" + word, lambda: h.bake_probes(pos, normals, kind=kind, flags=RAYS_P, **pk))
    rk = dict(samples=SPP, seed=SEED, sample_index_base=BASE, streams=ray_ids)
    for route, flags in ROUTES:
        out["rays/%s" % route] = h.trace_rays(o, d, BOUNCES, flags=flags, **rk)
    out["rays/persistent"] = counted(h, routes, "rays", lambda: h.trace_rays(o, d, BOUNCES, flags=RAYS_P, **rk))
    vk = dict(samples=SPP, seeds=SEEDS, sample_index_base=BASE)
    out["views/default"] = h.render_views(views, W, H, BOUNCES, **vk)
    out["views/persistent"] = counted(h, routes, "views", lambda: h.render_views(views, W, H, BOUNCES, flags=VIEWS_P, **vk))
    put(out, "vertices/default", h.trace_vertices(o, d, BOUNCES, **rk).arrays())
    put(out, "vertices/persistent", counted(h, routes, "vertices", lambda: h.trace_vertices(o, d, BOUNCES, flags=VERTICES_P, **rk)).arrays())
    if c.device:
        to = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")  # (a writable, contiguous copy of the shared arrays)
        put(out, "surface/device", h.hit_surface(to(o), to(d)))
        out["direct/device"] = h.bake_direct(to(pos), to(nrm), streams=to(ids.astype(np.int64)), **dk).cpu().numpy()
        put(out, "lightmap/device/inf", h.bake_lightmap(to(tris), to(uvs), w, h_, dilate=2, **lm))
    assert sorted(routes) == sorted(FLAGGED)
    return out, routes


def group(out, prefix):
    return {k[len(prefix) + 1:]: a for k, a in out.items() if k.startswith(prefix + "/")}


def on_the_handle_itself(h, c, scene, out, what):
    """2. of the docstring, the part that needs no second handle: `out` is calls(h)'s, `scene` the scene h holds now"""
    o, d, _ = C.rays(c.name)
    # a route, a flag, pieces and device arrays change no bit
    for prefix, others in (("surface/default", ["surface/general", "surface/pieces"] + ["surface/device"] * c.device),
                           ("lightmap/default/inf", ["lightmap/general/inf"] + ["lightmap/device/inf"] * c.device),
                           ("lightmap/default/half", ["lightmap/general/half"]), ("vertices/default", ["vertices/persistent"])):
        for other in others:
            assert differing(group(out, other), group(out, prefix)) == [], (what, other)
    for key, others in (("direct/default", ["direct/general"] + ["direct/device"] * c.device), ("lightmap_direct/default", ["lightmap_direct/general"]),
                        ("probes/sh9/default", ["probes/sh9/general", "probes/sh9/persistent"]), ("rays/default", ["rays/general", "rays/persistent"]),
                        ("probes/irradiance/default", ["probes/irradiance/general", "probes/irradiance/persistent"]),
                        ("views/default", ["views/persistent"])):
        for other in others:
            assert same(out[other], out[key]), (what, other)
    # hit_surface: t and object are closest_hit's; the named triangle reproduces t and the weights
    got = group(out, "surface/default")
    t, _, obj = h.closest_hit(o, d)
    assert same(got["t"], t) and same(got["object"], obj), what
    idx, _, time, uvw, _ = SM.restate(scene, o, d, obj, got["child"], got["primitive"])
    assert len(idx) == (got["primitive"] >= 0).sum(), what
    if len(idx):
        assert SM.same(time, t[idx]) and SM.same(uvw, got["barycentric"][idx]) and (uvw >= 0.0).all(), what
    # the lightmap: the model's raster; the dilation is the model's of the undilated maps; the reach matters
    plain = group(out, "lightmap/undilated")
    raw, owned = C.chart_texels(c.name)[:2]
    assert differing({k: plain[k] for k in RAW_NAMES}, raw) == [], what
    for reach in ("inf", "half"):
        m = group(out, "lightmap/default/" + reach)
        assert differing({k: m[k] for k in RAW_NAMES}, raw) == [], (what, reach)
    m = group(out, "lightmap/default/inf")
    for k in ("irradiance", "ao"):
        assert same(m[k], LM.dilate(plain[k], owned, 2)[0]), (what, k)
    assert ((plain["ao"][owned] >= 0.0) & (plain["ao"][owned] <= 1.0)).all(), what
    # filter_lightmap: the model's of the same arrays
    want = F.filter_lightmap(plain["irradiance"], plain["owner"], plain["position"], plain["normal"], **filter_kw(c.name))
    assert same(out["filter"], want), what
    if (plain["irradiance"] != 0.0).any():  # (mesh_from_two_leaves' creation leaves the chart dark: its 4 samples a texel find no light)
        assert not same(out["filter"], plain["irradiance"]), what
    # bake_lightmap_direct: bake_direct at the bake's own gather points, normals and stream ids, where a texel is owned
    ys, xs = np.nonzero(owned)
    at = h.bake_direct(np.ascontiguousarray(plain["position"][owned]), np.ascontiguousarray(plain["normal"][owned]), samples=C.DIRECT_SAMPLES,
                       seed=SEED, sample_index_base=BASE, streams=(C.streams(c.name)[1] + ys * C.LM_W + xs).astype(np.uint32))
    assert same(out["lightmap_direct/default"][owned], at), what
    return len(idx)


def raw_keys(out):
    return [k for k in out if k.startswith("lightmap/") and k.split("/")[-1] in RAW_NAMES]


def seen(c, step, warm, got):
    """3. of the docstring -> the figures as a line of text"""
    floor = C.shares(c.name)[step.name]
    t = C.share(warm["surface/default/t"], got["surface/default/t"])
    prim = C.share(warm["surface/default/primitive"], got["surface/default/primitive"])
    ao = C.share(warm["lightmap/undilated/ao"].reshape(-1, 1), got["lightmap/undilated/ao"].reshape(-1, 1))
    irr = C.share(warm["lightmap/undilated/irradiance"].reshape(-1, 3), got["lightmap/undilated/irradiance"].reshape(-1, 3))
    direct = C.share(warm["direct/default"], got["direct/default"])
    said = "%s, %s: the oracle's share of hit distances that change %.1f %%; hit_surface's t differs on %.1f %% of the rays, its primitive on " \
           "%.1f %%; the lightmap's ao differs on %.1f %% of the texels, its irradiance on %.1f %%; bake_direct on %.1f %% of the points (the " \
           "table: %s)" % (c.name, step.name, 100.0 * floor["t"], 100.0 * t, 100.0 * prim, 100.0 * ao, 100.0 * irr, 100.0 * direct,
                          C.DIRECT_CHANGES[c.name][step.name])
    assert differing({k: got[k] for k in raw_keys(got)}, {k: warm[k] for k in raw_keys(warm)}) == [], said
    assert (direct > 0.0) == C.DIRECT_CHANGES[c.name][step.name], said
    if c.moves:
        assert floor["t"] >= 0.05 and t >= 0.5 * floor["t"], said
    else:  # lights, materials: no answer about where a ray ends changes
        keep = [k for k in warm if k.startswith("surface/") or (k.startswith("lightmap/") and k.endswith("/ao"))]
        assert len(keep) >= 15 and differing({k: got[k] for k in keep}, {k: warm[k] for k in keep}) == [], said
    if c.name == "lights":
        for k in ("lightmap/undilated/irradiance", "lightmap/default/inf/irradiance", "probes/sh9/default", "probes/irradiance/default",
                  "rays/default", "filter", "lightmap_direct/default"):
            assert not same(warm[k], got[k]), (said, k)
    return said


def routes_line(where, routes):
    return "%s: rpt_paths launches (per-tree launches) " % where + ", ".join("%s %d (%d)" % ((k,) + routes[k]) for k in FLAGGED)


@pytest.mark.parametrize("name", C.NAMES)
def test_an_updated_handle_gives_a_fresh_handles_bits(name, monkeypatch):
    c = C.cases()[name]
    g = GpuScene(c.scene0, 0, **c.options)
    said = []
    try:
        warm, warm_routes = calls(g, c, monkeypatch)
        on_the_handle_itself(g, c, c.scene0, warm, "%s, before any update" % name)
        said.append(routes_line("%s, before any update" % name, warm_routes))
        assert all(warm_routes[k][0] > 0 for k in FLAGGED), said[-1]  # no tree_kids at creation: every request is honoured
        for step in c.steps:
            step.apply(g)
            got, routes = calls(g, c, monkeypatch)
            what = "%s, step %r" % (name, step.name)
            named = on_the_handle_itself(g, c, step.scene, got, what)
            if step.back:
                assert differing(got, warm) == [], what + ": not the creation's results again"
                continue
            f = GpuScene(step.scene, 0, **c.options)
            try:
                want, fresh_routes = calls(f, c, monkeypatch)
            finally:
                f.close()
            assert differing(got, want) == [], what + ": differs from a fresh handle"
            said.append(seen(c, step, warm, got) + "; %d rays name a triangle" % named)
            said.append(routes_line(what, routes))
            assert all(routes[k][0] == fresh_routes[k][0] for k in FLAGGED), (said[-1], routes_line("a fresh handle", fresh_routes))
            if c.flags_rise:  # tree_kids: the requests are dropped, on g as on f, and the per-tree pipeline runs
                assert all(routes[k] == (0, routes[k][1]) and routes[k][1] > 0 and fresh_routes[k][1] > 0 for k in FLAGGED), said[-1]
            else:
                assert all(routes[k][0] > 0 for k in FLAGGED), said[-1]
    finally:
        g.close()
        print("\n".join(said))  # (shown with -rP, and when the test fails)
