"""rptgpu_bake_direct and rptgpu_bake_lightmap_direct on the GPU, held to include/rpt_gpu_direct.h to the bit.

The call is DEFINED by things the repository already pins: Light::illuminate — the oracle's, called light after light on the
point's stream —, rptgpu_closest_hit for the ray towards each light sample, and a fold in the header's order, which
tests/direct_model.py restates in numpy (itself held to closed forms and to the oracle in tests/test_direct_host.py).  The
points are first hits of each scene's camera rays, lifted off their surface (tests/direct_cases.py, where the oracle alone
shows that they are lit, shadowed and facing away often enough).  Scenes: flat with a mesh light (cornell), an in-kernel
group under ambient + directional + point lights (fractal_spheres), the per-tree route under a sphere light (wine_glass), a
quad light + a point light (polygon_room), two sphere lights of which the first often faces away (two_lamps: the stream goes
on behind a light that adds nothing), the extended-shape build under a MonomialSurface light (monomial), trees of trees under
a lamp that is a group of groups (nested_groups); every one again under RPT_FLAG_GENERAL_TRAVERSAL.  The normals are no unit
vectors.  Tolerance 0 (the raw bits) everywhere
but in the tie to the renderer, whose bound is the rounding of two orders of multiplication."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from oracle import oracle_ffi as O
from rpt_amd import GpuScene, Light, Material, Object, _abi, plane, sphere

import direct_cases as DC
import direct_model as DM
import lightmap_model as LM

pytestmark = pytest.mark.gpu

N, SEED = DC.N_POINTS, DC.SEED
GENERAL = _abi.RPT_FLAG_GENERAL_TRAVERSAL
same = LM.same


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(DC.scene(name)[0], 0)


def casting(name):
    return sum(l.kind != _abi.RPT_LIGHT_AMBIENT for l in DC.scene(name)[0].lights)


@functools.lru_cache(maxsize=None)
def case(name, samples, base=0):
    """(out, the triples' details) as the header defines them for the scene's points: the oracle's illuminate, the device's
    closest_hit, the model's fold — computed once, shared, read-only"""
    pos, nrm, ids = DC.points(name)
    g = gpu(name)
    out, det = DM.direct(DC.scene(name)[0].lights, pos, nrm, samples, SEED, lambda o, d: g.closest_hit(o, d)[0],
                         sample_index_base=base, streams=ids, illuminate=DC.oracle_illuminate, details=True)
    out.setflags(write=False)
    return out, det


def bake(g, name, samples, **kw):
    pos, nrm, ids = DC.points(name)
    kw.setdefault("streams", ids)
    return g.bake_direct(kw.pop("pos", pos), kw.pop("nrm", nrm), samples=samples, seed=SEED, **kw)


# ---- 1. the definition, bit for bit, on every route
@pytest.mark.parametrize("flags", [0, GENERAL], ids=["routed", "general"])
@pytest.mark.parametrize("samples", [16, 33])
@pytest.mark.parametrize("name", DC.SCENES)
def test_bake_direct_is_the_fold_of_illuminate_and_closest_hit(name, samples, flags):
    want, det = case(name, samples)
    assert (want != 0.0).any() and 0.10 <= det["adds"].mean() <= 0.90  # (with the device's t, as with the oracle's)
    g = gpu(name)
    g.reset_stats()
    got = bake(g, name, samples, flags=flags)
    assert got.dtype == np.float64 and got.shape == (N, 3)
    assert same(got, want), (np.flatnonzero((got != want).any(axis=1)), np.abs(got - want).max())
    st = g.stats()
    queued = int(((det["cosv"] > 0.0) & ~(det["c"] == 0.0).all(axis=1)).sum())  # the triples whose light can add something
    assert st.shadow_rays == N * samples * casting(name) and st.shadow_rays_traced == queued and st.samples == 0
    assert 0 < queued < st.shadow_rays  # (some light faces away from some point: its ray is never traced)
    assert st.kernel_launches[_abi.RPT_K_SHADOW] >= 1 and st.kernel_launches[_abi.RPT_K_PATHS] == 0


# ---- 2. a result depends on its point and on nothing else
@pytest.mark.parametrize("name", DC.SCENES)
def test_bake_direct_does_not_depend_on_pieces_order_or_company(name, monkeypatch):
    samples = 33
    want, _ = case(name, samples)
    pos, nrm, ids = DC.points(name)
    g = gpu(name)
    assert same(bake(g, name, samples, pos=pos[::-1], nrm=nrm[::-1], streams=ids[::-1])[::-1], want)
    monkeypatch.setenv("RPTGPU_DIRECT_PIECE", "5")
    assert same(bake(g, name, samples), want)
    assert same(bake(g, name, samples, flags=GENERAL), want)
    monkeypatch.delenv("RPTGPU_DIRECT_PIECE")
    for i in range(N):
        assert same(bake(g, name, samples, pos=pos[i:i + 1], nrm=nrm[i:i + 1], streams=ids[i:i + 1]), want[i:i + 1])
    # the later samples of every point in a call of their own: the header's stream, from sample_index_base on
    assert same(bake(g, name, 17, sample_index_base=16), case(name, 17, 16)[0])


def test_stream_ids_default_to_the_indices(monkeypatch):
    pos, nrm, _ = DC.points("cornell")
    g = gpu("cornell")
    a = g.bake_direct(pos, nrm, samples=16, seed=SEED)
    assert same(a, g.bake_direct(pos, nrm, samples=16, seed=SEED, streams=np.arange(N, dtype=np.uint32)))
    assert not same(a, case("cornell", 16)[0])  # (the ids matter: the mesh light is sampled from the stream)
    monkeypatch.setenv("RPTGPU_DIRECT_PIECE", "5")  # ... the indices of the CALL, not of the piece
    assert same(a, g.bake_direct(pos, nrm, samples=16, seed=SEED))


@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_several_passes_per_piece(name, monkeypatch):
    """a handle whose passes hold 1024 slots (the least a handle takes), and 128 points — the scene's 16, eight times over under
    ids of their own — in one piece: their 33 samples run as five passes of at most eight samples each"""
    pos, nrm, ids = DC.points(name)
    pos, nrm, ids = np.tile(pos, (8, 1)), np.tile(nrm, (8, 1)), np.concatenate([ids + 1000 * r for r in range(8)])
    want = gpu(name).bake_direct(pos, nrm, samples=33, seed=SEED, streams=ids)
    assert same(want[:N], case(name, 33)[0])
    monkeypatch.setenv("RPTGPU_DIRECT_PIECE", "128")
    g = GpuScene(DC.scene(name)[0], 0, target_paths=1024)
    g.reset_stats()
    got = g.bake_direct(pos, nrm, samples=33, seed=SEED, streams=ids)
    launches = g.stats().kernel_launches[_abi.RPT_K_SHADOW]
    g.close()
    assert same(got, want)
    assert launches >= 5


@pytest.mark.parametrize("name", ["cornell", "fractal_spheres", "wine_glass", "two_lamps", "nested_groups"])
def test_device_arrays_give_the_host_calls_bits(name):
    want, _ = case(name, 33)
    pos, nrm, ids = DC.points(name)
    g = gpu(name)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a writable, contiguous copy of the shared arrays)
    d_pos, d_nrm, d_ids = to(pos), to(nrm), to(ids.astype(np.int64))
    got = g.bake_direct(d_pos, d_nrm, samples=33, seed=SEED, streams=d_ids)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device == dev and tuple(got.shape) == (N, 3)
    assert same(got.cpu().numpy(), want)
    assert same(d_pos.cpu().numpy(), pos) and same(d_nrm.cpu().numpy(), nrm)  # the inputs are as they were
    # an output inside a larger allocation: what lies behind it stays
    store = torch.full((N + 5, 3), 7.0, dtype=torch.float64, device=dev)
    out = store[:N]
    assert g.bake_direct(d_pos, d_nrm, samples=33, seed=SEED, streams=d_ids, out=out) is out
    assert same(out.cpu().numpy(), want) and (store[N:] == 7.0).all().item()
    no_ids_host = g.bake_direct(pos, nrm, samples=16, seed=SEED)
    assert same(g.bake_direct(d_pos, d_nrm, samples=16, seed=SEED).cpu().numpy(), no_ids_host)


def test_after_live_updates_the_results_are_a_fresh_handles():
    name = "polygon_room"
    scene = DC.scene(name)[0]
    pos, nrm, ids = DC.points(name)
    g = GpuScene(scene, 0)
    before = bake(g, name, 16)
    assert same(before, case(name, 16)[0])
    # the point light moves and brightens, the first cube moves
    lights = list(scene.lights)
    k = [i for i, l in enumerate(lights) if l.kind == _abi.RPT_LIGHT_POINT][0]
    moved = Light.Point((35.0, 30.0, 10.0), (1.0, 1.5, 3.0))
    g.set_lights([k], [moved])
    j = [i for i, o in enumerate(scene.objects) if isinstance(o.shape, rpt_amd.shape.Transformed)][0]
    cube = Object(scene.objects[j].shape.translate((0.3, 0.8, 1.5))).material(Material.diffuse((0.8, 0.8, 0.8)))
    g.set_objects([j], [cube])
    after = bake(g, name, 16)
    g.close()
    updated = rpt_amd.Scene()
    updated.objects, updated.lights, updated.environment = list(scene.objects[:j]) + [cube] + list(scene.objects[j + 1:]), lights[:k] + [moved] + lights[k + 1:], scene.environment
    fresh = GpuScene(updated, 0)
    want = fresh.bake_direct(pos, nrm, samples=16, seed=SEED, streams=ids)
    fresh.close()
    assert same(after, want) and not same(after, before)


@pytest.mark.parametrize("ambient", [False, True], ids=["no lights", "ambient only"])
def test_a_scene_without_a_light_that_casts(ambient):
    scene = DC.scene("cornell")[0]
    bare = rpt_amd.Scene()
    bare.objects, bare.environment = list(scene.objects), scene.environment
    if ambient:
        bare.add(Light.Ambient((0.3, 0.3, 0.3)))
        bare.add(Light.Ambient((0.1, 0.2, 0.3)))
    pos, nrm, ids = DC.points("cornell")
    g = GpuScene(bare, 0)
    g.reset_stats()
    got = g.bake_direct(pos, nrm, samples=16, seed=SEED, streams=ids)
    dev = torch.device("cuda", 0)
    got_dev = g.bake_direct(torch.from_numpy(np.array(pos)).to(dev), torch.from_numpy(np.array(nrm)).to(dev), samples=16, seed=SEED,
                            out=torch.full((N, 3), 7.0, dtype=torch.float64, device=dev)).cpu().numpy()
    st = g.stats()
    g.close()
    for a in (got, got_dev):
        assert a.shape == (N, 3) and (a == 0.0).all() and not np.signbit(a).any()
    assert st.shadow_rays == 0 and st.shadow_rays_traced == 0 and st.kernel_launches[_abi.RPT_K_SHADOW] == 0


def test_nothing_to_do_and_refusals_on_a_live_handle():
    g = gpu("cornell")
    assert g.bake_direct(np.zeros((0, 3)), np.zeros((0, 3)), samples=4, seed=1).shape == (0, 3)
    pos, nrm, ids = DC.points("cornell")
    with pytest.raises(rpt_amd.RptGpuError) as e:
        g.bake_direct(pos, nrm, samples=4, seed=1, flags=_abi.RPT_FLAG_PERSISTENT)
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and "RPT_FLAG_PERSISTENT" in str(e.value)
    with pytest.raises(rpt_amd.RptGpuError) as e:
        g.bake_direct(pos, nrm, samples=0, seed=1)
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and "samples == 0" in str(e.value)
    assert same(bake(g, "cornell", 16), case("cornell", 16)[0])  # the handle is as good as before
    # a NaN and a zero normal are not refused: +0.0
    bad = np.array(nrm)
    bad[0], bad[1] = (float("nan"), 0.0, 1.0), (0.0, 0.0, 0.0)
    got = bake(g, "cornell", 16, nrm=bad)
    assert (got[:2] == 0.0).all() and not np.signbit(got[:2]).any() and same(got[2:], case("cornell", 16)[0][2:])


# ---- 3. the tie to the renderer: a hit's next-event term is bsdf * bake_direct
def test_a_renders_direct_term_is_bsdf_times_bake_direct():
    """One point light, a diffuse plane and a sphere that shadows part of it.  trace_rays with max_bounces = 0 and one sample
    returns emission (none) + bsdf * I * (wi . n) where the light is seen: the hit's stream starts at first_draw = 0, where
    the direct call's starts.  Fewer than ten roundings of 2^-53 separate `(bsdf * I) * cos` from `bsdf * (I * cos)`, the
    hit point and the normal are the same bits: 1e-12 relative leaves a margin of about 10^3."""
    grey = Material.diffuse((0.8, 0.5, 0.3))
    light = Light.Point((40.0, 50.0, 60.0), (1.0, 4.0, 2.0))
    scene = rpt_amd.Scene()
    scene.add(Object(plane((0.0, 1.0, 0.0), -1.0)).material(grey))
    scene.add(Object(sphere().scale((1.8, 1.8, 1.8)).translate((0.5, 1.0, 1.0))).material(Material.diffuse((0.2, 0.2, 0.2))))
    scene.add(light)
    g = GpuScene(scene, 0)
    rs = np.random.RandomState(8)
    o = rs.uniform((-4.0, 2.0, -4.0), (4.0, 5.0, 4.0), (96, 3))
    d = rs.uniform((-0.4, -1.0, -0.4), (0.4, -0.6, 0.4), (96, 3))
    t, nrm, obj = g.closest_hit(o, d)
    on_plane = obj == 0
    assert on_plane.sum() >= 48
    o, d, t, nrm = o[on_plane], d[on_plane], t[on_plane], nrm[on_plane]
    ids = np.arange(len(o), dtype=np.uint32) + 11
    rgb = g.trace_rays(o, d, 0, streams=ids, samples=1, seed=SEED, first_draw=0)
    pos = o + t[:, None] * d  # renderer.rs:149, in its order
    direct = g.bake_direct(pos, nrm, samples=1, seed=SEED, streams=ids)
    g.close()
    lit = (direct != 0.0).any(axis=1)
    assert 0.2 <= lit.mean() <= 0.8, lit.mean()  # the sphere's shadow is there, and so is the light (by the oracle: 0.40)
    want = np.zeros_like(rgb)
    for i in range(len(o)):
        wo = -d[i] / np.sqrt(DM.dot(d[i], d[i]))
        wi = DM.illuminate(light, pos[i], SEED, int(ids[i]), 0, 0)[1]
        want[i] = O.bsdf(grey, nrm[i], wo, wi) * direct[i]
    assert (rgb[~lit] == 0.0).all()
    assert (np.abs(rgb - want) <= 1e-12 * np.abs(want)).all(), np.abs(rgb / np.where(want == 0.0, 1.0, want) - 1.0).max()


# ---- 4. the lightmap form
FLOOR = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 559.2], [556.0, 0.0, 559.2]], [[0.0, 0.0, 0.0], [556.0, 0.0, 559.2], [556.0, 0.0, 0.0]]])
FLOOR_UV = np.array([[[1 / 16, 1 / 16], [1 / 16, 15 / 16], [15 / 16, 15 / 16]], [[1 / 16, 1 / 16], [15 / 16, 15 / 16], [15 / 16, 1 / 16]]])
FLOOR_UP = np.tile(np.array([0.0, 2.0, 0.0]), (2, 3, 1))  # (no unit vectors: the texel pass normalises)
LM_KW = dict(normals=FLOOR_UP, samples=8, seed=SEED, offset=0.5, stream_base=1000, sample_index_base=3)
RAW = _abi.RPT_LIGHTMAP_OWNER | _abi.RPT_LIGHTMAP_POSITION | _abi.RPT_LIGHTMAP_NORMAL


@functools.lru_cache(maxsize=None)
def undilated(w, h):
    out = gpu("cornell").bake_lightmap_direct(FLOOR, FLOOR_UV, w, h, **LM_KW)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("w,h", [(16, 16), (13, 7)])
def test_a_lightmap_is_bake_direct_scattered_at_the_lightmaps_own_texels(w, h, monkeypatch):
    g = gpu("cornell")
    raw = g.bake_lightmap(FLOOR, FLOOR_UV, w, h, normals=FLOOR_UP, seed=SEED, offset=0.5, channels=RAW)
    owned = raw["owner"] >= 0
    assert 0.4 <= owned.mean() < 1.0
    ys, xs = np.nonzero(owned)
    at = g.bake_direct(np.ascontiguousarray(raw["position"][owned]), np.ascontiguousarray(raw["normal"][owned]), samples=8, seed=SEED,
                       sample_index_base=3, streams=(1000 + ys * w + xs).astype(np.uint32))
    want = np.zeros((h, w, 3))
    want[owned] = at
    got = undilated(w, h)
    assert got.shape == (h, w, 3) and same(got, want)
    assert (got[owned] != 0.0).any() and not np.signbit(got[~owned]).any()
    # ... in pieces of 7 texels, through the generic walker, and from device arrays
    monkeypatch.setenv("RPTGPU_LIGHTMAP_PIECE", "7")
    assert same(g.bake_lightmap_direct(FLOOR, FLOOR_UV, w, h, **LM_KW), want)
    monkeypatch.delenv("RPTGPU_LIGHTMAP_PIECE")
    assert same(g.bake_lightmap_direct(FLOOR, FLOOR_UV, w, h, flags=GENERAL, **LM_KW), want)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)
    kw = dict(LM_KW, normals=to(FLOOR_UP))
    on_dev = g.bake_lightmap_direct(to(FLOOR), to(FLOOR_UV), w, h, **kw)
    assert on_dev.device == dev and same(on_dev.cpu().numpy(), want)


@pytest.mark.parametrize("rounds", [0, 1, 3, "max"])
@pytest.mark.parametrize("w,h", [(16, 16), (13, 7)])
def test_a_lightmaps_dilation_is_the_models_over_its_own_undilated_output(w, h, rounds):
    rounds = max(w, h) if rounds == "max" else rounds
    g = gpu("cornell")
    owner = g.bake_lightmap(FLOOR, FLOOR_UV, w, h, normals=FLOOR_UP, seed=SEED, offset=0.5, channels=_abi.RPT_LIGHTMAP_OWNER)["owner"]
    want, filled = LM.dilate(undilated(w, h), owner >= 0, rounds)
    got = g.bake_lightmap_direct(FLOOR, FLOOR_UV, w, h, dilate=rounds, **LM_KW)
    assert same(got, want)
    if rounds == max(w, h):
        assert filled.all() and same(g.bake_lightmap_direct(FLOOR, FLOOR_UV, w, h, dilate=10 ** 6, **LM_KW), want)


def test_a_lightmap_without_triangles():
    got = gpu("cornell").bake_lightmap_direct(np.zeros((0, 3, 3)), np.zeros((0, 3, 2)), 13, 7, samples=4, seed=1, dilate=2)
    assert got.shape == (7, 13, 3) and (got == 0.0).all() and not np.signbit(got).any()
