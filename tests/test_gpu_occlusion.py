"""rptgpu_occluded and rptgpu_bake_ao on the GPU: visibility for rays the caller brings, and ambient occlusion whose
directions the library draws itself.

Both calls are DEFINED by things the repository already pins (include/rpt_gpu.h): `out = ~(t > fmin(max_t, DBL_MAX))` with
t from GpuScene.closest_hit, and for ambient occlusion the directions of RPT_PROBE_IRRADIANCE — restated here from the
oracle's stream and Sphere::sample, as test_gpu_probes.directions restates them — pushed through the same closest_hit and
folded in numpy in the header's order.  Tolerance 0 (== on bytes and f64 arrays) everywhere but in one closed form, whose
bound is the rounding of S additions.  The scenes: flat (cornell), every analytic shape (coverage), a deep mesh through the
per-tree queries (wine_glass), the extended build with NaN hits (monomial), trees of trees through the generic walker
(nested_groups)."""
import functools
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, _abi

import small_scenes
import test_gpu_probes as probes_test

pytestmark = pytest.mark.gpu

DBL_MAX = 1.7976931348623157e308
INF = float("inf")
SCENES = ["cornell", "coverage", "wine_glass", "monomial", "nested_groups"]
# where rays start and points stand: test_gpu_probes' boxes, and boxes of the same kind for the two scenes it does not use
BOXES = {name: probes_test.BOXES[name] for name in ("cornell", "coverage", "wine_glass")}
BOXES["monomial"] = ((-3.0, -0.9, -2.5), (3.0, 3.5, 2.5))
BOXES["nested_groups"] = ((-2.5, -0.9, -3.0), (2.5, 3.0, 2.5))
N_RAYS = 600    # three 256-thread blocks, the last one partial
N_POINTS = 16   # x S = 16, 33: 256 and 528 slots
SEED = 0x0CC1
GENERAL = _abi.RPT_FLAG_GENERAL_TRAVERSAL


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(small_scenes.small(name)[0], 0)


@functools.lru_cache(maxsize=None)
def rays(name):
    """(origins, directions that are NOT unit vectors, max_t, closest_hit's t, the expected bytes) — computed once, shared,
    read-only.  max_t cycles through +inf, NaN, 0, -1, t, the doubles next to t, t / 2 and 2 t (a random finite value where
    the ray misses and there is no t to derive one from)."""
    rs = np.random.RandomState(sum(map(ord, name)) + 1)
    lo, hi = BOXES[name]
    o = rs.uniform(lo, hi, (N_RAYS, 3))
    d = rs.standard_normal((N_RAYS, 3)) * rs.uniform(0.25, 4.0, (N_RAYS, 1))
    if name == "monomial":
        # test_gpu_shadow_nan's construction for this scene's monomial_surface(2, 4).translate((0, -1, 0)): an exactly
        # vertical ray over a corner of its box (5 < 2 (x^2 + z^2)^2 there), whose Newton step divides by -0
        for k, (sx, sz) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
            o[9 * k + 2] = (0.95 * sx, 4.0, 0.95 * sz)  # (rows whose max_t is 0.0 ...
            d[9 * k + 2] = (0.0, -1.0, 0.0)
            o[9 * k + 4 + 9 * 8] = (0.93 * sx, 4.0, 0.96 * sz)  # ... and rows whose max_t is t itself: NaN, which stops nowhere
            d[9 * k + 4 + 9 * 8] = (0.0, -1.0, 0.0)
    t = gpu(name).closest_hit(o, d)[0]
    finite = rs.uniform(0.0, 2.0 * np.linalg.norm(np.subtract(hi, lo)) / 4.0, N_RAYS)
    base = np.where(np.isinf(t), finite, t)
    forms = [np.full(N_RAYS, INF), np.full(N_RAYS, np.nan), np.zeros(N_RAYS), np.full(N_RAYS, -1.0), base,
             np.nextafter(base, -INF), np.nextafter(base, INF), 0.5 * base, 2.0 * base]
    max_t = np.choose(np.arange(N_RAYS) % len(forms), forms)
    want = (~(t > np.fmin(max_t, DBL_MAX))).astype(np.uint8)
    for a in (o, d, max_t, t, want):
        a.setflags(write=False)
    return o, d, max_t, t, want


@functools.lru_cache(maxsize=None)
def points(name):
    """test_gpu_probes' probes of the scene: positions, unit normals, stream ids that are not the indices"""
    if name in probes_test.BOXES:
        return probes_test.probes(name)
    rs = np.random.RandomState(sum(map(ord, name)))
    lo, hi = BOXES[name]
    pos = rs.uniform(lo, hi, (N_POINTS, 3))
    nrm = rs.standard_normal((N_POINTS, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ids = rs.permutation(1000)[:N_POINTS].astype(np.uint32) + 5
    for a in (pos, nrm, ids):
        a.setflags(write=False)
    return pos, nrm, ids


def half_diagonal(name):
    lo, hi = BOXES[name]
    return 0.5 * float(np.linalg.norm(np.subtract(hi, lo)))


def fold(d, t, max_distance):
    """the header's result from the directions [n][S][3] and closest_hit's t [n][S]: k ascending, from +0.0"""
    n, S = t.shape
    v = t > np.fmin(max_distance, DBL_MAX)
    acc = np.zeros((n, 3))
    for k in range(S):
        acc = np.where(v[:, k, None], acc + d[:, k], acc)
    return v.sum(axis=1).astype(np.float64) / float(S), acc / float(S)


@functools.lru_cache(maxsize=None)
def ao_case(name, samples, far):
    """(ao, bent) as include/rpt_gpu.h defines them for the scene's points — computed once, shared, read-only"""
    pos, nrm, ids = points(name)
    d, _ = probes_test.directions(probes_test.IRR, nrm, ids, SEED, samples, 0)
    t = gpu(name).closest_hit(np.repeat(pos, samples, axis=0), d.reshape(-1, 3))[0].reshape(N_POINTS, samples)
    ao, bent = fold(d, t, INF if far else half_diagonal(name))
    ao.setflags(write=False)
    bent.setflags(write=False)
    return ao, bent


def bake(g, name, samples, far, **kw):
    pos, nrm, ids = points(name)
    kw.setdefault("streams", ids)
    return g.bake_ao(kw.pop("pos", pos), kw.pop("nrm", nrm), samples=samples, seed=SEED,
                     max_distance=INF if far else half_diagonal(name), bent_normals=True, **kw)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the definition, bit for bit
@pytest.mark.parametrize("name", SCENES)
def test_occluded_is_closest_hit_held_against_max_t(name):
    o, d, max_t, t, want = rays(name)
    assert want.mean() >= 0.10 and (1 - want).mean() >= 0.10, want.mean()  # both answers, often
    if name == "monomial":
        assert np.isnan(t).any() and want[np.isnan(t)].all()  # a NaN hit is there, and it occludes
    g = gpu(name)
    g.reset_stats()
    got = g.occluded(o, d, max_t)
    assert got.dtype == np.uint8 and got.shape == (N_RAYS,)
    assert (got == want).all(), "%d of %d rays differ: %s" % ((got != want).sum(), N_RAYS, np.flatnonzero(got != want)[:8])
    st = g.stats()
    assert st.shadow_rays == N_RAYS and st.shadow_rays_traced == N_RAYS and st.samples == 0
    assert st.kernel_launches[_abi.RPT_K_SHADOW] >= 1 and st.kernel_launches[_abi.RPT_K_PATHS] == 0


@pytest.mark.parametrize("far", [True, False], ids=["inf", "half-diagonal"])
@pytest.mark.parametrize("samples", [16, 33])
@pytest.mark.parametrize("name", SCENES)
def test_bake_ao_is_the_fold_of_closest_hits(name, samples, far):
    want_ao, want_bent = ao_case(name, samples, far)
    assert not (want_ao == 0.0).all() and not (want_ao == 1.0).all()
    g = gpu(name)
    g.reset_stats()
    ao, bent = bake(g, name, samples, far)
    assert ao.dtype == np.float64 and ao.shape == (N_POINTS,) and bent.dtype == np.float64 and bent.shape == (N_POINTS, 3)
    assert (ao == want_ao).all(), (ao, want_ao)
    assert (bent == want_bent).all(), np.abs(bent - want_bent).max()
    st = g.stats()
    assert st.shadow_rays == N_POINTS * samples and st.shadow_rays_traced == N_POINTS * samples and st.samples == 0
    assert st.kernel_launches[_abi.RPT_K_SHADOW] >= 1 and st.kernel_launches[_abi.RPT_K_PATHS] == 0
    # without the bent normals: the same fractions
    pos, nrm, ids = points(name)
    only = g.bake_ao(pos, nrm, samples=samples, seed=SEED, max_distance=INF if far else half_diagonal(name), streams=ids)
    assert same(only, ao)


# ---- 2. a result depends on its ray or point and on nothing else
@pytest.mark.parametrize("name", SCENES)
def test_occluded_does_not_depend_on_pieces_order_or_company(name, monkeypatch):
    o, d, max_t, t, want = rays(name)
    g = gpu(name)
    assert same(g.occluded(o[::-1], d[::-1], max_t[::-1].copy())[::-1], want)
    assert same(g.occluded(o, d, max_t, flags=GENERAL), want)
    monkeypatch.setenv("RPTGPU_OCCLUSION_PIECE", "100")
    assert same(g.occluded(o, d, max_t), want)
    monkeypatch.delenv("RPTGPU_OCCLUSION_PIECE")
    alone = np.concatenate([g.occluded(o[i:i + 1], d[i:i + 1], max_t[i:i + 1]) for i in range(N_RAYS)])
    assert same(alone, want)


@pytest.mark.parametrize("name", SCENES)
def test_bake_ao_does_not_depend_on_pieces_order_or_company(name, monkeypatch):
    samples, far = 33, False
    want_ao, want_bent = ao_case(name, samples, far)
    pos, nrm, ids = points(name)
    g = gpu(name)
    ao, bent = bake(g, name, samples, far, pos=pos[::-1], nrm=nrm[::-1], streams=ids[::-1])
    assert same(ao[::-1], want_ao) and same(bent[::-1], want_bent)
    ao, bent = bake(g, name, samples, far, flags=GENERAL)
    assert same(ao, want_ao) and same(bent, want_bent)
    monkeypatch.setenv("RPTGPU_OCCLUSION_PIECE", "5")
    ao, bent = bake(g, name, samples, far)
    assert same(ao, want_ao) and same(bent, want_bent)
    monkeypatch.delenv("RPTGPU_OCCLUSION_PIECE")
    for i in range(N_POINTS):
        ao, bent = bake(g, name, samples, far, pos=pos[i:i + 1], nrm=nrm[i:i + 1], streams=ids[i:i + 1])
        assert same(ao, want_ao[i:i + 1]) and same(bent, want_bent[i:i + 1])
    # the samples of a point in two calls of their own: the counts add up (sample_index_base)
    a0 = g.bake_ao(pos, nrm, samples=16, seed=SEED, max_distance=half_diagonal(name), streams=ids)
    a1 = g.bake_ao(pos, nrm, samples=17, seed=SEED, max_distance=half_diagonal(name), streams=ids, sample_index_base=16)
    assert (np.rint(a0 * 16.0) + np.rint(a1 * 17.0) == np.rint(want_ao * 33.0)).all()


def test_stream_ids_default_to_the_indices(monkeypatch):
    pos, nrm, _ = points("cornell")
    g = gpu("cornell")
    a = g.bake_ao(pos, nrm, samples=16, seed=SEED, bent_normals=True)
    b = g.bake_ao(pos, nrm, samples=16, seed=SEED, bent_normals=True, streams=np.arange(N_POINTS, dtype=np.uint32))
    assert same(a[0], b[0]) and same(a[1], b[1])
    # ... of the CALL, not of the piece
    monkeypatch.setenv("RPTGPU_OCCLUSION_PIECE", "5")
    c = g.bake_ao(pos, nrm, samples=16, seed=SEED, bent_normals=True)
    assert same(a[0], c[0]) and same(a[1], c[1])


@pytest.mark.parametrize("name", ["cornell", "wine_glass", "nested_groups"])
def test_device_arrays_give_the_host_calls_bits(name):
    o, d, max_t, t, want = rays(name)
    g = gpu(name)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a writable, contiguous copy of the shared arrays)
    got = g.occluded(to(o), to(d), to(max_t))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and got.device == dev
    assert same(got.cpu().numpy(), want)
    assert same(g.occluded(to(o), to(d)).cpu().numpy(), g.occluded(o, d))  # without max_t
    out = torch.full((N_RAYS,), 7, dtype=torch.uint8, device=dev)
    assert g.occluded(to(o), to(d), to(max_t), out=out) is out and same(out.cpu().numpy(), want)
    want_ao, want_bent = ao_case(name, 33, False)
    pos, nrm, ids = points(name)
    ao, bent = bake(g, name, 33, False, pos=to(pos), nrm=to(nrm), streams=to(ids.astype(np.int64)))
    assert ao.device == dev and same(ao.cpu().numpy(), want_ao) and same(bent.cpu().numpy(), want_bent)
    no_ids_host = g.bake_ao(pos, nrm, samples=16, seed=SEED)
    assert same(g.bake_ao(to(pos), to(nrm), samples=16, seed=SEED).cpu().numpy(), no_ids_host)


@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_no_max_t_is_infinity(name):
    o, d, _, t, _ = rays(name)
    g = gpu(name)
    got = g.occluded(o, d)
    assert same(got, g.occluded(o, d, np.full(N_RAYS, INF)))
    assert same(got, (~(t > DBL_MAX)).astype(np.uint8))  # = "it hits something"


def test_a_scene_without_lights():
    """no light, hence no shadow column in a render of it: the calls bring their own"""
    scene = small_scenes.small("cornell")[0]
    bare = rpt_amd.Scene()
    bare.objects, bare.environment = list(scene.objects), scene.environment
    assert len(scene.lights) > 0 and len(bare.lights) == 0
    o, d, max_t, t, want = rays("cornell")
    g = GpuScene(bare, 0)
    assert same(g.closest_hit(o, d)[0], t)  # (cornell's lights are no objects of its closest-hit query)
    assert same(g.occluded(o, d, max_t), want)
    want_ao, want_bent = ao_case("cornell", 33, False)
    ao, bent = bake(g, "cornell", 33, False)
    g.close()
    assert same(ao, want_ao) and same(bent, want_bent)


def test_nothing_to_do_and_refusals_on_a_live_handle():
    g = gpu("cornell")
    assert g.occluded(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    assert g.bake_ao(np.zeros((0, 3)), np.zeros((0, 3)), samples=4, seed=1).shape == (0,)
    o, d, max_t, _, want = rays("cornell")
    with pytest.raises(rpt_amd.RptGpuError) as e:
        g.occluded(o, d, max_t, flags=_abi.RPT_FLAG_PERSISTENT)
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and "RPT_FLAG_PERSISTENT" in str(e.value)
    pos, nrm, _ = points("cornell")
    with pytest.raises(rpt_amd.RptGpuError) as e:
        g.bake_ao(pos, nrm, samples=0, seed=1)
    assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and "samples == 0" in str(e.value)
    assert same(g.occluded(o, d, max_t), want)  # the handle is as good as before


# ---- 3. closed forms
@pytest.mark.parametrize("samples", [1, 64])
def test_the_centre_of_a_large_sphere(samples):
    """every direction meets the sphere at t = R (|d| = 1 up to rounding): open below R, closed beyond"""
    R = 10.0
    scene = rpt_amd.Scene()
    scene.add(rpt_amd.Object(rpt_amd.sphere().scale((R, R, R))).material(rpt_amd.Material.diffuse((0.5, 0.5, 0.5))))
    g = GpuScene(scene, 0)
    rs = np.random.RandomState(5)
    nrm = rs.standard_normal((N_POINTS, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pos = np.zeros((N_POINTS, 3))
    ids = np.arange(N_POINTS, dtype=np.uint32) * 7 + 1
    ao, bent = g.bake_ao(pos, nrm, samples=samples, seed=SEED, max_distance=0.5 * R, streams=ids, bent_normals=True)
    closed, closed_bent = g.bake_ao(pos, nrm, samples=samples, seed=SEED, streams=ids, bent_normals=True)
    g.close()
    assert (ao == 1.0).all() and (closed == 0.0).all() and (closed_bent == 0.0).all()
    # all S directions are visible: bent = (d_0 + .. + d_{S-1}) / S.  Every partial sum is at most S long, so each of the S
    # additions rounds by at most S * 2^-53, the sum by S^2 * 2^-53, the quotient by S * 2^-53 and its own rounding
    d, _ = probes_test.directions(probes_test.IRR, nrm, ids, SEED, samples, 0)
    mean = np.array([[math.fsum(d[i, :, c]) / samples for c in range(3)] for i in range(N_POINTS)])
    assert np.abs(bent - mean).max() <= (samples + 2) * 2.0 ** -53
    assert (np.einsum("ij,ij->i", bent, nrm) > 0.0).all()  # cosine-weighted about the normal


def test_above_a_lone_plane():
    """directions about the plane's own normal never come back to it"""
    scene = rpt_amd.Scene()
    scene.add(rpt_amd.Object(rpt_amd.plane((0.0, 1.0, 0.0), 0.0)).material(rpt_amd.Material.diffuse((0.5, 0.5, 0.5))))
    g = GpuScene(scene, 0)
    rs = np.random.RandomState(6)
    pos = rs.uniform((-5.0, 0.01, -5.0), (5.0, 3.0, 5.0), (N_POINTS, 3))
    up = np.tile(np.array([0.0, 1.0, 0.0]), (N_POINTS, 1))
    ao = g.bake_ao(pos, up, samples=64, seed=SEED)
    down = g.bake_ao(pos, -up, samples=64, seed=SEED)
    g.close()
    assert (ao == 1.0).all()
    assert (down == 0.0).all()  # ... and about the opposite normal every one of them meets it
