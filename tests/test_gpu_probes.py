"""rptgpu_bake_probes on the GPU: light probes whose directions the library draws itself.

A probe is `samples` paths, each along a direction made from the head of its own Philox stream.  The test makes the same
directions on the host from the oracle's restatement of the stream (oracle_rng_sample: UnitDisc; oracle_shape_sample:
Sphere::sample), hands them to GpuScene.trace_rays — which test_gpu_trace_rays.py ties to the oracle's frame and to the
independent path tracer — with the draw each direction stopped at, and folds the radiance in numpy in the order
include/rpt_gpu.h states.  bake_probes must return those bits: tolerance 0 (== on the f64 arrays) everywhere but in the
closed forms, whose bound is the rounding of at most 4096 additions."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, _abi, make_params, sphere

import small_scenes

pytestmark = pytest.mark.gpu

SH9, IRR = _abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE
KINDS = {"sh9": SH9, "irradiance": IRR}
FOUR_PI, PI = 12.566370614359172, 3.141592653589793
# where the probes stand: inside the box of each fixture scene (between, and now and then inside, its objects)
BOXES = {"cornell": ((20.0, 20.0, 20.0), (536.0, 528.0, 540.0)), "coverage": ((-2.5, -0.9, -2.5), (2.5, 3.0, 2.5)),
         "glass": ((-2.5, -1.5, -2.5), (2.5, 1.5, 2.5)), "wine_glass": ((-2.0, 0.1, -2.0), (2.0, 4.0, 2.0))}
N_PROBES = 16  # (a block of 256 paths per sample is exceeded by n * S: 16 * 33 = 528 paths, three blocks, the last one partial)


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(small_scenes.small(name)[0], 0)


@functools.lru_cache(maxsize=None)
def probes(name, n=N_PROBES):
    """(positions, unit normals, stream ids that are NOT the indices) of n probes in the scene's box — shared, read-only"""
    rs = np.random.RandomState(sum(map(ord, name)))
    lo, hi = BOXES[name]
    pos = rs.uniform(lo, hi, (n, 3))
    nrm = rs.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ids = rs.permutation(1000)[:n].astype(np.uint32) + 5
    for a in (pos, nrm, ids):
        a.setflags(write=False)
    return pos, nrm, ids


def directions(kind, nrm, ids, seed, samples, base):
    """the directions of include/rpt_gpu.h restated from the oracle's stream -> ([n][S][3] directions, [n][S] draws taken)"""
    from oracle import oracle_ffi as O
    n = len(ids)
    d = np.empty((n, samples, 3))
    draws = np.empty((n, samples), dtype=np.uint32)
    unit = sphere()
    for i in range(n):
        for k in range(samples):
            if kind == SH9:
                (x1, x2), draws[i, k] = O.rng_sample(4, seed=seed, pixel=int(ids[i]), sample=base + k, draw=0)
                x1, x2 = float(x1), float(x2)
                s = x1 * x1 + x2 * x2
                r = 2.0 * math.sqrt(1.0 - s)
                d[i, k] = (x1 * r, x2 * r, 1.0 - 2.0 * s)
            else:
                d[i, k], _, _, draws[i, k] = O.shape_sample(unit, nrm[i], seed=seed, pixel=int(ids[i]), sample=base + k, draw=0)
    return d, draws


def restated(g, kind, pos, nrm, ids, bounces, seed, samples, base=0):
    """the probes from the public ray call: one trace_rays per (sample index, draw count) group — first_draw and the
    sample index are the call's —, then the header's fold in numpy, k ascending"""
    n = len(pos)
    d, draws = directions(kind, nrm, ids, seed, samples, base)
    L = np.full((n, samples, 3), np.nan)
    for k in range(samples):
        for c in sorted(set(draws[:, k].tolist())):
            m = draws[:, k] == c
            L[m, k] = g.trace_rays(pos[m], d[m, k], bounces, samples=1, seed=seed, sample_index_base=base + k,
                                   streams=ids[m], first_draw=c, exposure_value=0.0)
    assert not np.isnan(L).any()
    if kind == SH9:
        acc = np.zeros((n, 9, 3))
        for k in range(samples):
            Y = rpt_amd.sh9_basis(d[:, k])                      # [n][9]
            acc = acc + L[:, k, None, :] * Y[:, :, None]         # acc[j][c] = acc[j][c] + L_k[c] * Y_j(d_k)
        return acc * (FOUR_PI / float(samples)), d, draws
    acc = np.zeros((n, 3))
    for k in range(samples):
        acc = acc + L[:, k]
    return acc * (PI / float(samples)), d, draws


@functools.lru_cache(maxsize=None)
def case(name, kind_name, samples):
    """(what bake_probes must return for the scene's probes, the draws their directions took) — computed once, shared"""
    kind = KINDS[kind_name]
    pos, nrm, ids = probes(name)
    p = small_scenes.small(name)[2]
    want, d, draws = restated(gpu(name), kind, pos, nrm, ids, p.max_bounces, p.seed, samples)
    want.setflags(write=False)
    return want, draws


def bake(g, name, kind, samples, pos=None, nrm=None, streams="ids", **kw):
    p0, n0, ids = probes(name)
    pos = p0 if pos is None else pos
    nrm = n0 if nrm is None else nrm
    p = small_scenes.small(name)[2]
    kw.setdefault("seed", p.seed)
    kw.setdefault("max_bounces", p.max_bounces)
    return g.bake_probes(pos, nrm if kind == IRR else None, kind=kind, samples=samples,
                         streams=ids if isinstance(streams, str) else streams, **kw)


# ---- 1. the public ray call's bits
@pytest.mark.parametrize("name,kind_name,samples", [
    ("cornell", "sh9", 33), ("cornell", "irradiance", 16), ("coverage", "sh9", 16), ("coverage", "irradiance", 33),
    ("glass", "sh9", 16), ("glass", "irradiance", 33), ("wine_glass", "sh9", 33), ("wine_glass", "irradiance", 16)])
def test_the_ray_calls_bits(name, kind_name, samples):
    """flat and deep-tree routing, object lights, HDRI misses, both kinds, an even and an odd sample count"""
    kind = KINDS[kind_name]
    want, draws = case(name, kind_name, samples)
    assert len(set(draws.ravel().tolist())) >= 2  # UnitDisc rejects now and then: the paths do not all start at one draw
    g = gpu(name)
    g.reset_stats()
    got = bake(g, name, kind, samples)
    assert got.dtype == np.float64 and got.shape == ((N_PROBES, 9, 3) if kind == SH9 else (N_PROBES, 3))
    assert np.isfinite(want).all() and (want != 0.0).any()
    assert (got == want).all(), "%d of %d probes differ" % ((got != want).reshape(N_PROBES, -1).any(axis=1).sum(), N_PROBES)
    st = g.stats()
    assert st.samples == N_PROBES * samples and st.extend_rays >= N_PROBES * samples
    assert st.kernel_launches[_abi.RPT_K_RAYGEN] >= 1 and st.kernel_launches[_abi.RPT_K_PATHS] == 0  # wavefront only


# ---- 2. closed forms
@pytest.mark.parametrize("samples", [1, 33, 4096])
def test_constant_environment(samples):
    """no objects, no lights, Environment::Color(c): every path is one miss and L_k = c exactly"""
    c = np.array([0.3, 1.0, 3.5])
    scene = rpt_amd.Scene()
    scene.environment = rpt_amd.Environment.Color(tuple(c))
    g = GpuScene(scene, 0)
    pos, nrm, ids = probes("coverage")
    seed = 77
    ir = g.bake_probes(pos, nrm, kind=IRR, samples=samples, max_bounces=3, seed=seed, streams=ids)
    sh = g.bake_probes(pos, kind=SH9, samples=samples, max_bounces=3, seed=seed, streams=ids)
    g.close()
    # S equal terms c: the running sum's relative error is at most (S - 1) * 2^-53 < 4.6e-13 for S <= 4096, then one
    # multiplication by a rounded pi / S (two more roundings)
    assert np.abs(ir / (PI * c) - 1.0).max() <= 1e-12
    # Y0 is a constant: the (0,0) coefficient is c * Y0 * 4 pi = c * sqrt(4 pi), whatever the directions are
    assert np.abs(sh[:, 0] / (c * 3.5449077018110318) - 1.0).max() <= 1e-12
    # the higher coefficients are the projection of the directions themselves: restated, tolerance 0
    d, _ = directions(SH9, nrm, ids, seed, samples, 0)
    acc = np.zeros((len(pos), 9, 3))
    for k in range(samples):
        acc = acc + c[None, None, :] * rpt_amd.sh9_basis(d[:, k])[:, :, None]
    assert (sh == acc * (FOUR_PI / float(samples))).all()


# ---- 3. the contract
@pytest.mark.parametrize("kind_name", ["sh9", "irradiance"])
def test_a_probes_result_is_its_own(kind_name, monkeypatch, capfd):
    name, samples, kind = "wine_glass", 16, KINDS[kind_name]
    scene = small_scenes.small(name)[0]
    pos, nrm, ids = probes(name)
    n = len(pos)
    g = gpu(name)
    base = bake(g, name, kind, samples)
    assert (base == case(name, kind_name, samples)[0]).all()
    # permuted, probes and stream ids together
    perm = np.random.RandomState(77).permutation(n)
    assert (bake(g, name, kind, samples, pos[perm], nrm[perm], ids[perm]) == base[perm]).all()
    # split over two calls, at an odd place
    k = 7
    assert (bake(g, name, kind, samples, pos[:k], nrm[:k], ids[:k]) == base[:k]).all()
    assert (bake(g, name, kind, samples, pos[k:], nrm[k:], ids[k:]) == base[k:]).all()
    # pieces of 3 probes (the last one of 1), with ids and without
    plain = bake(g, name, kind, samples, streams=None)
    assert (plain == bake(g, name, kind, samples, streams=np.arange(n, dtype=np.uint32))).all()
    assert (plain != base).any()
    monkeypatch.setenv("RPTGPU_PROBES_PIECE", "3")
    g.reset_stats()
    assert (bake(g, name, kind, samples) == base).all()
    assert g.stats().kernel_launches[_abi.RPT_K_RAYGEN] >= (n + 2) // 3 and g.stats().samples == n * samples
    assert (bake(g, name, kind, samples, streams=None) == plain).all()  # probe i of piece k has stream 3 k + i
    assert (bake(g, name, kind, samples, pos[perm], nrm[perm], ids[perm]) == base[perm]).all()
    monkeypatch.delenv("RPTGPU_PROBES_PIECE")
    assert (bake(g, name, kind, samples, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL) == base).all()
    assert (bake(g, name, kind, samples, flags=_abi.RPT_FLAG_PROFILE_KERNELS | _abi.RPT_FLAG_WAVEFRONT) == base).all()
    # a record pool that runs out: the pass starts over and nothing of the failed attempt shows (a fresh handle: the
    # figure is taken when a handle first sees a max_bounces)
    monkeypatch.setenv("RPTGPU_REC_RATIO", "0.01")
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    g2 = GpuScene(scene, 0)
    capfd.readouterr()
    got = bake(g2, name, kind, samples)
    err = capfd.readouterr().err
    st = g2.stats()
    g2.close()
    monkeypatch.delenv("RPTGPU_REC_RATIO")
    monkeypatch.delenv("RPTGPU_PRINT_LAUNCH")
    assert "started over" in err
    assert st.samples == n * samples  # a pass that is started over counts once
    assert (got == base).all()


@pytest.mark.parametrize("kind_name", ["sh9", "irradiance"])
def test_samples_over_several_passes(kind_name, capfd, monkeypatch):
    """passes of at most 1024 paths (the smallest a handle takes): 32 probes x 100 samples run as a measuring pass of one
    sample and four more; the sums cross each border in sample order"""
    kind = KINDS[kind_name]
    scene = small_scenes.small("cornell")[0]
    pos, nrm, ids = probes("cornell", 32)
    kw = dict(kind=kind, samples=100, max_bounces=3, seed=5, streams=ids)
    want = gpu("cornell").bake_probes(pos, nrm if kind == IRR else None, **kw)
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    g = GpuScene(scene, 0, target_paths=1024)
    capfd.readouterr()
    got = g.bake_probes(pos, nrm if kind == IRR else None, **kw)
    err = capfd.readouterr().err
    g.close()
    assert err.count("wavefront pass:") >= 5, err[-600:]
    assert (got == want).all()


@pytest.mark.parametrize("kind_name", ["sh9", "irradiance"])
def test_sample_index_base(kind_name):
    """S = 11 from sample 5 on: the restated sum of samples 5 .. 15"""
    name, kind = "coverage", KINDS[kind_name]
    pos, nrm, ids = probes(name)
    p = small_scenes.small(name)[2]
    g = gpu(name)
    want, _, _ = restated(g, kind, pos, nrm, ids, p.max_bounces, p.seed, 11, base=5)
    got = bake(g, name, kind, 11, sample_index_base=5)
    assert (got == want).all()
    assert (got != bake(g, name, kind, 11)).any()


# ---- 4. the device entry point
@pytest.mark.parametrize("kind_name", ["sh9", "irradiance"])
def test_device_entry_point(kind_name):
    """torch tensors on the GPU in, a tensor on the GPU out: the host entry point's bits, the inputs untouched, and
    nothing written behind [n][27] / [n][3]"""
    name, samples, kind = "wine_glass", 16, KINDS[kind_name]
    want = case(name, kind_name, samples)[0]
    pos, nrm, ids = probes(name)
    n, width = len(pos), 27 if kind == SH9 else 3
    g = gpu(name)
    dev = torch.device("cuda", 0)
    tp, tn = torch.from_numpy(pos.copy()).to(dev), torch.from_numpy(nrm.copy()).to(dev)
    ts = torch.from_numpy(ids.astype(np.int32)).to(dev)
    keep = tp.clone(), tn.clone(), ts.clone()
    got = bake(g, name, kind, samples, tp, tn, ts)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert (got.cpu().numpy() == want).all()
    buf = torch.full((n * width + 64,), 7.0, dtype=torch.float64, device=dev)
    out = buf[:n * width].view(want.shape)
    assert bake(g, name, kind, samples, tp, tn, ts, out=out) is out
    host = buf.cpu().numpy()
    assert (host[:n * width].reshape(want.shape) == want).all() and (host[n * width:] == 7.0).all()
    assert (bake(g, name, kind, samples, tp, tn, None).cpu().numpy() == bake(g, name, kind, samples, streams=None)).all()
    assert torch.equal(tp, keep[0]) and torch.equal(tn, keep[1]) and torch.equal(ts, keep[2])
    with pytest.raises(ValueError):
        bake(g, name, kind, samples, tp, torch.from_numpy(nrm.copy()) if kind == IRR else tn, torch.from_numpy(ids.astype(np.int32)))
    assert tuple(bake(g, name, kind, samples, tp[:0], tn[:0], ts[:0]).shape) == (0,) + want.shape[1:]


# ---- 5. refusals on a live handle
def test_refusals_on_a_live_handle():
    name = "cornell"
    scene, camera, p0 = small_scenes.small(name)
    p = make_params(37, 21, p0.max_bounces, 2, seed=p0.seed, flags=_abi.RPT_FLAG_WAVEFRONT)
    g = gpu(name)
    frame = g.render_batch(camera, p)
    want = {k: bake(g, name, KINDS[k], 16) for k in KINDS}
    pos, nrm, ids = probes(name)
    lib = _abi.load_library()
    PD = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for kind_name, kind in KINDS.items():
        out = np.full(want[kind_name].shape, 7.0)
        for kw, word in ((dict(flags=_abi.RPT_FLAG_PERSISTENT), "RPT_FLAG_PERSISTENT"), (dict(samples=0), "samples == 0"),
                         (dict(max_bounces=255), "max_bounces > 254")):
            args = dict(kind=kind, samples=16, max_bounces=2, seed=1, streams=ids, out=out)
            args.update(kw)
            with pytest.raises(rpt_amd.RptGpuError) as e:
                g.bake_probes(pos, nrm if kind == IRR else None, **args)
            assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
            assert (out == 7.0).all()
    # what the Python wrapper never passes on: an unknown kind, irradiance without normals — straight to the library
    q = _abi.RptProbeQuery()
    q.struct_size, q.kind, q.samples, q.max_bounces, q.seed = C.sizeof(q), 2, 16, 2, 1
    out = np.full((N_PROBES, 27), 7.0)
    assert lib.rptgpu_bake_probes(g.handle, N_PROBES, PD(pos), None, None, C.byref(q), PD(out)) == _abi.RPTGPU_E_INVALID_ARGUMENT
    assert b"unknown kind" in lib.rptgpu_last_error_detail(g.handle)
    q.kind = IRR
    assert lib.rptgpu_bake_probes(g.handle, N_PROBES, PD(pos), None, None, C.byref(q), PD(out)) == _abi.RPTGPU_E_INVALID_ARGUMENT
    assert b"null normals" in lib.rptgpu_last_error_detail(g.handle)
    assert (out == 7.0).all()
    assert g.bake_probes(np.zeros((0, 3)), kind=SH9, samples=4, max_bounces=2, seed=1).shape == (0, 9, 3)  # n == 0
    for kind_name, kind in KINDS.items():
        assert (bake(g, name, kind, 16) == want[kind_name]).all()
    assert (g.render_batch(camera, p) == frame).all()
