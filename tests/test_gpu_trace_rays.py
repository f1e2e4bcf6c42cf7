"""rptgpu_trace_rays on the GPU: the path estimator for rays the caller supplies.

The oracle has no entry point for loose rays, but a path behind its first kernel is an origin, a direction, a Philox
stream and a draw counter: handed the oracle's OWN camera rays (oracle_camera_ray) with the pixel's stream id and the
draw the camera stopped at, the call must return the oracle's frame, bit for bit.  The rest follows from the stream
contract of include/rpt_gpu.h: a ray's result is its own, whatever shares the call.  Tolerance 0 (== on the f64 arrays)
everywhere but in the comparison with the independent Python path tracer, whose limits are that file's."""
import functools

import numpy as np
import pytest

import rpt_amd
from rpt_amd import Camera, GpuScene, _abi, make_params

import small_scenes

pytestmark = pytest.mark.gpu

# the smallest frames that still take more than one 256-thread block, an odd number of them, and (wine_glass, glass: 8
# and 6 bounces over deep trees) paths of every length
SIZES = {"cornell": (37, 21), "coverage": (35, 19), "glass": (33, 23), "wine_glass": (37, 21)}


def pinhole(camera):
    """the scene's camera without its lens (coverage and glass are focused: their rays take more than two draws, which
    is test_depth_of_field's subject)"""
    return Camera(camera.eye, camera.direction, camera.up, camera.fov, 0.0, 0.0)


def camera_rays(oracle, camera, p, s):
    """the oracle's camera ray of every pixel at sample s, the pixel as stream id, and the draws the camera took —
    replayed: the two gen_range of renderer.rs:137-138, then UnitDisc under a lens (camera.rs:71)"""
    w, h = p.width, p.height
    dim = float(max(w, h))
    o, d = np.empty((h * w, 3)), np.empty((h * w, 3))
    draws = np.empty(h * w, dtype=np.uint32)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            o[i], d[i] = oracle.camera_ray(camera, p, x, y, s)
            _, n = oracle.rng_sample(1, -1.0 / dim, 1.0 / dim, seed=p.seed, pixel=i, sample=s, draw=0)
            _, n = oracle.rng_sample(1, -1.0 / dim, 1.0 / dim, seed=p.seed, pixel=i, sample=s, draw=n)
            if camera.aperture > 0.0:
                _, n = oracle.rng_sample(4, seed=p.seed, pixel=i, sample=s, draw=n)
            draws[i] = n
    return o, d, np.arange(h * w, dtype=np.uint32), draws


@functools.lru_cache(maxsize=None)
def case(name, s):
    """(scene, camera, params of ONE sample at index s, the oracle's rays, their streams and draw counts, the oracle's
    frame) — computed once, shared, never written to"""
    from oracle import oracle_ffi as oracle
    scene, camera, p0 = small_scenes.small(name)
    camera = pinhole(camera)
    w, h = SIZES[name]
    p = make_params(w, h, p0.max_bounces, 1, seed=p0.seed, sample_index_base=s)
    o, d, streams, draws = camera_rays(oracle, camera, p, s)
    want = oracle.OracleScene(scene).render(camera, p)
    for a in (o, d, streams, draws, want):
        a.setflags(write=False)
    return scene, camera, p, o, d, streams, draws, want


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(small_scenes.small(name)[0], 0)


def trace(g, p, o, d, **kw):
    kw.setdefault("seed", p.seed)
    kw.setdefault("sample_index_base", p.sample_index_base)
    kw.setdefault("first_draw", 2)
    return g.trace_rays(o, d, p.max_bounces, **kw)


@pytest.mark.parametrize("s", [0, 5])
@pytest.mark.parametrize("name", ["cornell", "coverage", "glass", "wine_glass"])
def test_the_oracles_frame_from_the_oracles_rays(name, s):
    """flat and deep-tree routing, object lights, HDRI misses: the frame of OracleScene.render, tolerance 0"""
    scene, camera, p, o, d, streams, draws, want = case(name, s)
    assert (draws == 2).all()
    g = gpu(name)
    g.reset_stats()
    got = trace(g, p, o, d, streams=streams)
    assert got.shape == want.shape and got.dtype == np.float64
    assert (got == want).all(), "%d of %d rays differ" % ((got != want).any(axis=1).sum(), len(want))
    st = g.stats()
    assert st.samples == len(o) and st.extend_rays >= len(o)
    assert st.kernel_launches[_abi.RPT_K_RAYGEN] >= 1 and st.kernel_launches[_abi.RPT_K_PATHS] == 0  # wavefront only


def test_depth_of_field(oracle):
    """cornell under a lens: UnitDisc rejects, so the rays' streams stop at different draws; one call per draw count
    (first_draw is the call's), every pixel in some group, and the oracle's frame comes out"""
    scene, camera0, p0 = small_scenes.small("cornell")
    camera = pinhole(camera0).focus((278.0, 273.0, 280.0), 20.0)  # the middle of the box, a lens of 20 of its 555 units
    assert camera.aperture > 0.0
    w, h = SIZES["cornell"]
    p = make_params(w, h, p0.max_bounces, 1, seed=p0.seed, sample_index_base=3)
    o, d, streams, draws = camera_rays(oracle, camera, p, 3)
    want = oracle.OracleScene(scene).render(camera, p)
    counts = sorted(set(draws.tolist()))
    assert counts[0] == 4 and len(counts) >= 2  # two draws per attempt at the disc, a fifth of the attempts rejected
    got = np.full_like(want, np.nan)
    done = np.zeros(len(o), dtype=bool)
    for c in counts:
        m = draws == c
        got[m] = trace(gpu("cornell"), p, o[m], d[m], streams=streams[m], first_draw=c)
        done |= m
    assert done.all()
    assert (got == want).all()


def test_a_rays_result_is_its_own(monkeypatch, capfd):
    scene, camera, p, o, d, streams, draws, want = case("wine_glass", 0)
    n = len(o)
    assert n > 200
    g = gpu("wine_glass")
    base = trace(g, p, o, d, streams=streams)
    assert (base == want).all()
    # permuted, rays and streams together
    perm = np.random.RandomState(77).permutation(n)
    assert (trace(g, p, o[perm], d[perm], streams=streams[perm]) == base[perm]).all()
    # split over two calls, at an odd place
    k = 333
    assert (trace(g, p, o[:k], d[:k], streams=streams[:k]) == base[:k]).all()
    assert (trace(g, p, o[k:], d[k:], streams=streams[k:]) == base[k:]).all()
    # without ids a ray's stream is its index in the call's arrays: the same as naming arange(n) — in pieces too
    assert (trace(g, p, o, d) == base).all()
    monkeypatch.setenv("RPTGPU_RAYS_PIECE", "100")
    g.reset_stats()
    assert (trace(g, p, o, d, streams=streams) == base).all()
    pieces = (n + 99) // 100
    assert g.stats().kernel_launches[_abi.RPT_K_RAYGEN] >= pieces and g.stats().samples == n
    assert (trace(g, p, o, d) == base).all()  # ray i of piece k has stream 100 k + i
    assert (trace(g, p, o[perm], d[perm], streams=streams[perm]) == base[perm]).all()
    monkeypatch.delenv("RPTGPU_RAYS_PIECE")
    assert (trace(g, p, o, d, streams=streams, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL) == base).all()
    assert (trace(g, p, o, d, streams=streams, flags=_abi.RPT_FLAG_PROFILE_KERNELS | _abi.RPT_FLAG_WAVEFRONT) == base).all()
    # a record pool that runs out: the pass starts over and nothing of the failed attempt shows (a fresh handle: the
    # figure is taken when a handle first sees a max_bounces)
    monkeypatch.setenv("RPTGPU_REC_RATIO", "0.01")
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    g2 = GpuScene(scene, 0)
    capfd.readouterr()
    got = g2.trace_rays(o, d, p.max_bounces, samples=3, seed=p.seed, sample_index_base=0, streams=streams, first_draw=2)
    err = capfd.readouterr().err
    st = g2.stats()
    g2.close()
    monkeypatch.delenv("RPTGPU_REC_RATIO")
    monkeypatch.delenv("RPTGPU_PRINT_LAUNCH")
    assert "started over" in err
    assert st.samples == 3 * n  # a pass that is started over counts once
    assert (got == g.trace_rays(o, d, p.max_bounces, samples=3, seed=p.seed, sample_index_base=0, streams=streams, first_draw=2)).all()


@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_several_samples(name):
    """sum in sample order, / iterations, * 2^EV — rpt_resolve's and rpt_finish's arithmetic, restated in numpy"""
    scene, camera, p, o, d, streams, draws, want = case(name, 0)
    g = gpu(name)
    L = [trace(g, p, o, d, streams=streams, sample_index_base=b) for b in (8, 9, 10, 11)]
    got = trace(g, p, o, d, streams=streams, samples=4, sample_index_base=8, exposure_value=1.5)
    assert (got == (((L[0] + L[1]) + L[2]) + L[3]) / 4.0 * 2.0 ** 1.5).all()
    assert not (L[0] == L[1]).all()


def sphere_directions(rs, n):
    v = rs.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_rays_that_no_camera_makes(oracle):
    """256 rays from points above the floor into every direction, against tests/test_independent_pathtracer.py's tracer —
    another program in another language with another libm, so its own limits apply: within 1e-9 * max(1, |want|) for at
    least 99 % of the rays (that file: 1500 of 1500 between the tracer and the oracle).
    The shares of rays that agree and that are bit-equal are printed; they have not been recorded on an MI355X yet."""
    import test_independent_pathtracer as T
    import test_independent_shading as H
    seed, n, bounces = 20260, 256, 4
    scene, camera = T.scene_lights_and_shapes()
    rs = np.random.RandomState(seed)
    o = rs.uniform((-2.5, -0.9, -2.5), (2.5, 3.0, 2.5), (n, 3))
    d = sphere_directions(rs, n)
    tr = T.Tracer(scene, camera, 1, 1, bounces)
    want = np.array([tr.trace_ray(o[i], d[i], 0, H.Stream(seed, i, 0, 0)) for i in range(n)])
    g = GpuScene(scene, 0)
    got = g.trace_rays(o, d, bounces, seed=seed)
    g.close()
    tol = 1e-9 * np.maximum(1.0, np.abs(want).max(axis=1))
    close = np.abs(got - want).max(axis=1) <= tol
    same = (got == want).all(axis=1)
    print("independent tracer: %d of %d rays within 1e-9 (%.2f %%), %d bit-equal (%.2f %%)"
          % (close.sum(), n, 100.0 * close.mean(), same.sum(), 100.0 * same.mean()))
    assert np.isfinite(got).all()
    assert close.mean() >= 0.99, (close.mean(), same.mean())
    # a miss is the environment, exactly
    scene, camera = T.scene_glass_and_sky()
    o = rs.uniform((-3.0, -2.0, -3.0), (3.0, 2.0, 3.0), (n, 3))
    d = sphere_directions(rs, n)
    _, _, obj = oracle.OracleScene(scene).closest_hit(o, d)
    miss = obj < 0
    assert 20 < miss.sum() < n
    g = GpuScene(scene, 0)
    got = g.trace_rays(o, d, 6, seed=seed)
    g.close()
    for i in np.flatnonzero(miss):
        assert (got[i] == oracle.env_color(scene.environment, d[i])).all(), i


def test_device_entry_point():
    """torch tensors on the GPU in, a tensor on the GPU out: the host entry point's bits, the inputs untouched"""
    import torch
    scene, camera, p, o, d, streams, draws, want = case("wine_glass", 0)
    g = gpu("wine_glass")
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    ts = torch.from_numpy(streams.astype(np.int32)).to(dev)
    keep = to.clone(), td.clone(), ts.clone()
    got = trace(g, p, to, td, streams=ts)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert (got.cpu().numpy() == want).all()
    out = torch.full((len(o), 3), -1.0, dtype=torch.float64, device=dev)
    assert trace(g, p, to, td, out=out, samples=2) is out  # no ids: the indices
    assert (out.cpu().numpy() == trace(g, p, o, d, samples=2)).all()
    assert torch.equal(to, keep[0]) and torch.equal(td, keep[1]) and torch.equal(ts, keep[2])
    # Rays still being PRODUCED when the call is made: the arrays hold zeros until a copy that stands behind some 30 ms
    # of queued kernels on the producer's stream has run.  The handle's stream is not ordered with any of torch's, so a
    # call that does not wait for the producer reads the zeros and returns other bits.  On torch's default stream (the
    # null stream, which has no handle to give the library: the wrapper waits) and on a stream of its own (the library
    # waits for the handle it is given).
    ballast = torch.ones(64 << 20, dtype=torch.float32, device=dev)
    for stream in (torch.cuda.current_stream(dev), torch.cuda.Stream(dev)):
        late_o, late_d, late_s = torch.zeros_like(to), torch.zeros_like(td), torch.zeros_like(ts)
        stream.wait_stream(torch.cuda.current_stream(dev))  # (the zeros above are there)
        with torch.cuda.stream(stream):
            for _ in range(200):
                ballast.mul_(1.0)
            late_o.copy_(to), late_d.copy_(td), late_s.copy_(ts)
            got = trace(g, p, late_o, late_d, streams=late_s)
        assert (got.cpu().numpy() == want).all(), "default stream" if stream.cuda_stream == 0 else "a stream of its own"
        torch.cuda.current_stream(dev).wait_stream(stream)
    with pytest.raises(ValueError):
        trace(g, p, to, torch.from_numpy(d.copy()))  # a host tensor among device tensors
    assert tuple(g.trace_rays(to[:0], td[:0], 2).shape) == (0, 3)


# (The one refusal of the call that no test reaches is the abandoned handle's, RPTGPU_E_COMM: a handle is abandoned only
# when the device fails to drain an aborted multi-rank batch within the communicator's time-out (api_comm.cpp), and the
# suite has no way to bring that about — nor should it hang a device to get there.  The check is REFUSE_IF_ABANDONED,
# the macro every entry point that enqueues work shares.)
def test_refusals_on_a_live_handle():
    scene, camera, p, o, d, streams, draws, want = case("cornell", 0)
    g = gpu("cornell")
    out = np.full((len(o), 3), 7.0)
    for kw, word in ((dict(flags=_abi.RPT_FLAG_PERSISTENT), "RPT_FLAG_PERSISTENT"), (dict(samples=0), "iterations == 0")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            trace(g, p, o, d, streams=streams, out=out, **kw)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
        assert (out == 7.0).all()
    assert g.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)), 2).shape == (0, 3)  # n == 0: nothing to do
    assert (g.render_batch(camera, p) == want).all()
    assert (trace(g, p, o, d, streams=streams) == want).all()
