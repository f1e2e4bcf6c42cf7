"""rptgpu_trace_vertices on the GPU: the vertices of the paths rptgpu_trace_rays runs (include/rpt_gpu_vertices.h).

Every bit of the call is defined by entry points that already exist, so every check is one of them restated, tolerance 0:
RGB is rptgpu_trace_rays' output (and, one sample of the oracle's own camera rays, the oracle's frame); the fold of the
exported factors in numpy is RGB; every vertex is rptgpu_first_hits of the ray that ends there, and that ray starts where the
vertex before it lies; rptgpu_trace_rays continued from a vertex with the stream at the exported draw returns the suffix of
the fold.  The rays are test_gpu_trace_rays' — the oracle's camera rays at that file's sizes, so the paths are a real
frame's —, at the scenes' own max_bounces, 3 samples from sample index 5.
(Restated device calls cannot see a factor that every one of them multiplies by a zero suffix, nor a draw counter that is off
in all of them alike: tests/test_gpu_vertices_oracle.py holds the same vertices to the oracle's records and functions.)"""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, _abi

import small_scenes
import test_gpu_trace_rays as R

pytestmark = pytest.mark.gpu

NAMES = ["cornell", "coverage", "glass", "wine_glass"]
SAMPLES, BASE = 3, 5
ALL = _abi.RPT_VERTEX_ALL
PER_VERTEX = ("t", "normal", "object", "position", "direction", "draw", "radiance", "bsdf", "inv_pdf", "abs_cos")
BITS = {"length": _abi.RPT_VERTEX_LENGTH, "t": _abi.RPT_VERTEX_T, "normal": _abi.RPT_VERTEX_NORMAL, "object": _abi.RPT_VERTEX_OBJECT,
        "position": _abi.RPT_VERTEX_POSITION, "direction": _abi.RPT_VERTEX_DIRECTION, "draw": _abi.RPT_VERTEX_DRAW,
        "radiance": _abi.RPT_VERTEX_RADIANCE, "bsdf": _abi.RPT_VERTEX_BSDF, "inv_pdf": _abi.RPT_VERTEX_INV_PDF,
        "abs_cos": _abi.RPT_VERTEX_ABS_COS, "rgb": _abi.RPT_VERTEX_RGB}


def bits(a):
    """the raw bits of an array: -0.0 != +0.0, a NaN equals the same NaN"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def differing(got, want):
    """the channels of two results (PathVertices, or dicts of arrays) whose bits differ"""
    got, want = (x.arrays() if hasattr(x, "arrays") else x for x in (got, want))
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or not same(got[k], want[k]))


def rays(name):
    """the oracle's camera rays of sample 5 and the pixels as stream ids"""
    scene, camera, p, o, d, streams, draws, want = R.case(name, BASE)
    return p, o, d, streams


def vertices(g, name, o=None, d=None, streams=None, **kw):
    p, o0, d0, s0 = rays(name)
    kw.setdefault("samples", SAMPLES)
    kw.setdefault("seed", p.seed)
    kw.setdefault("sample_index_base", BASE)
    kw.setdefault("first_draw", 2)
    return g.trace_vertices(o0 if o is None else o, d0 if d is None else d, p.max_bounces, streams=s0 if o is None else streams, **kw)


@functools.lru_cache(maxsize=None)
def base(name):
    """every channel of the scene's rays on the shared handle — computed once, shared, never written to"""
    v = vertices(R.gpu(name), name)
    for a in v.arrays().values():
        a.setflags(write=False)
    return v


def fold(v):
    """the header's fold over the exported channels -> (L [n][S][B+1][3]: the suffix value L_d at every vertex d < len, +0.0
    behind it; the sum over the samples in ascending order from +0.0)"""
    n, S, V = v.t.shape
    L = np.zeros((n, S, V, 3))
    with np.errstate(all="ignore"):
        for d in range(V - 1, -1, -1):
            last, inner = v.length - 1 == d, v.length - 1 > d
            L[last, d] = v.radiance[last, d]
            if d + 1 < V:
                ind = (v.inv_pdf[:, :, d, None] * (v.bsdf[:, :, d] * L[:, :, d + 1])) * v.abs_cos[:, :, d, None]
                val = v.radiance[:, :, d] + np.fmin(ind, 100.0)  # C's fmin: the other operand for a NaN
                L[inner, d] = val[inner]
        acc = np.zeros((n, 3))
        for s in range(S):
            acc = acc + L[:, s, 0]
    return L, acc


# ---- 1. RGB is rptgpu_trace_rays'
@pytest.mark.parametrize("name", NAMES)
def test_rgb_is_trace_rays(name):
    p, o, d, streams = rays(name)
    g = R.gpu(name)
    want = g.trace_rays(o, d, p.max_bounces, samples=SAMPLES, seed=p.seed, sample_index_base=BASE, streams=streams, first_draw=2)
    v = base(name)
    assert v.rgb.shape == want.shape and v.rgb.dtype == np.float64
    assert (v.rgb == want).all(), "%d of %d rays differ" % ((v.rgb != want).any(axis=1).sum(), len(want))
    if name == "cornell":  # one sample: the oracle's frame
        one = vertices(g, name, samples=1, channels=_abi.RPT_VERTEX_RGB | _abi.RPT_VERTEX_LENGTH)
        assert (one.rgb == R.case(name, BASE)[7]).all()
        assert (one.length == v.length[:, :1]).all()


# ---- 2. the fold
@pytest.mark.parametrize("name", NAMES)
def test_the_fold_of_the_exported_factors_is_rgb(name):
    p = rays(name)[0]
    v = base(name)
    n, B = len(v.rgb), p.max_bounces
    assert v.length.shape == (n, SAMPLES) and v.length.dtype == np.uint32 and v.t.shape == (n, SAMPLES, B + 1)
    assert v.length.min() >= 1 and v.length.max() <= B + 1
    L, acc = fold(v)
    assert (acc / SAMPLES * 2.0 ** 0.0 == v.rgb).all(), "%d rays differ" % (acc / SAMPLES != v.rgb).any(axis=1).sum()
    lengths = np.unique(v.length)
    print("%s: lengths %s, counts %s" % (name, lengths.tolist(), np.bincount(v.length.ravel())[lengths].tolist()))
    if name in ("glass", "wine_glass"):
        assert len(lengths) >= 3  # (not on trivial paths)
    # under an exposure value the scale comes last
    ev = vertices(R.gpu(name), name, channels=_abi.RPT_VERTEX_RGB, exposure_value=1.5)
    assert (ev.rgb == acc / SAMPLES * 2.0 ** 1.5).all()


# ---- 3. the chain
@pytest.mark.parametrize("name", NAMES)
def test_every_vertex_is_the_first_hit_of_the_ray_that_ends_there(name):
    p, o, d, streams = rays(name)
    v = base(name)
    n, S, V = v.t.shape
    depth = np.arange(V)[None, None, :]
    valid = depth < v.length[:, :, None]
    assert (v.draw[:, :, 0] == 2).all() and v.draw.dtype == np.uint32 and v.object.dtype == np.int32
    assert same(v.direction[:, :, 0], np.broadcast_to(d[:, None, :], (n, S, 3)).copy())
    # origin_d: the caller's origin, then the position of the vertex before
    origin = np.concatenate([np.broadcast_to(o[:, None, None, :], (n, S, 1, 3)), v.position[:, :, :-1]], axis=2)
    # the escape vertex is a path's last, and a path that ends early on a surface ended there by itself
    assert (v.object[valid & (depth < v.length[:, :, None] - 1)] >= 0).all()
    assert ((v.object < 0) & valid).any() or name == "cornell"
    hit = R.gpu(name).first_hits(origin[valid], v.direction[valid],
                                 channels=_abi.RPT_HIT_T | _abi.RPT_HIT_NORMAL | _abi.RPT_HIT_OBJECT | _abi.RPT_HIT_POSITION)
    got = {k: getattr(v, k)[valid] for k in ("t", "normal", "object", "position")}
    assert differing(got, hit) == [], "of %d vertices" % valid.sum()
    miss = got["object"] < 0
    assert np.isposinf(got["t"][miss]).all() and not bits(got["position"][miss]).any()


# ---- 4. continuation
@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_a_path_continues_from_any_vertex(name):
    """trace_rays from (origin_d, dir_d) with the path's stream at DRAW_d, B - d bounces and the path's sample index is the
    suffix L_d of the fold: one call per (d, draw, sample), every vertex d >= 1 of the chosen rays in exactly one of them"""
    p, o, d, streams = rays(name)
    v = base(name)
    B = p.max_bounces
    L, _ = fold(v)
    # 64 rays from the middle of the frame on, the first ones chosen so that three lengths are there
    longest = v.length.max(axis=1)
    picked = []
    for want in np.unique(longest)[::-1][:3]:
        picked.append(int(np.flatnonzero(longest == want)[0]))
    picked += [i for i in range(len(o) // 2, len(o)) if i not in picked][:64 - len(picked)]
    picked = np.array(sorted(picked))
    assert len(picked) >= 64 and len(np.unique(v.length[picked])) >= 3
    g = R.gpu(name)
    todo = [(int(i), s, dd) for i in picked for s in range(SAMPLES) for dd in range(1, int(v.length[i, s]))]
    assert len(todo) >= 64
    groups = {}
    for i, s, dd in todo:
        groups.setdefault((dd, int(v.draw[i, s, dd]), s), []).append(i)
    done = 0
    for (dd, draw, s), idx in sorted(groups.items()):
        idx = np.array(idx)
        got = g.trace_rays(v.position[idx, s, dd - 1], v.direction[idx, s, dd], B - dd, samples=1, seed=p.seed,
                           sample_index_base=BASE + s, streams=streams[idx], first_draw=draw)
        assert (got == L[idx, s, dd]).all(), (dd, draw, s)
        done += len(idx)
    assert done == len(todo)
    print("%s: %d vertices of %d rays continued in %d calls" % (name, done, len(picked), len(groups)))


# ---- 5. a path's records are its own
def test_a_paths_records_are_its_own(monkeypatch, capfd):
    name = "wine_glass"
    p, o, d, streams = rays(name)
    scene = small_scenes.small(name)[0]
    n = len(o)
    g = R.gpu(name)
    want = base(name)
    rows = lambda v, sel: {k: a[sel] for k, a in v.arrays().items()}
    # permuted, rays and streams together
    perm = np.random.RandomState(78).permutation(n)
    assert differing(vertices(g, name, o[perm], d[perm], streams[perm]), rows(want, perm)) == []
    # split over two calls, at an odd place
    k = 333
    assert differing(vertices(g, name, o[:k], d[:k], streams[:k]), rows(want, slice(0, k))) == []
    assert differing(vertices(g, name, o[k:], d[k:], streams[k:]), rows(want, slice(k, n))) == []
    # in pieces — and without ids, where ray i of piece k has stream 100 k + i
    by_index = vertices(g, name, o, d, None)
    monkeypatch.setenv("RPTGPU_VERTICES_PIECE", "100")
    g.reset_stats()
    assert differing(vertices(g, name), want) == []
    assert g.stats().kernel_launches[_abi.RPT_K_RAYGEN] >= (n + 99) // 100 and g.stats().samples == n * SAMPLES
    assert differing(vertices(g, name, o, d, None), by_index) == []
    assert differing(vertices(g, name, o[perm], d[perm], streams[perm]), rows(want, perm)) == []
    monkeypatch.delenv("RPTGPU_VERTICES_PIECE")
    # with streams that are the indices, and without: the same
    assert differing(vertices(g, name, o, d, np.arange(n, dtype=np.uint32)), by_index) == []
    assert differing(by_index, want) == []  # (the pixels ARE the indices here)
    assert differing(vertices(g, name, o[perm], d[perm], None), rows(want, perm)) != []  # ... and other ids are other paths
    assert differing(vertices(g, name, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL), want) == []
    assert differing(vertices(g, name, flags=_abi.RPT_FLAG_PROFILE_KERNELS | _abi.RPT_FLAG_WAVEFRONT), want) == []
    # a record pool that runs out: the pass starts over after some depths stored their vertices, and nothing of the
    # failed attempt shows (a fresh handle: the figure is taken when a handle first sees a max_bounces)
    monkeypatch.setenv("RPTGPU_REC_RATIO", "0.01")
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    g2 = GpuScene(scene, 0)
    capfd.readouterr()
    got = vertices(g2, name)
    err = capfd.readouterr().err
    st = g2.stats()
    g2.close()
    monkeypatch.delenv("RPTGPU_REC_RATIO")
    assert "started over" in err
    assert st.samples == SAMPLES * n  # a pass that is started over counts once
    assert differing(got, want) == []
    # passes of at most 1024 paths: the piece's three samples take three passes, each writing its own sample's entries
    g3 = GpuScene(scene, 0, target_paths=1024)
    capfd.readouterr()
    got = vertices(g3, name)
    err = capfd.readouterr().err
    g3.close()
    monkeypatch.delenv("RPTGPU_PRINT_LAUNCH")
    assert err.count("wavefront pass:") >= 3, err[-600:]
    assert differing(got, want) == []


@pytest.mark.parametrize("name", ["wine_glass", "coverage"])
def test_the_path_reorder_is_scheduling_only(name, monkeypatch):
    """every tree in-kernel and the paths of every depth re-ordered by ray key (threshold 1 path): pid travels with the state"""
    monkeypatch.setenv("RPTGPU_PATH_REORDER", "1")
    monkeypatch.setenv("RPTGPU_PATH_REORDER_MIN", "1")
    monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "1000")
    g = GpuScene(small_scenes.small(name)[0], 0)
    got = vertices(g, name)
    g.close()
    assert differing(got, base(name)) == []


# ---- 6. channel subsets
SUBSETS = [_abi.RPT_VERTEX_LENGTH | _abi.RPT_VERTEX_RGB, _abi.RPT_VERTEX_OBJECT, _abi.RPT_VERTEX_POSITION, _abi.RPT_VERTEX_DIRECTION | _abi.RPT_VERTEX_DRAW,
           _abi.RPT_VERTEX_RADIANCE | _abi.RPT_VERTEX_ABS_COS, _abi.RPT_VERTEX_T | _abi.RPT_VERTEX_NORMAL | _abi.RPT_VERTEX_BSDF | _abi.RPT_VERTEX_INV_PDF,
           _abi.RPT_VERTEX_RGB]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("channels", SUBSETS)
def test_channel_subsets(channels, device):
    """through the C entry points with sentinel-filled arrays behind EVERY pointer: a named channel gets the all-channel
    call's bits, an unnamed one keeps its sentinel"""
    import ctypes as C
    name = "glass"
    p, o, d, streams = rays(name)
    want = base(name).arrays()
    g = R.gpu(name)
    dev = torch.device("cuda", 0)
    q = _abi.RptVertexQuery()
    q.struct_size, q.max_bounces, q.iterations, q.first_draw = C.sizeof(q), p.max_bounces, SAMPLES, 2
    q.seed, q.sample_index_base, q.channels = p.seed, BASE, channels
    a = _abi.RptVertexArrays()
    a.struct_size = C.sizeof(a)
    types = dict(_abi.RptVertexArrays._fields_)
    outs = {}
    for k, w in want.items():
        sentinel = np.full(w.shape, 7, dtype=w.dtype)
        if device:  # (u32 travels as i32: the same bits)
            sentinel = sentinel.view(np.int32) if sentinel.dtype == np.uint32 else sentinel
        outs[k] = torch.from_numpy(sentinel).to(dev) if device else sentinel
        setattr(a, k, C.cast(C.c_void_p(outs[k].data_ptr() if device else outs[k].ctypes.data), types[k]))
    if device:
        to, td, ts = (torch.from_numpy(np.array(x)).to(dev) for x in (o, d, streams.astype(np.int32)))
        torch.cuda.synchronize()
        rc = g.lib.rptgpu_trace_vertices_device(g.handle, len(o), C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()),
                                                C.c_void_p(ts.data_ptr()), C.byref(q), C.byref(a), None)
        outs = {k: t.cpu().numpy().view(want[k].dtype) for k, t in outs.items()}
    else:
        PD = C.POINTER(C.c_double)
        rc = g.lib.rptgpu_trace_vertices(g.handle, len(o), o.ctypes.data_as(PD), d.ctypes.data_as(PD),
                                         streams.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(q), C.byref(a))
    _abi.check(rc, g.handle)
    for k, w in want.items():
        if channels & BITS[k]:
            assert same(outs[k], w), k
        else:
            assert (outs[k] == 7).all(), k


def test_one_channel_of_a_host_caller_in_pieces_of_three(monkeypatch):
    """7 rays in pieces of 3 — the last holds one —, NORMAL alone (not the first channel, three components), against the same
    rays in one piece with every channel: a wrong staging offset, component count or row of the channel table shows"""
    name = "cornell"
    p, o, d, streams = rays(name)
    g = R.gpu(name)
    o, d, streams = (np.ascontiguousarray(x[:7]) for x in (o, d, streams))
    whole = vertices(g, name, o, d, streams).arrays()
    monkeypatch.setenv("RPTGPU_VERTICES_PIECE", "3")
    got = vertices(g, name, o, d, streams, channels=_abi.RPT_VERTEX_NORMAL).arrays()
    assert differing(got, {"normal": whole["normal"]}) == []
    assert differing(whole, {k: a[:7] for k, a in base(name).arrays().items()}) == []


def test_the_filler():
    v = base("glass")
    n, S, V = v.t.shape
    behind = np.arange(V)[None, None, :] >= v.length[:, :, None]
    assert behind.any() and (~behind).any()
    for k in PER_VERTEX:
        a = getattr(v, k)[behind]
        if k == "object":
            assert (a == -1).all()
        else:
            assert not bits(a).any(), k  # +0.0, draw 0
    # ... and at a path's last vertex the three factors are +0.0
    last = np.arange(V)[None, None, :] == v.length[:, :, None] - 1
    for k in ("bsdf", "inv_pdf", "abs_cos"):
        assert not bits(getattr(v, k)[last]).any(), k
    inner = np.arange(V)[None, None, :] < v.length[:, :, None] - 1
    assert (v.inv_pdf[inner] > 0).all()


# ---- 7. the device form
def test_device_entry_point():
    """torch tensors on the GPU in, tensors on the GPU out: the host entry point's bits, the inputs untouched"""
    name = "wine_glass"
    p, o, d, streams = rays(name)
    g = R.gpu(name)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    ts = torch.from_numpy(streams.astype(np.int32)).to(dev)
    keep = to.clone(), td.clone(), ts.clone()
    got = vertices(g, name, to, td, ts)
    assert got.channels == ALL and all(isinstance(t, torch.Tensor) and t.device == dev for t in got.arrays().values())
    want = base(name).arrays()
    for k, t in got.arrays().items():
        a = t.cpu().numpy()
        if k in ("length", "draw"):
            a = a.view(np.uint32)
        assert same(a, want[k]), k
    assert torch.equal(to, keep[0]) and torch.equal(td, keep[1]) and torch.equal(ts, keep[2])
    # rays still being produced on a stream of their own when the call is made: the library waits for the stream it is given
    stream = torch.cuda.Stream(dev)
    ballast = torch.ones(32 << 20, dtype=torch.float32, device=dev)
    late_o, late_d = torch.zeros_like(to), torch.zeros_like(td)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for _ in range(100):
            ballast.mul_(1.0)
        late_o.copy_(to), late_d.copy_(td)
        late = vertices(g, name, late_o, late_d, ts, channels=_abi.RPT_VERTEX_RGB | _abi.RPT_VERTEX_LENGTH)
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert same(late.rgb.cpu().numpy(), want["rgb"]) and same(late.length.cpu().numpy().view(np.uint32), want["length"])
    with pytest.raises(ValueError):
        vertices(g, name, to, torch.from_numpy(d.copy()), ts)  # a host tensor among device tensors
    none = g.trace_vertices(to[:0], td[:0], 2)
    assert tuple(none.t.shape) == (0, 1, 3) and tuple(none.rgb.shape) == (0, 3)


# ---- 8. stats
def test_stats_advance_as_for_trace_rays():
    name = "coverage"
    p, o, d, streams = rays(name)
    g = R.gpu(name)
    base(name)  # (the handle has measured its record ratio: both calls below take the same passes)
    g.reset_stats()
    g.trace_rays(o, d, p.max_bounces, samples=SAMPLES, seed=p.seed, sample_index_base=BASE, streams=streams, first_draw=2)
    st = g.stats()
    rays_counts = (st.samples, st.extend_rays, st.shadow_rays, st.shadow_rays_traced, [int(x) for x in st.kernel_launches])
    g.reset_stats()
    vertices(g, name)
    st = g.stats()
    assert st.samples == len(o) * SAMPLES and st.kernel_launches[_abi.RPT_K_PATHS] == 0
    assert (st.samples, st.extend_rays, st.shadow_rays, st.shadow_rays_traced, [int(x) for x in st.kernel_launches]) == rays_counts


# ---- 9. refusals
def test_refusals_on_a_live_handle():
    name = "cornell"
    scene, camera, p, o, d, streams, draws, want = R.case(name, BASE)
    g = R.gpu(name)
    for kw, word in ((dict(flags=_abi.RPT_FLAG_PERSISTENT), "RPT_FLAG_PERSISTENT"), (dict(samples=0), "iterations == 0"),
                     (dict(channels=0), "channels == 0"), (dict(channels=1 << 12), "unknown RPT_VERTEX_")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            vertices(g, name, **kw)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
    none = g.trace_vertices(np.zeros((0, 3)), np.zeros((0, 3)), 2)  # n == 0: nothing to do
    assert none.t.shape == (0, 1, 3) and none.length.shape == (0, 1)
    assert (g.render_batch(camera, p) == want).all()
    assert differing(vertices(g, name), base(name)) == []
