"""RPT_FLAG_VERTICES_PERSISTENT on the GPU (include/rpt_gpu_vertices_persistent.h): rptgpu_trace_vertices in
the persistent path kernel, rpt_paths_vertices.  Tolerance 0 everywhere — raw bytes, a NaN equal to the same NaN, no vertex
skipped: the flagged call writes the bytes of the unflagged call of the same arguments — the wavefront pipeline's — into
every named array, and on the oracle's own rays the oracle's records and frame.

The scenes, and the instantiation each reaches (the names RPTGPU_PRINT_LAUNCH prints as `rpt_paths_vertices<...>`; the form
has the plain hand-out only, so no line names the fused query or the pool):
  cornell     rpt_paths_vertices<KdFlat>
  glass       rpt_paths_vertices<KdFlatG> + parked environment lookups
  wine_glass  rpt_paths_vertices<KdLds> (deep trees: the general form)
  KdFlatF     tests/test_gpu_parity.py's polygon room behind the object filter
  monomial    the extended shape set: kernels_vertices_strict_ext (KdFlatG, parked)
Shapes: the 777 camera rays of a 37x21 frame (twelve waves and nine lanes), 65, 5 and 1 rays; 3 samples from sample index 5
at the scenes' own max_bounces.  Every flagged call is held to the route by its stats (test_gpu_rays_persistent.on_route)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

from rpt_amd import GpuScene, Material, Object, _abi, cube, hex_color, make_params, scenes

import shading_matrix as M
import small_scenes
import test_gpu_rays_persistent as RP
import test_gpu_trace_rays as TR
import test_gpu_vertices as V
import test_gpu_vertices_oracle as VO
import test_shading_matrix_host as H

pytestmark = pytest.mark.gpu

FLAG = getattr(_abi, "RPT_FLAG_VERTICES_PERSISTENT", 64)
NAMES = ("cornell", "glass", "wine_glass", "KdFlatF", "monomial")
SAMPLES, BASE = 3, 5
N = 777


def call(g, name, sel=slice(None), streams="ids", **kw):
    _, o, d, ids, bounces, seed = RP.rays(name)
    kw.setdefault("samples", SAMPLES)
    kw.setdefault("seed", seed)
    kw.setdefault("sample_index_base", BASE)
    kw.setdefault("first_draw", 2)
    return g.trace_vertices(o[sel], d[sel], kw.pop("max_bounces", bounces), streams=ids[sel] if isinstance(streams, str) else streams, **kw)


def flagged(g, name, sel=slice(None), min_launches=1, **kw):
    """the flagged call, held to the route: the samples, rpt_paths' launches and rays, and no wavefront launch"""
    g.reset_stats()
    v = call(g, name, sel, flags=FLAG | kw.pop("flags", 0), **kw)
    n = len(RP.rays(name)[1][sel])
    RP.on_route(g, n, kw.get("samples", SAMPLES), min_launches)
    return v


@functools.lru_cache(maxsize=None)
def reference(name, first_draw=2):
    """the unflagged call over all rays, every channel — computed once, shared, never written to"""
    v = call(RP.gpu(name), name, first_draw=first_draw)
    for a in v.arrays().values():
        a.setflags(write=False)
    assert v.length.min() >= 1 and np.isfinite(v.rgb).all() and (v.rgb != 0).any()
    return v


def rows(v, sel):
    return {k: a[sel] for k, a in v.arrays().items()}


def test_the_library_reads_the_flag():
    assert _abi.vertices_persistent_supported()


# (name -> the instantiation's name, what its launch line says, what it does not say)
LAUNCH_LINES = {
    "cornell": ("KdFlat", (), ("one query", "scene constants", "wave-level pool", "parked")),
    "glass": ("KdFlatG", ("parked environment lookups",), ("one query", "wave-level pool")),
    "wine_glass": ("KdLds", (), ("parked", "one query", "wave-level pool")),
    "KdFlatF": ("KdFlatF", (), ("parked", "one query", "wave-level pool")),
    "monomial": ("KdFlatG", ("parked environment lookups",), ("one query", "wave-level pool")),
}


@pytest.mark.parametrize("name", NAMES)
def test_the_instantiation_each_scene_reaches(name, monkeypatch, capfd):
    kernel, says, says_not = LAUNCH_LINES[name]
    g = RP.gpu(name)
    want = reference(name)
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    capfd.readouterr()
    got = flagged(g, name)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths")]
    monkeypatch.delenv("RPTGPU_PRINT_LAUNCH")
    kernels = [ln for ln in lines if "blocks/CU" in ln]
    assert len(kernels) == 1 and kernels[0].startswith("rpt_paths_vertices<%s>:" % kernel), lines
    assert all(w in kernels[0] for w in says) and not any(w in kernels[0] for w in says_not), kernels[0]
    assert V.differing(got, want) == []


# ---- flagged == unflagged
@pytest.mark.parametrize("first_draw", [0, 2, 5])
@pytest.mark.parametrize("name", NAMES)
def test_flagged_is_unflagged(name, first_draw):
    """all twelve channels; a stream that starts at draw 0, 2 and 5 (odd: the cached half of a Philox block)"""
    want = reference(name, first_draw)
    got = flagged(RP.gpu(name), name, first_draw=first_draw)
    assert got.channels == _abi.RPT_VERTEX_ALL and got.t.shape == (N, SAMPLES, RP.rays(name)[4] + 1)
    bad = V.differing(got, want)
    assert bad == [], {k: int((V.bits(getattr(got, k)) != V.bits(getattr(want, k))).sum()) for k in bad}
    assert (got.draw[:, :, 0] == first_draw).all()
    if first_draw != 2:
        assert V.differing(want, reference(name, 2)) != []
    if name in ("glass", "wine_glass"):
        assert len(np.unique(want.length)) >= 3  # (not on trivial paths)


@pytest.mark.parametrize("name", NAMES)
def test_a_paths_records_are_its_own(name, monkeypatch):
    """streams given, permuted and NULL; a call split in two; pieces of 100 (rpt_rays_ids names the streams of a piece)"""
    g = RP.gpu(name)
    want = reference(name)
    perm = np.random.RandomState(79).permutation(N)
    assert V.differing(flagged(g, name, perm), rows(want, perm)) == []
    assert V.differing(flagged(g, name, streams=None), want) == []  # the oracle's streams are the indices
    k = 333
    assert V.differing(flagged(g, name, slice(0, k)), rows(want, slice(0, k))) == []
    assert V.differing(flagged(g, name, slice(k, N)), rows(want, slice(k, N))) == []
    monkeypatch.setenv("RPTGPU_VERTICES_PIECE", "100")
    pieces = (N + 99) // 100
    assert V.differing(flagged(g, name, min_launches=pieces), want) == []
    assert V.differing(flagged(g, name, streams=None, min_launches=pieces), want) == []  # ray i of piece k has stream 100 k + i
    assert V.differing(flagged(g, name, perm, min_launches=pieces), rows(want, perm)) == []


@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"])
def test_work_items_of_one_and_two_samples(name, chunk):
    """one path's samples spread over lanes: every lane writes its own sample's entries"""
    g = RP.make_gpu(name, paths_chunk=chunk)
    try:
        got = flagged(g, name)
    finally:
        g.close()
    assert V.differing(got, reference(name)) == []


@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"])
def test_three_launches_per_piece(name):
    """5 samples and a per-sample radiance buffer with room for TWO samples of the piece: exactly three launches of 2, 2 and 1
    samples, whose vertices go to the entries of samples s_first = 0, 2 and 4 on"""
    want = call(RP.gpu(name), name, samples=5)
    g = RP.make_gpu(name, lbuf_bytes=N * 24 * 2)
    try:
        got = flagged(g, name, samples=5, min_launches=3)
        assert g.stats().kernel_launches[_abi.RPT_K_PATHS] == 3
    finally:
        g.close()
    assert V.differing(got, want) == []
    assert V.differing(rows(want, (slice(None), slice(0, 3))), rows(reference(name), (slice(None), slice(0, 3)))) == ["rgb"]


@pytest.mark.parametrize("name", ["cornell", "glass", "monomial"])
def test_sample_base_across_the_32_bit_boundary(name):
    g = RP.gpu(name)
    want = call(g, name, sample_index_base=2 ** 32 - 2)
    assert V.differing(flagged(g, name, sample_index_base=2 ** 32 - 2), want) == []
    assert V.differing(want, reference(name)) != []


@pytest.mark.parametrize("name", ["cornell", "glass", "KdFlatF"])
def test_no_bounces(name):
    """max_bounces 0: one vertex per path, a stride of 1"""
    g = RP.gpu(name)
    want = call(g, name, max_bounces=0)
    got = flagged(g, name, max_bounces=0)
    assert got.t.shape == (N, SAMPLES, 1) and (got.length == 1).all()
    assert V.differing(got, want) == []


@pytest.mark.parametrize("n", [1, 5, 65])
@pytest.mark.parametrize("name", ["cornell", "glass", "KdFlatF"])
def test_less_than_a_wave_and_a_wave_and_a_lane(name, n):
    sel = slice(300, 300 + n)
    assert V.differing(flagged(RP.gpu(name), name, sel), rows(reference(name), sel)) == []


@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"])
def test_general_traversal_and_profiling(name):
    g = RP.gpu(name)
    assert V.differing(flagged(g, name, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL), reference(name)) == []
    assert V.differing(flagged(g, name, flags=_abi.RPT_FLAG_PROFILE_KERNELS), reference(name)) == []


# ---- channel subsets
POISON = 0x10  # a pointer that is neither NULL nor anybody's memory: a channel that is not named has its pointer never read


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("channels", V.SUBSETS)
def test_channel_subsets(channels, device):
    """through the C entry points, twice: with sentinel-filled arrays behind EVERY pointer — a named channel gets the
    all-channel call's bytes, an unnamed one keeps its sentinel — and with a poisoned non-NULL pointer in the place of every
    channel that is not named"""
    name = "glass"
    _, o, d, streams, bounces, seed = RP.rays(name)
    want = reference(name).arrays()
    g = RP.gpu(name)
    dev = torch.device("cuda", 0)
    q = _abi.RptVertexQuery()
    q.struct_size, q.max_bounces, q.iterations, q.first_draw = C.sizeof(q), bounces, SAMPLES, 2
    q.seed, q.sample_index_base, q.channels, q.flags = seed, BASE, channels, FLAG
    types = dict(_abi.RptVertexArrays._fields_)
    for poisoned in (False, True):
        a = _abi.RptVertexArrays()
        a.struct_size = C.sizeof(a)
        outs = {}
        for k, w in want.items():
            sentinel = np.full(w.shape, 7, dtype=w.dtype)
            if device:  # (u32 travels as i32: the same bits)
                sentinel = sentinel.view(np.int32) if sentinel.dtype == np.uint32 else sentinel
            outs[k] = torch.from_numpy(sentinel).to(dev) if device else sentinel
            where = outs[k].data_ptr() if device else outs[k].ctypes.data
            setattr(a, k, C.cast(C.c_void_p(POISON if poisoned and not channels & V.BITS[k] else where), types[k]))
        g.reset_stats()
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
        RP.on_route(g, len(o), SAMPLES)
        for k, w in want.items():
            if channels & V.BITS[k]:
                assert V.same(outs[k], w), (k, poisoned)
            else:
                assert (outs[k] == 7).all(), (k, poisoned)


# ---- the device form
@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_device_entry_point_on_torch_tensors(name):
    _, o, d, ids, bounces, seed = RP.rays(name)
    g = RP.gpu(name)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    ts = torch.from_numpy(ids.astype(np.int32)).to(dev)
    keep = to.clone(), td.clone(), ts.clone()
    g.reset_stats()
    got = g.trace_vertices(to, td, bounces, streams=ts, samples=SAMPLES, seed=seed, sample_index_base=BASE, first_draw=2, flags=FLAG)
    RP.on_route(g, N, SAMPLES)
    assert got.channels == _abi.RPT_VERTEX_ALL and all(isinstance(t, torch.Tensor) and t.device == dev for t in got.arrays().values())
    want = reference(name).arrays()
    for k, t in got.arrays().items():
        a = t.cpu().numpy()
        if k in ("length", "draw"):
            a = a.view(np.uint32)
        assert V.same(a, want[k]), k
    assert torch.equal(to, keep[0]) and torch.equal(td, keep[1]) and torch.equal(ts, keep[2])


# ---- a scene the persistent kernel cannot walk
def test_a_group_with_tree_children_runs_the_wavefront_route(oracle):
    scene, camera, p0 = small_scenes.small("fractal_teapots")
    p = make_params(21, 13, p0.max_bounces, 1, seed=p0.seed)
    o, d, streams, _ = TR.camera_rays(oracle, TR.pinhole(camera), p, 0)
    g = GpuScene(scene, 0)
    try:
        kw = dict(samples=2, seed=p.seed, streams=streams, first_draw=2)
        want = g.trace_vertices(o, d, p.max_bounces, **kw)
        g.reset_stats()
        got = g.trace_vertices(o, d, p.max_bounces, flags=FLAG, **kw)
        st = g.stats()
    finally:
        g.close()
    assert st.kernel_launches[_abi.RPT_K_PATHS] == 0 and st.kernel_launches[_abi.RPT_K_RAYGEN] >= 1 and st.samples == 2 * len(o)
    assert V.differing(got, want) == [] and (want.rgb != 0).any()


# ---- after a live update
def test_after_a_live_update():
    """set_objects on a warm handle of the Cornell box: the flagged call's bytes are a fresh handle's, flagged and not"""
    def moved():
        scene, _, _ = scenes.cornell()
        scene.objects[6] = Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(0.4).translate((300.0, 120.0, 140.0))) \
            .material(Material.diffuse(hex_color(0x3366CC)))
        return scene
    g = GpuScene(scenes.cornell()[0], 0)
    fresh = GpuScene(moved(), 0)
    try:
        before = flagged(g, "cornell")
        g.set_objects([6], [moved().objects[6]])
        got = flagged(g, "cornell")
        want = flagged(fresh, "cornell")
        unflagged = call(fresh, "cornell")
    finally:
        g.close()
        fresh.close()
    assert V.differing(got, want) == [] and V.differing(want, unflagged) == []
    assert V.differing(before, reference("cornell")) == [] and V.differing(got, before) != []


# ---- the fold, and the ray call on its own persistent route
@pytest.mark.parametrize("name", NAMES)
def test_the_fold_of_the_flagged_channels_is_rgb_is_flagged_trace_rays(name):
    _, o, d, ids, bounces, seed = RP.rays(name)
    g = RP.gpu(name)
    v = flagged(g, name, exposure_value=1.5)
    _, acc = V.fold(v)
    assert (acc / SAMPLES * 2.0 ** 1.5 == v.rgb).all(), "%d rays differ" % (acc / SAMPLES * 2.0 ** 1.5 != v.rgb).any(axis=1).sum()
    g.reset_stats()
    rgb = g.trace_rays(o, d, bounces, samples=SAMPLES, seed=seed, sample_index_base=BASE, streams=ids, first_draw=2,
                       exposure_value=1.5, flags=_abi.RPT_FLAG_RAYS_PERSISTENT)
    RP.on_route(g, N, SAMPLES)
    assert V.same(v.rgb, rgb)


# ---- the oracle anchor
def test_cornell_against_the_oracle(oracle):
    """every flagged vertex against shading_matrix.oracle_path on the oracle's own camera rays of sample 5; one sample: the
    oracle's frame"""
    scene, camera, p, o, d, streams, draws, frame = RP.case("cornell", BASE)
    g = RP.gpu("cornell")
    kw = dict(streams=streams, seed=p.seed, sample_index_base=BASE, first_draw=2, flags=FLAG)
    g.reset_stats()
    v = g.trace_vertices(o, d, p.max_bounces, samples=SAMPLES, **kw)
    RP.on_route(g, len(o), SAMPLES)
    VO.assert_oracle_path(v, M.oracle_vertices(oracle.OracleScene(scene), scene, o, d, streams, SAMPLES, BASE, 2, p.seed, p.max_bounces))
    g.reset_stats()
    one = g.trace_vertices(o, d, p.max_bounces, samples=1, channels=_abi.RPT_VERTEX_RGB | _abi.RPT_VERTEX_LENGTH, **kw)
    RP.on_route(g, len(o), 1)
    assert (one.rgb == frame).all() and (one.length == v.length[:, :1]).all()


class _Flagged:
    """a handle whose trace_vertices carries the flag (and holds every call to the route): for
    test_gpu_vertices_oracle.matrix_on_device"""

    def __init__(self, g):
        self.g = g

    def trace_vertices(self, o, d, bounces, **kw):
        self.g.reset_stats()
        v = self.g.trace_vertices(o, d, bounces, flags=FLAG, **kw)
        RP.on_route(self.g, len(o), kw.get("samples", 1))
        return v


def test_the_material_matrix_against_the_oracle(oracle):
    """the lit scene of the material matrix, seen from outside: trace_sample's records and oracle_path's vertices"""
    lit, inside = True, False
    scene, of, osc, cam, p, rec, length = H.matrix_case(lit, inside)
    v = VO.matrix_on_device(_Flagged(VO.matrix_gpu(lit)), lit, inside)
    VO.assert_records(v, rec, length)
    VO.assert_oracle_path(v, H.matrix_vertices(lit, inside))
