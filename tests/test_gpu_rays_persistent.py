"""RPT_FLAG_RAYS_PERSISTENT on the GPU (include/rpt_gpu_rays_persistent.h): the caller's rays and
light probes in the persistent path kernel, rpt_paths_rays.  Tolerance 0 (== on the f64 arrays) everywhere: the flagged call
gives the bits of the unflagged call of the same arguments — the wavefront pipeline's —, and on the oracle's own camera rays
the oracle's frame.

The scenes, and the instantiation each reaches (the names RPTGPU_PRINT_LAUNCH prints as `rpt_paths_rays<...>`):
  cornell     rpt_paths_rays<KdFlat>, the fused form with a hit's scene constants and the wave-level pool (POOL)
  glass       rpt_paths_rays<KdFlatG> + parked environment lookups (the plain fetch, PARK)
  wine_glass  rpt_paths_rays<KdLds> (deep trees: the general form)
  KdFlatG     tests/test_gpu_parity.py's three spheres under a colour environment
  KdFlatF     its polygon room behind the object filter
  monomial    the extended shape set: kernels_rays_strict_ext (KdFlatG, parked)
  ambient     the Cornell box with a second, ambient light: no fused query, so rpt_paths_rays<KdFlat, false> — the per-lane
              STASH with pre-traced rays (RayStashHit: stash_put_path / stash_take_hit / stash_take_path)
  cube_hdri   test_gpu_parity.py's glass cube on a polygon under an HDRI, its handle made under RPTGPU_NO_PLANE_TABLE:
              rpt_paths_rays<KdFlat, true> — the per-lane STASH without the pre-trace (RayStash), parked lookups.  (The
              parked queues leave a triangle scene 2 560 B of the wave's LDS for its tables; with the plane table even one
              polygon needs 3 200 B and takes the fused or the unparked form, so only the A/B switch reaches this one.)
So the hand-out forms are reached by: POOL cornell; STASH ambient and cube_hdri; the plain fetch all the others
(test_the_instantiation_each_scene_reaches holds the scenes to these launch lines).
Shapes: the 777 camera rays of a 37x21 frame (twelve waves and nine lanes), 65, 5 and 1 rays, 16 probes x 33 samples."""
import functools
import os

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, Light, Material, Object, _abi, cube, hex_color, make_params, scenes

import small_scenes
import test_gpu_parity as GP
import test_gpu_probes as PR
import test_gpu_trace_rays as TR

pytestmark = pytest.mark.gpu

FLAG = getattr(_abi, "RPT_FLAG_RAYS_PERSISTENT", 32)
SMALL = ("cornell", "glass", "wine_glass")
STASH = ("ambient", "cube_hdri")  # the scenes of the per-lane stash forms
NAMES = SMALL + ("KdFlatG", "KdFlatF", "monomial") + STASH
W, H = 37, 21
SPP = 4
WAVEFRONT_KINDS = (_abi.RPT_K_RAYGEN, _abi.RPT_K_EXTEND, _abi.RPT_K_SHADE, _abi.RPT_K_SHADOW, _abi.RPT_K_RESOLVE)
N_PROBES, PROBE_SAMPLES = PR.N_PROBES, 33
# where the probes of the scenes without a box in test_gpu_probes stand (between, and now and then inside, the objects)
BOXES = {"KdFlatG": ((-2.0, -0.8, -2.0), (2.0, 1.0, 1.0)), "KdFlatF": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),
         "monomial": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "ambient": PR.BOXES["cornell"],
         "cube_hdri": ((-2.0, 0.05, -2.0), (2.0, 2.0, 2.0))}


@functools.lru_cache(maxsize=None)
def case(name, s):
    """test_gpu_trace_rays.case at 37x21 for every scene (its glass is 33x23): (scene, camera, params of ONE sample at index
    s, the oracle's rays, their streams and draw counts, the oracle's frame) — computed once, shared, never written to"""
    if TR.SIZES[name] == (W, H):
        return TR.case(name, s)
    from oracle import oracle_ffi as oracle
    scene, camera, p0 = small_scenes.small(name)
    camera = TR.pinhole(camera)
    p = make_params(W, H, p0.max_bounces, 1, seed=p0.seed, sample_index_base=s)
    o, d, streams, draws = TR.camera_rays(oracle, camera, p, s)
    want = oracle.OracleScene(scene).render(camera, p)
    for a in (o, d, streams, draws, want):
        a.setflags(write=False)
    return scene, camera, p, o, d, streams, draws, want


@functools.lru_cache(maxsize=None)
def rays(name):
    """-> (scene, origins, dirs, stream ids, max_bounces, seed): the oracle's camera rays of a 37x21 frame of the scene's
    pinhole camera at sample 0, the pixel as stream id — shared, read-only"""
    if name in SMALL:
        scene, camera, p, o, d, streams, draws, want = case(name, 0)
        return scene, o, d, streams, p.max_bounces, p.seed
    from oracle import oracle_ffi as oracle
    if name == "monomial":
        scene, camera, p0 = small_scenes.small("monomial")
        bounces, seed = p0.max_bounces, p0.seed
    elif name == "ambient":
        scene, camera, p0 = small_scenes.small("cornell")
        scene.add(Light.Ambient((0.02, 0.03, 0.04)))
        bounces, seed = p0.max_bounces, p0.seed
    elif name == "cube_hdri":
        scene, camera, p0 = GP._hdri_scene("cube")
        bounces, seed = p0.max_bounces, p0.seed
    else:
        scene, camera = GP._thin_lens_scene(name)
        bounces, seed = 3, 131
    o, d, streams, draws = TR.camera_rays(oracle, TR.pinhole(camera), make_params(W, H, bounces, 1, seed=seed), 0)
    for a in (o, d, streams):
        a.setflags(write=False)
    return scene, o, d, streams, bounces, seed


def make_gpu(name, **options):
    """a handle of the scene; cube_hdri's without the plane table (read when the handle is made), see the top of this file"""
    if name != "cube_hdri":
        return GpuScene(rays(name)[0], 0, **options)
    os.environ["RPTGPU_NO_PLANE_TABLE"] = "1"
    try:
        return GpuScene(rays(name)[0], 0, **options)
    finally:
        del os.environ["RPTGPU_NO_PLANE_TABLE"]


@functools.lru_cache(maxsize=None)
def gpu(name):
    return TR.gpu(name) if name in SMALL else make_gpu(name)


def trace(g, name, sel=slice(None), streams="ids", **kw):
    _, o, d, ids, bounces, seed = rays(name)
    kw.setdefault("samples", SPP)
    kw.setdefault("seed", seed)
    kw.setdefault("first_draw", 2)
    kw.setdefault("exposure_value", 1.5)
    return g.trace_rays(o[sel], d[sel], kw.pop("max_bounces", bounces), streams=ids[sel] if isinstance(streams, str) else streams, **kw)


def on_route(g, n, iterations, min_launches=1):
    """RptStats as for a render through rpt_paths: the samples, the kernel's launches and rays — and no wavefront launch"""
    st = g.stats()
    assert st.kernel_launches[_abi.RPT_K_PATHS] >= min_launches, "the persistent kernel did not run"
    assert [st.kernel_launches[k] for k in WAVEFRONT_KINDS] == [0] * len(WAVEFRONT_KINDS)
    assert st.samples == n * iterations
    assert st.extend_rays >= st.samples


def flagged(g, name, sel=slice(None), min_launches=1, **kw):
    g.reset_stats()
    out = trace(g, name, sel, flags=FLAG | kw.pop("flags", 0), **kw)
    on_route(g, len(out), kw.get("samples", SPP), min_launches)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, first_draw=2):
    """the unflagged call over all rays, 4 samples — computed once, never written to"""
    out = trace(gpu(name), name, first_draw=first_draw)
    assert np.isfinite(out).all() and (out != 0).any()
    out.setflags(write=False)
    return out


def test_the_library_reads_the_flag():
    assert _abi.rays_persistent_supported()


# (name -> the instantiation's name, what its launch line says, what it does not say)
LAUNCH_LINES = {
    "cornell": ("KdFlat", ("shadow and bounce rays in one query", "scene constants", "wave-level pool"), ("parked",)),
    "glass": ("KdFlatG", ("parked environment lookups",), ()),
    "wine_glass": ("KdLds", (), ("parked",)),
    "KdFlatG": ("KdFlatG", (), ("parked",)),
    "KdFlatF": ("KdFlatF", (), ("parked",)),
    "monomial": ("KdFlatG", ("parked environment lookups",), ()),
    "ambient": ("KdFlat", (), ("one query", "wave-level pool", "parked")),
    "cube_hdri": ("KdFlat", ("parked environment lookups",), ("one query", "wave-level pool")),
}


@pytest.mark.parametrize("name", NAMES)
def test_the_instantiation_each_scene_reaches(name, monkeypatch, capfd):
    """the launch diagnostics name the kernel and the form: among them the two per-lane STASH forms, rpt_paths_rays<KdFlat,
    false> without the fused query (ambient) and rpt_paths_rays<KdFlat, true> (cube_hdri), and the POOL form (cornell)"""
    kernel, says, says_not = LAUNCH_LINES[name]
    g = gpu(name)
    reference(name), probes_reference(name, "sh9")
    monkeypatch.setenv("RPTGPU_PRINT_LAUNCH", "1")
    capfd.readouterr()
    got = flagged(g, name)
    got_p = flagged_bake(g, name, PR.SH9)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths")]
    monkeypatch.delenv("RPTGPU_PRINT_LAUNCH")
    kernels = [ln for ln in lines if "blocks/CU" in ln]
    assert len(kernels) == 2 and all(ln.startswith("rpt_paths_rays<%s>:" % kernel) for ln in kernels), lines
    for ln in kernels:
        assert all(w in ln for w in says) and not any(w in ln for w in says_not), ln
    assert (got == reference(name)).all() and (got_p == probes_reference(name, "sh9")).all()


# ---- the oracle anchor
@pytest.mark.parametrize("s", [0, 5])
@pytest.mark.parametrize("name", SMALL)
def test_the_oracles_frame_from_the_oracles_rays(name, s):
    scene, camera, p, o, d, streams, draws, want = case(name, s)
    assert len(o) == 777 and (draws == 2).all()
    g = gpu(name)
    g.reset_stats()
    got = TR.trace(g, p, o, d, streams=streams, flags=FLAG)
    on_route(g, 777, 1)
    assert got.shape == want.shape and got.dtype == np.float64
    assert (got == want).all(), "%d of %d rays differ" % ((got != want).any(axis=1).sum(), len(want))


def test_the_oracles_frame_under_a_lens(oracle):
    """cornell under a lens: the rays' streams stop at different draws; one flagged call per draw count (4, 6, 8, ...)"""
    scene, camera0, p0 = small_scenes.small("cornell")
    camera = TR.pinhole(camera0).focus((278.0, 273.0, 280.0), 20.0)
    p = make_params(W, H, p0.max_bounces, 1, seed=p0.seed, sample_index_base=3)
    o, d, streams, draws = TR.camera_rays(oracle, camera, p, 3)
    want = oracle.OracleScene(scene).render(camera, p)
    counts = sorted(set(draws.tolist()))
    assert counts[0] == 4 and len(counts) >= 2
    got = np.full_like(want, np.nan)
    g = gpu("cornell")
    for c in counts:
        m = draws == c
        g.reset_stats()
        got[m] = TR.trace(g, p, o[m], d[m], streams=streams[m], first_draw=c, flags=FLAG)
        on_route(g, int(m.sum()), 1)
    assert (got == want).all()


# ---- flagged == unflagged: rays
@pytest.mark.parametrize("first_draw", [0, 2, 5])
@pytest.mark.parametrize("name", NAMES)
def test_flagged_is_unflagged(name, first_draw):
    """4 samples, an exposure; a stream that starts at draw 0, 2 and 5 (odd: the cached half of a Philox block is what
    pool_take — cornell — and stash_take_path — ambient, cube_hdri — have to bring back)"""
    want = reference(name, first_draw)
    got = flagged(gpu(name), name, first_draw=first_draw)
    assert got.shape == (777, 3) and got.dtype == np.float64
    assert (got == want).all(), "%d of 777 rays differ" % (got != want).any(axis=1).sum()
    if first_draw != 2:
        assert not (want == reference(name, 2)).all()


@pytest.mark.parametrize("n", [1, 5, 65])
@pytest.mark.parametrize("name", ["cornell", "glass", "KdFlatF"] + list(STASH))
def test_less_than_a_wave_and_a_wave_and_a_lane(name, n):
    sel = slice(300, 300 + n)
    assert (flagged(gpu(name), name, sel) == reference(name)[sel]).all()


@pytest.mark.parametrize("name", NAMES)
def test_a_rays_result_is_its_own(name, monkeypatch):
    """streams given, permuted and NULL; a call split in two; pieces of 100 (rpt_rays_ids names the streams of a piece)"""
    g = gpu(name)
    want = reference(name)
    n = len(want)
    perm = np.random.RandomState(77).permutation(n)
    assert (flagged(g, name, perm) == want[perm]).all()
    assert (flagged(g, name, streams=None) == want).all()  # the oracle's streams are the indices
    k = 333
    assert (flagged(g, name, slice(0, k)) == want[:k]).all()
    assert (flagged(g, name, slice(k, n)) == want[k:]).all()
    monkeypatch.setenv("RPTGPU_RAYS_PIECE", "100")
    pieces = (n + 99) // 100
    assert (flagged(g, name, min_launches=pieces) == want).all()
    assert (flagged(g, name, streams=None, min_launches=pieces) == want).all()  # ray i of piece k has stream 100 k + i
    assert (flagged(g, name, perm, min_launches=pieces) == want[perm]).all()
    assert (trace(g, name, streams=None) == want).all()  # (the unflagged call in the same pieces)


@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass", "KdFlatF"] + list(STASH))
def test_work_items_of_one_and_two_samples(name, chunk):
    g = make_gpu(name, paths_chunk=chunk)
    try:
        got = [flagged(g, name, first_draw=fd) for fd in (0, 2, 5)]
    finally:
        g.close()
    assert all((got[i] == reference(name, fd)).all() for i, fd in enumerate((0, 2, 5)))


@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"] + list(STASH))
def test_three_launches_per_piece(name, monkeypatch):
    """5 samples and a per-sample radiance buffer with room for TWO samples of a piece: three launches of 2, 2 and 1 samples,
    fr.sample_base stepping by 2 — over the whole call and over pieces of 100 (the last one, 77 rays, takes three as well)"""
    want = trace(gpu(name), name, samples=5)
    g = make_gpu(name, lbuf_bytes=777 * 24 * 2)
    g2 = make_gpu(name, lbuf_bytes=100 * 24 * 2)
    try:
        whole = flagged(g, name, samples=5, min_launches=3)
        assert g.stats().kernel_launches[_abi.RPT_K_PATHS] == 3
        monkeypatch.setenv("RPTGPU_RAYS_PIECE", "100")
        cut = flagged(g2, name, samples=5, min_launches=3 * 8)
        assert g2.stats().kernel_launches[_abi.RPT_K_PATHS] == 3 * 8
    finally:
        g.close()
        g2.close()
    assert (whole == want).all() and (cut == want).all() and not (want == reference(name)).all()


@pytest.mark.parametrize("name", ["cornell", "glass", "monomial"])
def test_sample_base_across_the_32_bit_boundary(name):
    g = gpu(name)
    want = trace(g, name, sample_index_base=2 ** 32 - 2)
    assert (flagged(g, name, sample_index_base=2 ** 32 - 2) == want).all()
    assert not (want == reference(name)).all()


@pytest.mark.parametrize("name", ["cornell", "glass", "KdFlatF"])
def test_no_bounces(name):
    g = gpu(name)
    want = trace(g, name, max_bounces=0)
    assert (flagged(g, name, max_bounces=0) == want).all() and not (want == reference(name)).all()


@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"])
def test_general_traversal_and_profiling(name):
    g = gpu(name)
    assert (flagged(g, name, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL) == reference(name)).all()
    assert (flagged(g, name, flags=_abi.RPT_FLAG_PROFILE_KERNELS) == reference(name)).all()


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_device_entry_point_on_torch_tensors(name):
    _, o, d, ids, bounces, seed = rays(name)
    g = gpu(name)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    ts = torch.from_numpy(ids.astype(np.int32)).to(dev)
    keep = to.clone(), td.clone(), ts.clone()
    kw = dict(samples=SPP, seed=seed, first_draw=2, exposure_value=1.5, flags=FLAG)
    g.reset_stats()
    got = g.trace_rays(to, td, bounces, streams=ts, **kw)
    on_route(g, 777, SPP)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.dtype == torch.float64
    assert (got.cpu().numpy() == reference(name)).all()
    out = torch.full((777, 3), -1.0, dtype=torch.float64, device=dev)
    g.reset_stats()
    assert g.trace_rays(to, td, bounces, out=out, **kw) is out  # no ids: the indices
    on_route(g, 777, SPP)
    assert (out.cpu().numpy() == reference(name)).all()
    assert torch.equal(to, keep[0]) and torch.equal(td, keep[1]) and torch.equal(ts, keep[2])


# ---- flagged == unflagged: probes
@functools.lru_cache(maxsize=None)
def probes(name):
    if name in PR.BOXES:
        return PR.probes(name)
    rs = np.random.RandomState(sum(map(ord, name)))
    lo, hi = BOXES[name]
    pos = rs.uniform(lo, hi, (N_PROBES, 3))
    nrm = rs.standard_normal((N_PROBES, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ids = rs.permutation(1000)[:N_PROBES].astype(np.uint32) + 5
    for a in (pos, nrm, ids):
        a.setflags(write=False)
    return pos, nrm, ids


def bake(g, name, kind, streams="ids", **kw):
    pos, nrm, ids = probes(name)
    kw.setdefault("seed", rays(name)[5])
    kw.setdefault("max_bounces", rays(name)[4])
    kw.setdefault("samples", PROBE_SAMPLES)
    return g.bake_probes(pos, nrm if kind == PR.IRR else None, kind=kind, streams=ids if isinstance(streams, str) else streams, **kw)


def flagged_bake(g, name, kind, min_launches=1, **kw):
    g.reset_stats()
    out = bake(g, name, kind, flags=FLAG | kw.pop("flags", 0), **kw)
    on_route(g, N_PROBES, kw.get("samples", PROBE_SAMPLES), min_launches)
    return out


@functools.lru_cache(maxsize=None)
def probes_reference(name, kind_name, with_ids=True):
    out = bake(gpu(name), name, PR.KINDS[kind_name], **({} if with_ids else dict(streams=None)))
    assert np.isfinite(out).all() and (out != 0).any()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("kind_name", ["sh9", "irradiance"])
@pytest.mark.parametrize("name", NAMES)
def test_flagged_probes_are_unflagged_probes(name, kind_name, monkeypatch):
    """16 probes x 33 samples (528 paths), both kinds; with stream ids and without; in pieces of 3 probes"""
    kind = PR.KINDS[kind_name]
    g = gpu(name)
    want = probes_reference(name, kind_name)
    got = flagged_bake(g, name, kind)
    assert got.shape == ((N_PROBES, 9, 3) if kind == PR.SH9 else (N_PROBES, 3)) and got.dtype == np.float64
    assert (got == want).all(), "%d of %d probes differ" % ((got != want).reshape(N_PROBES, -1).any(axis=1).sum(), N_PROBES)
    no_ids = probes_reference(name, kind_name, False)
    assert (flagged_bake(g, name, kind, streams=None) == no_ids).all() and not (no_ids == want).all()
    monkeypatch.setenv("RPTGPU_PROBES_PIECE", "3")
    assert (flagged_bake(g, name, kind, min_launches=6) == want).all()
    assert (flagged_bake(g, name, kind, streams=None, min_launches=6) == no_ids).all()  # probe i of piece k has stream 3 k + i


@pytest.mark.parametrize("kind_name", ["sh9", "irradiance"])
@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("name", ["cornell", "glass", "wine_glass"] + list(STASH))
def test_probes_over_launch_borders(name, chunk, kind_name, monkeypatch):
    """pieces of 3 probes and a per-sample radiance buffer of 8 samples of such a piece: five launches of 7, 7, 7, 7 and 5
    samples per piece (two of 17 and 16 for the last piece, one probe), so launch borders fall inside every probe's samples —
    where the wavefront's pass borders do not —, in work items of 1 and 2 samples"""
    kind = PR.KINDS[kind_name]
    monkeypatch.setenv("RPTGPU_PROBES_PIECE", "3")
    g = make_gpu(name, paths_chunk=chunk, lbuf_bytes=3 * 24 * 8)
    try:
        got = flagged_bake(g, name, kind, min_launches=5 * 5 + 2)
    finally:
        g.close()
    assert (got == probes_reference(name, kind_name)).all()


class _Flagged:
    """a handle whose trace_rays carries the flag (and holds every call to the route): for test_gpu_probes.restated"""

    def __init__(self, g):
        self.g = g

    def trace_rays(self, o, d, bounces, **kw):
        self.g.reset_stats()
        out = self.g.trace_rays(o, d, bounces, flags=FLAG, **kw)
        on_route(self.g, len(o), kw.get("samples", 1))
        return out


@pytest.mark.parametrize("name,kind_name", [("cornell", "sh9"), ("cornell", "irradiance"), ("glass", "sh9"), ("wine_glass", "irradiance")])
def test_probes_from_the_flagged_ray_call(name, kind_name):
    """test_gpu_probes' restatement on this route: the same directions through flagged trace_rays, one call per (sample, draw
    count), folded in numpy in the header's order"""
    kind = PR.KINDS[kind_name]
    pos, nrm, ids = probes(name)
    g = gpu(name)
    want, _, draws = PR.restated(_Flagged(g), kind, pos, nrm, ids, rays(name)[4], rays(name)[5], PROBE_SAMPLES)
    assert len(set(draws.ravel().tolist())) >= 2  # the paths do not all start at one draw
    assert (flagged_bake(g, name, kind) == want).all()
    assert (probes_reference(name, kind_name) == want).all()


@pytest.mark.parametrize("kind_name", ["sh9", "irradiance"])
def test_probes_device_entry_point(kind_name):
    kind = PR.KINDS[kind_name]
    pos, nrm, ids = probes("cornell")
    g = gpu("cornell")
    dev = torch.device("cuda", 0)
    tp, tn = torch.from_numpy(pos.copy()).to(dev), torch.from_numpy(nrm.copy()).to(dev)
    ti = torch.from_numpy(ids.astype(np.int32)).to(dev)
    keep = tp.clone(), tn.clone(), ti.clone()
    g.reset_stats()
    got = g.bake_probes(tp, tn if kind == PR.IRR else None, kind=kind, samples=PROBE_SAMPLES, max_bounces=rays("cornell")[4],
                        seed=rays("cornell")[5], sample_index_base=2 ** 32 - 20, streams=ti, flags=FLAG)
    on_route(g, N_PROBES, PROBE_SAMPLES)
    want = bake(g, "cornell", kind, sample_index_base=2 ** 32 - 20)
    assert isinstance(got, torch.Tensor) and (got.cpu().numpy() == want).all()
    assert not (want == probes_reference("cornell", kind_name)).all()
    assert torch.equal(tp, keep[0]) and torch.equal(tn, keep[1]) and torch.equal(ti, keep[2])


# ---- a scene the persistent kernel cannot walk
def test_a_group_with_tree_children_runs_the_wavefront_route(oracle):
    scene, camera, p0 = small_scenes.small("fractal_teapots")
    p = make_params(21, 13, p0.max_bounces, 1, seed=p0.seed)
    o, d, streams, _ = TR.camera_rays(oracle, TR.pinhole(camera), p, 0)
    pos = o[:N_PROBES] + 0.5 * d[:N_PROBES]
    g = GpuScene(scene, 0)
    try:
        kw = dict(samples=2, seed=p.seed, streams=streams, first_draw=2)
        want = g.trace_rays(o, d, p.max_bounces, **kw)
        g.reset_stats()
        got = g.trace_rays(o, d, p.max_bounces, flags=FLAG, **kw)
        st = g.stats()
        assert st.kernel_launches[_abi.RPT_K_PATHS] == 0 and st.kernel_launches[_abi.RPT_K_RAYGEN] >= 1 and st.samples == 2 * len(o)
        pk = dict(kind=PR.SH9, samples=5, max_bounces=p.max_bounces, seed=p.seed)
        want_p = g.bake_probes(pos, **pk)
        g.reset_stats()
        got_p = g.bake_probes(pos, flags=FLAG, **pk)
        st = g.stats()
        assert st.kernel_launches[_abi.RPT_K_PATHS] == 0 and st.kernel_launches[_abi.RPT_K_RAYGEN] >= 1
    finally:
        g.close()
    assert (got == want).all() and (want != 0).any()
    assert (got_p == want_p).all() and (want_p != 0).any()


# ---- after a live update
def test_after_a_live_update():
    """set_objects on the Cornell box: flagged rays and flagged probes on the updated handle == a fresh handle's"""
    def moved():
        scene, _, _ = scenes.cornell()
        scene.objects[6] = Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(0.4).translate((300.0, 120.0, 140.0))) \
            .material(Material.diffuse(hex_color(0x3366CC)))
        return scene
    g = GpuScene(scenes.cornell()[0], 0)
    fresh = GpuScene(moved(), 0)
    try:
        before = flagged(g, "cornell")
        before_p = flagged_bake(g, "cornell", PR.SH9)
        g.set_objects([6], [moved().objects[6]])
        got, got_p = flagged(g, "cornell"), flagged_bake(g, "cornell", PR.SH9)
        want, want_p = flagged(fresh, "cornell"), flagged_bake(fresh, "cornell", PR.SH9)
        unflagged, unflagged_p = trace(fresh, "cornell"), bake(fresh, "cornell", PR.SH9)
    finally:
        g.close()
        fresh.close()
    assert (got == want).all() and (got_p == want_p).all()
    assert (want == unflagged).all() and (want_p == unflagged_p).all()
    assert (before == reference("cornell")).all() and (before_p == probes_reference("cornell", "sh9")).all()
    assert not (got == before).all() and not (got_p == before_p).all()
