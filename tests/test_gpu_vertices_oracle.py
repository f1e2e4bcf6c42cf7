"""rptgpu_trace_vertices' shading channels held to the ORACLE, vertex by vertex.

tests/test_gpu_vertices.py restates every channel through other device calls, and every other oracle comparison of the
suite is a frame.  Neither sees a bsdf, a pdf, a sampled direction or a draw counter under a suffix that is exactly zero
— a path whose next vertex escapes into a black environment or dead-ends unlit multiplies them by 0 —, a third of
cornell's inner vertices and most of the dark matrix scene's (tests/shading_matrix.py, counted in
tests/test_shading_matrix_host.py).  Here:
  1. records   LENGTH, RADIANCE, BSDF, INV_PDF, ABS_COS (and OBJECT, NORMAL, POSITION, DIRECTION, DRAW) of every vertex of
               every (ray, sample) are oracle_trace_sample's records where the ray is the sample's own camera ray, and
               shading_matrix.oracle_path's — pinned to those records without a GPU — everywhere.
  2. the chain the DEVICE's exported NORMAL, POSITION, DIRECTION, OBJECT and DRAW of a vertex go through oracle_illuminate,
               oracle_sample_f and oracle_bsdf: the sampled direction is the next vertex's DIRECTION, 1/pdf is INV_PDF, the
               draw it ends at is the next DRAW, bsdf is BSDF; a path that ended by itself ended on a None.  A difference
               names the function and the material, wherever the path has gone.
  3. rays no camera makes: long and short directions, origins inside transparent cubes, rays 1e-6 rad off a face, scattered
               streams, and a sample index base of 2^32 - 1.
  4. frames of the matrix from the kernels that export no vertices: persistent (with the wave's tables of scene
               constants, where a scene can have them), wavefront, default; and frame, records and chain on the per-tree
               route, on a variant of the matrix with real trees (the tree-trace kernel must have launched).
Raw bits everywhere; a NaN equals any NaN (x86 and gfx950 make different quiet NaNs).  No vertex is skipped."""
import functools
import os

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

from rpt_amd import GpuScene, _abi, make_params
from rpt_amd.device import PathVertices

import shading_matrix as M
import test_gpu_trace_rays as R
import test_gpu_vertices as V
import test_shading_matrix_host as H

pytestmark = pytest.mark.gpu

SHADING = ("radiance", "bsdf", "inv_pdf", "abs_cos")
PER_TREE = {"RPTGPU_DEEP_DEPTH": "1", "RPTGPU_SORT_RAYS": "1", "RPTGPU_SORT_MIN_RAYS": "0"}  # test_axis_parallel_rays_...'s per_tree
TABLES = "a hit's scene constants from the wave's tables"
FUSED = "shadow and bounce rays in one query"


def differing(got, want, channels):
    """per channel, how many entries differ in their bits (a NaN equal to any NaN)"""
    out = {}
    for k in channels:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if g.dtype == np.float64:
            bad = (g.view(np.uint64) != w.view(np.uint64)) & ~(np.isnan(g) & np.isnan(w))
        else:
            bad = g != w
        if bad.any():
            out[k] = int(bad.sum())
    return out


def census(v):
    """(vertices, inner vertices, those under an all-zero suffix, those with a non-finite factor) of a result"""
    L, _ = V.fold(v)
    n, S, B1 = v.length.shape + (v.t.shape[2],)
    depth = np.arange(B1)[None, None, :]
    inner = depth < v.length[:, :, None].astype(np.int64) - 1
    zero = np.zeros_like(inner)
    zero[:, :, :-1] = (L[:, :, 1:] == 0.0).all(axis=3)
    nonfinite = ~(np.isfinite(v.bsdf).all(axis=3) & np.isfinite(v.inv_pdf) & np.isfinite(v.abs_cos))
    return int(v.length.sum()), int(inner.sum()), int((inner & zero).sum()), int((inner & nonfinite).sum())


def samples_of(results, pick):
    """a PathVertices of the per-path and per-vertex channels pick(name) makes of `results` (no RGB: that one is per ray)"""
    v = PathVertices(results[0].channels & ~_abi.RPT_VERTEX_RGB)
    for k in results[0].arrays():
        if k != "rgb":
            setattr(v, k, np.ascontiguousarray(pick(k)))
            getattr(v, k).setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def matrix_gpu(lit, part=None):
    return GpuScene(M.scene(lit, part)[0], 0)


def matrix_on_device(g, lit, inside, meshed=False):
    """the frame's paths on the device: one call per sample, on that sample's camera rays of the oracle"""
    from oracle import oracle_ffi
    scene, of, osc, cam, p, rec, length = H.matrix_case(lit, inside, meshed)
    out = []
    for s in range(p.iterations):
        o, d, streams, draws = R.camera_rays(oracle_ffi, cam, M.params(s, 1), s)
        out.append(g.trace_vertices(o, d, p.max_bounces, streams=streams, samples=1, seed=p.seed, sample_index_base=s, first_draw=2))
    return samples_of(out, lambda k: np.concatenate([getattr(x, k) for x in out], axis=1))


@functools.lru_cache(maxsize=None)
def matrix_device(lit, inside):
    return matrix_on_device(matrix_gpu(lit), lit, inside)


def assert_records(v, rec, length):
    """v's shading channels against trace_sample's records of the same (ray, sample)s, pixel-major then sample"""
    n, S, B1 = v.t.shape
    assert (v.length.reshape(-1) == length).all(), "%d of %d lengths differ" % ((v.length.reshape(-1) != length).sum(), len(length))
    rec = rec.reshape(n, S, B1, 8)
    want = {"radiance": rec[..., 0:3], "bsdf": rec[..., 3:6], "inv_pdf": rec[..., 6], "abs_cos": rec[..., 7]}
    assert differing(v.arrays(), want, SHADING) == {}
    last = np.arange(B1)[None, None, :] == v.length[:, :, None].astype(np.int64) - 1
    for k in ("bsdf", "inv_pdf", "abs_cos"):  # +0.0 at a path's last vertex, on both sides
        assert not V.bits(getattr(v, k)[last]).any() and not V.bits(np.ascontiguousarray(want[k])[last]).any(), k


def assert_oracle_path(v, want):
    got = v.arrays()
    assert differing(got, want, ("length", "object", "direction", "draw", "position") + SHADING) == {}
    hit = want["object"] >= 0
    assert differing({"normal": got["normal"][hit]}, {"normal": want["normal"][hit]}, ("normal",)) == {}


# ---- 1. records
@pytest.mark.parametrize("name", V.NAMES)
def test_records_of_the_small_scenes(oracle, name):
    """test_gpu_vertices' rays and samples: sample 5 runs along its own camera rays and is trace_sample's record; samples
    6 and 7 run along the same rays and are oracle_path's, as all three are"""
    scene, camera, p, o, d, streams, draws, frame = R.case(name, V.BASE)
    v = V.base(name)
    osc = oracle.OracleScene(scene)
    rec, length = M.records(osc, camera, p)
    assert_records(samples_of([v], lambda k: getattr(v, k)[:, :1]), rec, length)
    assert_oracle_path(v, M.oracle_vertices(osc, scene, o, d, streams, V.SAMPLES, V.BASE, 2, p.seed, p.max_bounces))
    print("%s: %d vertices, %d inner, %d under a zero suffix, %d with a non-finite factor" % ((name,) + census(v)))


@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "dark"])
def test_records_of_the_matrix(oracle, lit, inside):
    scene, of, osc, cam, p, rec, length = H.matrix_case(lit, inside)
    v = matrix_device(lit, inside)
    assert_records(v, rec, length)
    assert_oracle_path(v, H.matrix_vertices(lit, inside))
    print("matrix %s %s: %d vertices, %d inner, %d under a zero suffix, %d with a non-finite factor"
          % (("lit" if lit else "dark", "inside" if inside else "outside") + census(v)))


# ---- 2. the chain, per function
def chain_check(v, scene, names, streams, seed, bases, B):
    """every vertex of v (numpy PathVertices; path [i, s] on stream streams[i] at sample bases[s]) through the oracle's
    functions -> (vertices checked, {(what differs, material): count})"""
    ch = M.chain(scene)
    wrong = {}
    done = 0

    def note(what, obj):
        name = names[obj] if obj < len(names) else "object %d" % obj
        wrong[(what, name)] = wrong.get((what, name), 0) + 1

    def same(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())

    n, S, B1 = v.t.shape
    for i in range(n):
        for s in range(S):
            length = int(v.length[i, s])
            for d in range(length):
                obj = int(v.object[i, s, d])
                if obj < 0:
                    assert d == length - 1
                    continue
                if d == B:
                    continue  # (a path's vertex at its last depth samples no direction)
                some, wi, inv_pdf, f, abs_cos, after, _ = ch.step(obj, v.normal[i, s, d], v.position[i, s, d], v.direction[i, s, d], seed,
                                                                  int(streams[i]), int(bases[s]), int(v.draw[i, s, d]))
                done += 1
                if d == length - 1:  # ended by itself before depth B
                    if some:
                        note("sample_f is Some where the path ended", obj)
                    continue
                if not some:
                    note("sample_f is None where the path went on", obj)
                    continue
                if not same(wi, v.direction[i, s, d + 1]):
                    note("sample_f's wi", obj)
                if not same(inv_pdf, v.inv_pdf[i, s, d]):
                    note("sample_f's pdf", obj)
                if after != int(v.draw[i, s, d + 1]):
                    note("the draw sample_f ends at", obj)
                if not same(f, v.bsdf[i, s, d]):
                    note("bsdf", obj)
                if not same(abs_cos, v.abs_cos[i, s, d]):
                    note("|wi.n|", obj)
    return done, wrong


def matrix_names(of):
    return ["floor", "wall"] + [M.MATERIALS[i][0] for i in of[M.FIRST_OBJECT:]]


@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "dark"])
def test_the_chain_on_the_matrix(oracle, lit, inside):
    scene, of, osc, cam, p, rec, length = H.matrix_case(lit, inside)
    v = matrix_device(lit, inside)
    streams = np.arange(p.width * p.height, dtype=np.uint32)
    done, wrong = chain_check(v, scene, matrix_names(of), streams, p.seed, list(range(p.iterations)), p.max_bounces)
    print("matrix %s %s: %d vertices through the oracle's functions" % ("lit" if lit else "dark", "inside" if inside else "outside", done))
    assert wrong == {}


def test_the_chain_on_cornell(oracle):
    scene, camera, p, o, d, streams, draws, frame = R.case("cornell", V.BASE)
    v = V.base("cornell")
    names = ["object %d" % i for i in range(len(scene.objects))]
    done, wrong = chain_check(v, scene, names, streams, p.seed, [V.BASE + s for s in range(V.SAMPLES)], p.max_bounces)
    print("cornell: %d vertices through the oracle's functions" % done)
    assert wrong == {}


# ---- 3. rays no camera makes
@pytest.mark.parametrize("base", [0, 2 ** 32 - 1], ids=["base0", "base2p32m1"])
def test_rays_that_no_camera_makes(oracle, base):
    """the probe rays on the lit scene, 2 samples: at base 2^32 - 1 the two samples straddle the 32-bit boundary of the
    Philox counter's sample word"""
    scene, of = M.scene(True)
    o, d, streams, kind = M.probe_rays()
    B, seed = M.FRAME["bounces"], M.FRAME["seed"]
    v = matrix_gpu(True).trace_vertices(o, d, B, streams=streams, samples=M.PROBE_SAMPLES, seed=seed, sample_index_base=base, first_draw=0)
    done, wrong = chain_check(v, scene, matrix_names(of), streams, seed, [base + s for s in range(M.PROBE_SAMPLES)], B)
    print("probe rays, base %d: %d vertices through the oracle's functions; %d vertices, %d inner, %d under a zero suffix, %d non-finite"
          % ((base, done) + census(v)))
    assert wrong == {}
    if base == 0:
        assert_oracle_path(v, H.probe_vertices())
    else:
        assert differing(v.arrays(), H.probe_vertices(), ("direction", "bsdf")) != {}  # (other samples: other paths)


# ---- 4. frames, for the kernels that export no vertices
def assert_frame(g, osc, cam, p, what):
    got, want = g.render_batch(cam, p), osc.render(cam, p)
    bad = differing({"frame": got}, {"frame": want}, ("frame",))
    assert bad == {}, (what, bad)


@pytest.mark.parametrize("flags", [_abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT, 0], ids=["persistent", "wavefront", "default"])
@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "dark"])
def test_frames_of_the_matrix(oracle, lit, inside, flags):
    scene, of, osc, cam, p, rec, length = H.matrix_case(lit, inside)
    g = matrix_gpu(lit)
    g.reset_stats()
    assert_frame(g, osc, cam, M.params(flags=flags), (lit, inside, flags))
    paths = g.stats().kernel_launches[_abi.RPT_K_PATHS]
    if flags:
        assert paths >= 1 if flags == _abi.RPT_FLAG_PERSISTENT else paths == 0


def launch_lines(g, cam, capfd):
    capfd.readouterr()
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    try:
        g.render_batch(cam, make_params(16, 9, 2, 1, seed=1, flags=_abi.RPT_FLAG_PERSISTENT))
    finally:
        del os.environ["RPTGPU_PRINT_LAUNCH"]
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]


@pytest.mark.parametrize("part", range(M.PARTS))
def test_frames_from_the_waves_tables_of_scene_constants(oracle, capfd, part):
    """The persistent kernel reads a hit's material constants from per-wave tables only in its fused form — one light, a
    non-ambient one (scene_plan.h plan_flat) — and only while the tables fit the wave's share of LDS: the dark scene's
    thirds (17 materials each; its 53 objects together do not fit, and the lit scene has four lights).  The launch
    diagnostics must say that this kernel ran, so that a fallback cannot pass in its place."""
    scene, of = M.scene(False, (part, M.PARTS))
    osc = oracle.OracleScene(scene)
    g = GpuScene(scene, 0)
    try:
        for inside in (False, True):
            cam = M.camera(inside)
            lines = launch_lines(g, cam, capfd)
            assert lines and all(FUSED in ln and TABLES in ln for ln in lines), lines
            g.reset_stats()
            assert_frame(g, osc, cam, M.params(flags=_abi.RPT_FLAG_PERSISTENT), (part, inside))
            assert g.stats().kernel_launches[_abi.RPT_K_PATHS] >= 1
    finally:
        g.close()


def test_the_whole_dark_scene_runs_the_fused_kernel_without_the_tables(capfd):
    """(what test_frames_of_the_matrix[dark-*-persistent] ran: the third form of the kernel beside the lit scene's unfused
    one and the thirds' tables)"""
    g = matrix_gpu(False)
    lines = launch_lines(g, M.camera(False), capfd)
    assert lines and all(FUSED in ln and TABLES not in ln for ln in lines), lines
    lines = launch_lines(matrix_gpu(True), M.camera(False), capfd)
    assert lines and all(FUSED not in ln for ln in lines), lines


@pytest.mark.parametrize("lit", [True, False], ids=["lit", "dark"])
def test_the_per_tree_route(oracle, lit, monkeypatch):
    """The wavefront frame, the records and the chain once more on the per-tree route.  Only a tree below its root can
    take it (scene_plan.h route_object: depth >= deep_depth, which is at least 1), and the matrix has none — its only
    mesh is the wall's two triangles, a root leaf.  So this runs on the meshed variant, where the spheres of five
    materials, two of them transparent, are meshes of 168 triangles; the tree-trace kernel must have launched in the
    frame and in the vertex call, or the route was not taken."""
    for k, val in PER_TREE.items():
        monkeypatch.setenv(k, val)
    scene, of, osc, cam, p, rec, length = H.matrix_case(lit, False, True)
    g = GpuScene(scene, 0)
    try:
        g.reset_stats()
        assert_frame(g, osc, cam, M.params(flags=_abi.RPT_FLAG_WAVEFRONT), lit)
        assert g.stats().kernel_launches[_abi.RPT_K_TREE_TRACE] >= 1
        g.reset_stats()
        v = matrix_on_device(g, lit, False, True)
        assert g.stats().kernel_launches[_abi.RPT_K_TREE_TRACE] >= 1
        assert_records(v, rec, length)
        assert_oracle_path(v, H.matrix_vertices(lit, False, True))
        streams = np.arange(p.width * p.height, dtype=np.uint32)
        done, wrong = chain_check(v, scene, matrix_names(of), streams, p.seed, list(range(p.iterations)), p.max_bounces)
        on_mesh = int((np.isin(np.array(of)[np.maximum(v.object, 0)], M.MESHED) & (v.object >= 0)).sum())
        print("meshed %s, per tree: %d vertices, %d inner, %d under a zero suffix, %d non-finite; %d vertices on the meshes; %d through the oracle's functions"
              % (("lit" if lit else "dark",) + census(v) + (on_mesh, done)))
        assert wrong == {} and on_mesh >= 100
    finally:
        g.close()
