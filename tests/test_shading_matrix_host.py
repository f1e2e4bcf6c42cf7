"""tests/shading_matrix.py without a GPU: its oracle_path is the oracle's own path, record for record, and the scenes it
builds cover what tests/test_gpu_vertices_oracle.py is there to see — counted from the oracle alone, so that the code under
test cannot bend the counts.  The bounds are the ones the checks were planned with; the counts this layout gives stand
in shading_matrix's docstring."""
import functools

import numpy as np
import pytest

import rpt_amd

import shading_matrix as M
import test_gpu_trace_rays as R

CORNELL_SAMPLES = (5, 6, 7)


def equal_bits(a, b):
    """bit for bit, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def matrix_case(lit, inside, meshed=False):
    """(scene, material of every object, OracleScene, camera, params, trace_sample's records and lengths) of a matrix frame"""
    from oracle import oracle_ffi
    scene, of = M.scene(lit, None, meshed)
    osc = oracle_ffi.OracleScene(scene)
    cam, p = M.camera(inside), M.params()
    rec, length = M.records(osc, cam, p)
    return scene, of, osc, cam, p, rec, length


@functools.lru_cache(maxsize=None)
def matrix_vertices(lit, inside, meshed=False):
    """oracle_path of every pixel and sample of the frame, on the oracle's camera rays (a pinhole: one ray per sample)"""
    from oracle import oracle_ffi
    scene, of, osc, cam, p, rec, length = matrix_case(lit, inside, meshed)
    S = p.iterations
    out = []
    for s in range(S):
        o, d, streams, draws = R.camera_rays(oracle_ffi, cam, M.params(s, 1), s)
        assert (draws == 2).all()
        out.append(M.oracle_vertices(osc, scene, o, d, streams, 1, s, 2, p.seed, p.max_bounces))
    return {k: np.concatenate([v[k] for v in out], axis=1) for k in out[0]}


def assert_path_is_record(v, rec, length):
    """v: oracle_vertices' arrays (n, S, ...); rec, length: records() of the same frame, pixel-major then sample"""
    n, S = v["length"].shape
    assert (v["length"].reshape(-1) == length).all(), "%d lengths differ" % (v["length"].reshape(-1) != length).sum()
    rec = rec.reshape(n, S, rec.shape[1], 8)
    assert equal_bits(v["radiance"], rec[..., 0:3])
    assert equal_bits(v["bsdf"], rec[..., 3:6])
    assert equal_bits(v["inv_pdf"], rec[..., 6])
    assert equal_bits(v["abs_cos"], rec[..., 7])


@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "dark"])
def test_oracle_path_is_trace_sample_on_the_matrix(oracle, lit, inside):
    scene, of, osc, cam, p, rec, length = matrix_case(lit, inside)
    assert_path_is_record(matrix_vertices(lit, inside), rec, length)


@pytest.mark.parametrize("name", ["cornell", "coverage", "glass", "wine_glass"])
def test_oracle_path_is_trace_sample_on_the_small_scenes(oracle, name):
    """(cornell is the one the chain check runs on; the others pin the vertex radiance under every light kind, object
    lights of every shape and an HDRI environment, for the samples that no trace_sample record covers)"""
    scene, camera, p, o, d, streams, draws, want = R.case(name, 5)
    osc = oracle.OracleScene(scene)
    p3 = rpt_amd.make_params(p.width, p.height, p.max_bounces, 1, seed=p.seed, sample_index_base=5)
    rec, length = M.records(osc, camera, p3)
    v = M.oracle_vertices(osc, scene, o, d, streams, 1, 5, 2, p.seed, p.max_bounces)
    assert_path_is_record(v, rec, length)
    assert len(np.unique(length)) >= 3  # (not on trivial paths)


def test_every_material_is_one_scene_create_accepts():
    assert len(M.MATERIALS) == 51 and len({(m.color, m.index, m.roughness, m.metallic, m.emittance, m.transparent) for _, m in M.MATERIALS}) == 51
    for name, m in M.MATERIALS:
        assert 0.0 <= M.lobe_probability(m) <= 1.0, name
    assert M.lobe_probability(dict(M.MATERIALS)["white metal"]) == 1.0  # gen_bool takes no draw
    assert sum(M.lobe_probability(m) == 1.0 for _, m in M.MATERIALS) == 1
    for r in M.ROUGHNESS:
        for ix in M.INDEX:
            for kind in M.KINDS:
                assert "%s r=%g n=%.8g" % (kind, r, ix) in dict(M.MATERIALS)
    name, m = M.MATERIALS[M.INSIDE]
    assert m.transparent and M.is_cube(M.INSIDE) and m.index == 2.4
    # the parts the persistent kernel's tables hold: every material in exactly one of them
    parts = [M.scene(False, (k, M.PARTS))[1] for k in range(M.PARTS)]
    assert sorted(i for of in parts for i in of if i >= 0) == list(range(51))


# ---- the meshed variant, for the per-tree route
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "dark"])
def test_the_meshed_scenes(oracle, lit):
    """oracle_path is trace_sample's record there too, every meshed material is shaded at least 10 times in the frame
    (the bound of the other materials), on the mesh itself, and a mesh is large enough for a kd-tree below its root (the
    build makes a leaf of fewer than 16 triangles)"""
    scene, of, osc, cam, p, rec, length = matrix_case(lit, False, True)
    v = matrix_vertices(lit, False, True)
    assert_path_is_record(v, rec, length)
    assert M.MESH_TRIANGLES >= 64 and len(M.sphere_mesh()) == M.MESH_TRIANGLES
    counts = M.outcomes(v, of, p.max_bounces)
    inner, zero, nonfinite = M.census(rec, length)
    print("meshed %s: %d inner vertices, %d under a zero suffix, %d non-finite; on the meshes %s"
          % ("lit" if lit else "dark", inner, zero, nonfinite, {M.MATERIALS[i][0]: counts[i][0] for i in M.MESHED}))
    for i in M.MESHED:
        assert not M.is_cube(i) and counts[i][0] >= 10, (M.MATERIALS[i][0], counts[i])
    assert any(M.MATERIALS[i][1].transparent for i in M.MESHED)
    assert not matrix_vertices(lit, False)["bsdf"].tobytes() == v["bsdf"].tobytes()  # (facets: other paths than the spheres')


# ---- the coverage conditions
def test_cornell_has_vertices_under_a_zero_suffix(oracle):
    """at least 30 % of cornell's inner vertices (pinhole camera, test_gpu_trace_rays.SIZES, samples 5 to 7)"""
    scene, camera, p, o, d, streams, draws, want = R.case("cornell", 5)
    p3 = rpt_amd.make_params(p.width, p.height, p.max_bounces, len(CORNELL_SAMPLES), seed=p.seed, sample_index_base=CORNELL_SAMPLES[0])
    rec, length = M.records(oracle.OracleScene(scene), camera, p3)
    inner, zero, nonfinite = M.census(rec, length)
    print("cornell: %d paths, %d inner vertices, %d under a zero suffix (%.1f %%), %d non-finite" % (len(length), inner, zero, 100.0 * zero / inner, nonfinite))
    assert len(length) == 2331 and zero >= 0.30 * inner


def test_the_matrix_scenes_have_vertices_under_a_zero_suffix_and_non_finite_factors(oracle):
    """the outside camera's frame: at least 50 % of the dark scene's inner vertices and 40 % of the lit scene's lie under
    an all-zero suffix; at least 10 vertices of the matrix frames carry a non-finite factor.  The bounds are read as
    bounds on the outside camera's frame on purpose (shading_matrix's docstring says why): the inside frames are
    printed beside them and carry none"""
    total = 0
    for lit, bound in ((False, 0.50), (True, 0.40)):
        for inside in (False, True):
            rec, length = matrix_case(lit, inside)[5:]
            inner, zero, nonfinite = M.census(rec, length)
            print("%s, %s camera: %d paths, %d inner vertices, %d under a zero suffix (%.1f %%), %d non-finite"
                  % ("lit" if lit else "dark", "inside" if inside else "outside", len(length), inner, zero, 100.0 * zero / inner, nonfinite))
            total += nonfinite
            if not inside:
                assert zero >= bound * inner
    assert total >= 10


@functools.lru_cache(maxsize=None)
def probe_vertices():
    from oracle import oracle_ffi
    scene, of = M.scene(True)
    o, d, streams, kind = M.probe_rays()
    return M.oracle_vertices(oracle_ffi.OracleScene(scene), scene, o, d, streams, M.PROBE_SAMPLES, 0, 0, M.FRAME["seed"], M.FRAME["bounces"])


def test_every_material_is_shaded_and_every_transparent_one_in_every_way(oracle):
    """every material is the material of at least 10 inner vertices of the two scenes' two frames; every transparent one
    shows a reflection, a transmission and a None among those frames and the probe rays — but for index exactly 1.0,
    where sample_f's refraction cannot fail (shading_matrix.probe_rays says why) and the first two are asked for"""
    B = M.FRAME["bounces"]
    total = {i: np.zeros(4, dtype=np.int64) for i in range(len(M.MATERIALS))}
    for lit in (True, False):
        for inside in (False, True):
            got = M.outcomes(matrix_vertices(lit, inside), matrix_case(lit, inside)[1], B)
            for i, c in got.items():
                total[i] += c
    for i, (name, m) in enumerate(M.MATERIALS):
        assert total[i][0] >= 10, (name, total[i])
    frames = {i: c.copy() for i, c in total.items()}
    for i, c in M.outcomes(probe_vertices(), M.scene(True)[1], B).items():
        total[i] += c
    for i in M.TRANSPARENT:
        name, m = M.MATERIALS[i]
        print("%-36s frames %s, with the probe rays %s" % (name, frames[i].tolist(), total[i].tolist()))
        assert total[i][1] >= 1 and total[i][2] >= 1, (name, total[i])
        if m.index != 1.0:
            assert total[i][3] >= 1, (name, total[i])
        else:  # the claim as a check: with eta_t = 1 no path of the frames or the probe rays ends on a None
            assert total[i][3] == 0, (name, total[i])
    print("least inner vertices of a material: %d" % min(c[0] for c in frames.values()))


def test_the_probe_rays():
    o, d, streams, kind = M.probe_rays()
    assert 200 <= len(o) <= 400 and o.shape == d.shape == (len(o), 3) and streams.dtype == np.uint32
    lengths = np.linalg.norm(d[[k == "scaled" for k in kind]], axis=1)
    assert np.isclose(lengths, 3.0).any() and np.isclose(lengths, 1e-3).any()
    assert {"scaled", "inside", "inside grazing", "outside grazing"} == set(kind)
    assert len(np.unique(streams >> 24)) > 32  # scattered
    # the first vertex of an inside ray is an exit of a transparent object
    v = probe_vertices()
    scene, of = M.scene(True)
    for r in np.flatnonzero([k.startswith("inside") for k in kind]):
        obj = int(v["object"][r, 0, 0])
        assert obj >= 0 and M.MATERIALS[of[obj]][1].transparent
        assert (v["direction"][r, 0, 0] * v["normal"][r, 0, 0]).sum() > 0.0
