"""rptgpu_bake_direct and rptgpu_bake_lightmap_direct without a GPU: the four symbols and RptDirectQuery's layout against the
header, every refusal that comes before the device — through host and device entry points, with its code, its detail and
the arrays untouched —, no CPU fallback, what GpuScene.bake_direct / bake_lightmap_direct lower their arguments to, and
tests/direct_model.py — the header restated in numpy, which the GPU tests hold the library to — against closed forms worked
out by hand and against the oracle's illuminate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from oracle import oracle_ffi as O
from rpt_amd import Light, Material, Object, _abi, polygon, sphere

import direct_cases as DC
import direct_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_bake_direct", "rptgpu_bake_direct_device", "rptgpu_bake_lightmap_direct", "rptgpu_bake_lightmap_direct_device")
FIELDS = ("struct_size", "samples", "seed", "sample_index_base", "precision_mode", "flags")


def test_symbols_and_struct_layout_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and _abi.direct_supported(lib)
    assert [s[0] for s in _abi.DIRECT_SYMBOLS] == list(NAMES)
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptDirectQuery));' + \
          "".join('printf(" %%zu", offsetof(RptDirectQuery, %s));' % f for f in FIELDS) + \
          'printf(" %zu\\n", sizeof(RptLightmapQuery));return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(_abi.RptDirectQuery) == nums[0] == 32
    assert [getattr(_abi.RptDirectQuery, f).offset for f in FIELDS] == nums[1:-1] == [0, 4, 8, 16, 24, 28]
    assert [f for f, _ in _abi.RptDirectQuery._fields_] == list(FIELDS)
    assert C.sizeof(_abi.RptLightmapQuery) == nums[-1]  # the lightmap form takes the lightmap's query as it stands


def direct_query(**kw):
    q = _abi.RptDirectQuery()
    q.struct_size, q.samples, q.seed = C.sizeof(_abi.RptDirectQuery), 4, 1
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def lightmap_query(**kw):
    q = _abi.RptLightmapQuery()
    q.struct_size, q.width, q.height, q.samples, q.seed = C.sizeof(_abi.RptLightmapQuery), 4, 4, 4, 1
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; direct light at caller points runs the "
              "wavefront pipeline's shadow-ray query only").encode()
LM_PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a lightmap's direct light runs the "
                 "wavefront pipeline's shadow-ray query only").encode()
MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
SIZE = b"RptDirectQuery: struct_size is not sizeof(RptDirectQuery)"
LM_SIZE = b"RptLightmapQuery: struct_size is not sizeof(RptLightmapQuery)"
# (what is passed: q, and which arrays are NULL, n) -> the detail
REFUSALS = [
    ("no query", dict(q=None), b"null RptDirectQuery"),
    ("size 0", dict(q=direct_query(struct_size=0)), SIZE),
    ("size 24", dict(q=direct_query(struct_size=24)), SIZE),
    ("size 40", dict(q=direct_query(struct_size=40)), SIZE),
    ("samples", dict(q=direct_query(samples=0)), b"RptDirectQuery: samples == 0"),
    ("mode", dict(q=direct_query(precision_mode=1)), MODE),
    ("persistent", dict(q=direct_query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=direct_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("positions", dict(positions=False), b"null argument"),
    ("normals", dict(normals=False), b"null argument"),
    ("out", dict(out=False), b"null argument"),
    ("2^32 + 1 points without ids", dict(n=(1 << 32) + 1, streams=False),
     b"more than 2^32 points without stream ids (a stream id has 32 bits)"),
    ("handle", dict(), b"null handle"),
    ("handle, no ids", dict(streams=False), b"null handle"),
    ("handle, no points", dict(n=0, positions=False, normals=False, streams=False, out=False), b"null handle"),
]
LM_REFUSALS = [
    ("no query", dict(q=None), b"null RptLightmapQuery"),
    ("size 0", dict(q=lightmap_query(struct_size=0)), LM_SIZE),
    ("size 64", dict(q=lightmap_query(struct_size=64)), LM_SIZE),
    ("width", dict(q=lightmap_query(width=0)), b"RptLightmapQuery: width == 0 or height == 0"),
    ("height", dict(q=lightmap_query(height=0)), b"RptLightmapQuery: width == 0 or height == 0"),
    ("streams", dict(q=lightmap_query(width=1 << 16, height=1 << 16, stream_base=1)),
     b"RptLightmapQuery: width * height + stream_base > 2^32 (a texel's stream id has 32 bits)"),
    ("samples", dict(q=lightmap_query(samples=0)), b"RptLightmapQuery: samples == 0"),
    ("offset", dict(q=lightmap_query(offset=float("inf"))), b"RptLightmapQuery: offset is not finite"),
    ("mode", dict(q=lightmap_query(precision_mode=1)), MODE),
    ("persistent", dict(q=lightmap_query(flags=_abi.RPT_FLAG_PERSISTENT)), LM_PERSISTENT),
    ("out", dict(out=False), b"null out"),
    ("2^31 triangles", dict(n=1 << 31), b"more than 2^31 - 1 triangles (an owner is an int32)"),
    ("positions", dict(positions=False), b"null argument"),
    ("uvs", dict(uvs=False), b"null argument"),
    ("handle", dict(), b"null handle"),
    ("handle, flat", dict(normals=False), b"null handle"),
    # the fields the direct form does not read are not checked: the lightmap call refuses each of these
    ("handle, channels 0", dict(q=lightmap_query(channels=0)), b"null handle"),
    ("handle, unknown channel", dict(q=lightmap_query(channels=1 << 20)), b"null handle"),
    ("handle, 300 bounces", dict(q=lightmap_query(max_bounces=300)), b"null handle"),
    ("handle, NaN distance", dict(q=lightmap_query(max_distance=float("nan"))), b"null handle"),
    ("handle, no triangles", dict(n=0, positions=False, normals=False, uvs=False), b"null handle"),
]


def _another_detail_first(lib):
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_bake_direct_refuses_before_the_device(row, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    pos, nrm, out = np.full(12, 7.0), np.full(12, 7.0), np.full(12, 7.0)
    ids = np.full(4, 7, dtype=np.uint32)
    q = kw.get("q", direct_query())
    use = lambda name, a: a if kw.get(name, True) else None
    qp = C.byref(q) if q is not None else None
    _another_detail_first(lib)
    if device:  # (pointers that are never followed: every row is refused before the device is looked at)
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib.rptgpu_bake_direct_device(None, kw.get("n", 4), p(use("positions", pos)), p(use("normals", nrm)),
                                           p(use("streams", ids)), qp, p(use("out", out)), None)
    else:
        p = lambda a: a.ctypes.data_as(PD) if a is not None else None
        s = use("streams", ids)
        rc = lib.rptgpu_bake_direct(None, kw.get("n", 4), p(use("positions", pos)), p(use("normals", nrm)),
                                    s.ctypes.data_as(C.POINTER(C.c_uint32)) if s is not None else None, qp, p(use("out", out)))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (pos == 7).all() and (nrm == 7).all() and (out == 7).all() and (ids == 7).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(LM_REFUSALS)), ids=[r[0] for r in LM_REFUSALS])
def test_bake_lightmap_direct_refuses_before_the_device(row, device):
    _, kw, detail = LM_REFUSALS[row]
    lib = _abi.load_library()
    pos, nrm, uvs, out = np.full(18, 7.0), np.full(18, 7.0), np.full(12, 7.0), np.full(4 * 4 * 3, 7.0)
    q = kw.get("q", lightmap_query())
    use = lambda name, a: a if kw.get(name, True) else None
    qp = C.byref(q) if q is not None else None
    _another_detail_first(lib)
    if device:
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib.rptgpu_bake_lightmap_direct_device(None, kw.get("n", 2), p(use("positions", pos)), p(use("normals", nrm)),
                                                    p(use("uvs", uvs)), qp, p(use("out", out)), None)
    else:
        p = lambda a: a.ctypes.data_as(PD) if a is not None else None
        rc = lib.rptgpu_bake_lightmap_direct(None, kw.get("n", 2), p(use("positions", pos)), p(use("normals", nrm)),
                                             p(use("uvs", uvs)), qp, p(use("out", out)))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (pos == 7).all() and (nrm == 7).all() and (uvs == 7).all() and (out == 7).all()


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never an answer from the host."""
    scene = rpt_amd.scenes.sphere_scene()[0]
    pos = np.tile(np.array([3.0, -0.5, 0.0]), (4, 1))
    up = np.tile(np.array([0.0, 1.0, 0.0]), (4, 1))
    tri = np.array([[[-1.0, -0.5, -1.0], [-1.0, -0.5, 1.0], [1.0, -0.5, 1.0]]])
    uv = np.array([[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0]]])
    if gpu_available:
        g = rpt_amd.GpuScene(scene)
        out = g.bake_direct(pos, up, samples=3, seed=1)
        assert out.shape == (4, 3) and (out > 0.0).all()  # the lamp stands above the points
        assert (g.bake_direct(pos, -up, samples=3, seed=1) == 0.0).all()
        assert g.bake_lightmap_direct(tri, uv, 4, 4, samples=2, seed=1, offset=0.01).shape == (4, 4, 3)
        return
    for call in (lambda g: g.bake_direct(pos, up, samples=3, seed=1),
                 lambda g: g.bake_lightmap_direct(tri, uv, 4, 4, samples=2, seed=1)):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call(rpt_amd.GpuScene(scene))
        assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


class Recorder:
    """stands where the library stands in a GpuScene: keeps what the entry points are called with"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("rptgpu_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _floats(p, n):
    return np.ctypeslib.as_array(p, shape=(n,)).copy()


def test_what_the_python_calls_lower_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    pos = np.arange(12.0).reshape(4, 3)
    nrm = pos[::-1] * 0.5            # not contiguous: the call sees a contiguous copy
    out = g.bake_direct(pos, nrm, samples=33, seed=(1 << 63) + 5)
    name, (h, n, pp, pn, ps, q, po) = g.lib.calls.pop()
    q = q._obj
    assert name == "rptgpu_bake_direct" and h is g.handle and n == 4 and ps is None
    assert (q.struct_size, q.samples, q.seed, q.sample_index_base, q.precision_mode, q.flags) == (32, 33, (1 << 63) + 5, 0, 0, 0)
    assert (_floats(pp, 12) == pos.ravel()).all() and (_floats(pn, 12) == nrm.ravel()).all()
    assert out.shape == (4, 3) and out.dtype == np.float64 and C.addressof(po.contents) == out.ctypes.data
    mine = np.zeros((4, 3))
    got = g.bake_direct(pos, nrm, samples=2, seed=3, sample_index_base=1 << 40, streams=[9, 8, 7, 1 << 31],
                        flags=_abi.RPT_FLAG_PROFILE_KERNELS, out=mine)
    name, (h, n, pp, pn, ps, q, po) = g.lib.calls.pop()
    q = q._obj
    assert got is mine and C.addressof(po.contents) == mine.ctypes.data
    assert (q.samples, q.seed, q.sample_index_base, q.flags) == (2, 3, 1 << 40, _abi.RPT_FLAG_PROFILE_KERNELS)
    assert np.ctypeslib.as_array(ps, shape=(4,)).tolist() == [9, 8, 7, 1 << 31]

    tri = np.arange(18.0).reshape(2, 3, 3)
    uv = np.arange(12.0).reshape(2, 3, 2) / 16.0
    lm = g.bake_lightmap_direct(tri, uv, 13, 7, samples=5, seed=9, offset=0.25, dilate=3, stream_base=100, sample_index_base=6,
                                flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, pp, pn, pu, q, po) = g.lib.calls.pop()
    q = q._obj
    assert name == "rptgpu_bake_lightmap_direct" and h is g.handle and n == 2 and pn is None
    assert (q.struct_size, q.width, q.height, q.samples, q.dilate, q.stream_base, q.seed, q.sample_index_base, q.offset,
            q.precision_mode, q.flags) == (C.sizeof(_abi.RptLightmapQuery), 13, 7, 5, 3, 100, 9, 6, 0.25, 0,
                                           _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert (_floats(pp, 18) == tri.ravel()).all() and (_floats(pu, 12) == uv.ravel()).all()
    assert lm.shape == (7, 13, 3) and lm.dtype == np.float64 and C.addressof(po.contents) == lm.ctypes.data
    rows = np.concatenate([tri.reshape(2, 9), tri.reshape(2, 9) + 100.0], axis=1)  # a Mesh's rows: positions and normals in one
    g.bake_lightmap_direct(rows, uv, 4, 4, samples=1, seed=1)
    name, (h, n, pp, pn, pu, q, po) = g.lib.calls.pop()
    assert n == 2 and (_floats(pp, 18) == tri.ravel()).all() and (_floats(pn, 18) == tri.ravel() + 100.0).all()
    assert not g.lib.calls
    g.handle = None


def test_the_python_calls_check_their_shapes_and_dtypes():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    z = np.zeros((3, 3))
    kw = dict(samples=4, seed=1)
    with pytest.raises(ValueError, match=r"positions must be an \(n, 3\) float64 array"):
        g.bake_direct(np.zeros(9), z, **kw)
    with pytest.raises(ValueError, match="2 normals for 3 positions"):
        g.bake_direct(z, np.zeros((2, 3)), **kw)
    with pytest.raises(ValueError, match="5 stream ids for 3 points"):
        g.bake_direct(z, z, streams=np.arange(5), **kw)
    with pytest.raises(ValueError, match="out must be"):
        g.bake_direct(z, z, out=np.zeros((3, 1)), **kw)
    with pytest.raises(TypeError):
        g.bake_direct(z, z, 4, 1)  # samples and seed are keyword-only
    with pytest.raises(rpt_amd.RptGpuError) as e:  # well-formed arrays: the library speaks
        g.bake_direct(z, z, **kw)
    assert e.value.code == E and "null handle" in str(e.value)
    g.handle = None


# ---- the model against closed forms worked out by hand
def nothing_in_the_way(o, d):
    return np.full(len(o), np.inf)


def test_the_model_under_a_point_light():
    """a light of colour (8, 4, 2) two units above a point with an up normal: I = colour / 4, wi = up, cos = 1"""
    lights = [Light.Ambient((0.5, 0.5, 0.5)), Light.Point((8.0, 4.0, 2.0), (1.0, 2.0, 3.0))]
    pos, up = np.array([[1.0, 0.0, 3.0]]), np.array([[0.0, 3.0, 0.0]])  # (the normal is normalised by the call)
    assert DM.direct(lights, pos, up, 3, 1, nothing_in_the_way).tolist() == [[2.0, 1.0, 0.5]]
    # a 3-4-5 triangle: the light at distance 5, cos = 4 / 5 -> colour / 25 * 0.8 (each step exact or one rounding)
    lights = [Light.Point((25.0, 50.0, 100.0), (3.0, 4.0, 0.0))]
    got = DM.direct(lights, np.zeros((1, 3)), np.array([[0.0, 1.0, 0.0]]), 1, 1, nothing_in_the_way)
    assert got.tolist() == [[1.0 * 0.8, 2.0 * 0.8, 4.0 * 0.8]]
    # a blocker nearer than the light takes it away, one beyond it does not; exactly at the light: occluded (t > dist fails)
    for t, lit in ((4.0, False), (5.0, False), (np.nextafter(5.0, 6.0), True), (float("nan"), False)):
        got = DM.direct(lights, np.zeros((1, 3)), np.array([[0.0, 1.0, 0.0]]), 1, 1, lambda o, d: np.full(len(o), t))
        assert (got != 0.0).all() == lit and (got != 0.0).any() == lit and not np.signbit(got).any()


def test_the_model_under_a_directional_light():
    """light travelling along (0, -2, 0): wi = up, I = the colour, dist = +inf — only a miss is far enough"""
    lights = [Light.Directional((0.5, 0.25, 1.0), (0.0, -2.0, 0.0))]
    pos = np.array([[0.0, 0.0, 0.0], [5.0, 1.0, -2.0]])
    up = np.tile(np.array([0.0, 1.0, 0.0]), (2, 1))
    assert DM.direct(lights, pos, up, 4, 7, nothing_in_the_way).tolist() == [[0.5, 0.25, 1.0]] * 2
    assert (DM.direct(lights, pos, up, 4, 7, lambda o, d: np.full(len(o), 1e300)) == 0.0).all()  # any hit blocks the sun
    tilted = np.array([[0.0, 3.0, 4.0]])  # cos = 3 / 5
    assert DM.direct(lights, pos[:1], tilted, 1, 7, nothing_in_the_way).tolist() == [[0.5 * 0.6, 0.25 * 0.6, 1.0 * 0.6]]


@pytest.mark.parametrize("normal", [(0.0, -1.0, 0.0), (float("nan"), 1.0, 0.0), (0.0, 0.0, 0.0), (float("inf"), 0.0, 0.0)],
                         ids=["facing away", "NaN", "zero", "inf"])
def test_the_model_gives_plus_zero_without_a_facing_normal(normal):
    lights = [Light.Point((8.0, 4.0, 2.0), (0.0, 2.0, 0.0)), Light.Directional((1.0, 1.0, 1.0), (0.0, -1.0, 0.0))]
    got = DM.direct(lights, np.zeros((1, 3)), np.array([normal]), 2, 1, nothing_in_the_way)
    assert (got == 0.0).all() and not np.signbit(got).any()


def test_the_model_without_a_light_that_casts():
    for lights in ([], [Light.Ambient((1.0, 1.0, 1.0))]):
        got = DM.direct(lights, np.ones((2, 3)), np.ones((2, 3)), 2, 1, None)  # (no query is made)
        assert got.shape == (2, 3) and (got == 0.0).all() and not np.signbit(got).any()


# ---- the model's chain of lights against the oracle's illuminate, light after light with the returned draw count
def lamp(shape, colour=(1.0, 0.9, 0.8), power=30.0):
    return Light.Object(Object(shape).material(Material.light(colour, power)))


def test_the_models_chain_is_the_oracles_illuminate_light_after_light():
    lights = [Light.Point((30.0, 28.0, 25.0), (3.0, 4.0, 3.0)), Light.Ambient((0.1, 0.1, 0.1)),
              lamp(sphere().scale((0.5, 0.5, 0.5)).translate((-3.0, 3.5, 1.0))), Light.Directional((0.4, 0.4, 0.5), (0.3, -1.0, -0.2)),
              lamp(polygon([(-0.5, 3.8, -0.5), (-0.5, 3.8, 0.5), (0.5, 3.8, 0.5), (0.5, 3.8, -0.5)])), Light.Point((1.0, 2.0, 3.0), (0.0, -5.0, 0.0))]
    rs = np.random.RandomState(4)
    for pos in rs.uniform(-2.0, 2.0, (8, 3)):
        for sample in (0, 5, 1 << 40):
            got = DM.chain(lights, pos, DC.SEED, 77, sample, sample_object=DC.oracle_illuminate)
            draw, draws = 0, []
            for light, mine in zip(lights, got):
                if light.kind == _abi.RPT_LIGHT_AMBIENT:
                    assert mine is None
                    continue
                I, wi, dist, draw = O.illuminate(light, pos, seed=DC.SEED, pixel=77, sample=sample, draw=draw)
                draws.append(draw)
                assert mine[0].tobytes() == I.tobytes() and mine[1].tobytes() == wi.tobytes() and mine[2] == dist
            # the two lamps draw, the others do not: the second lamp starts where the first one stopped
            assert draws[0] == 0 and draws[1] > 0 and draws[2] == draws[1] and draws[3] > draws[2] and draws[4] == draws[3]


# ---- the GPU tests' inputs, checked here with the oracle alone
@pytest.mark.parametrize("name", DC.SCENES)
def test_the_points_show_both_outcomes(name):
    """of the (point, sample, light) triples of every scene at least 10 % contribute and at least 10 % do not — facing away
    or occluded —, and the result is not all zero"""
    pos, nrm, ids = DC.points(name)
    lights = DC.scene(name)[0].lights
    out, det = DM.direct(lights, pos, nrm, 16, DC.SEED, DC.oracle_closest_t(name), streams=ids, illuminate=DC.oracle_illuminate,
                         details=True)
    casting = sum(l.kind != _abi.RPT_LIGHT_AMBIENT for l in lights)
    assert len(det["adds"]) == DC.N_POINTS * 16 * casting
    assert 0.10 <= det["adds"].mean() <= 0.90, det["adds"].mean()
    assert (det["cosv"] <= 0.0).any() and ((det["cosv"] > 0.0) & ~det["adds"]).any()  # both ways of not contributing
    assert (out != 0.0).any() and np.isfinite(out).all()
    lengths = np.linalg.norm(nrm, axis=1)
    assert lengths.min() < 0.9 and lengths.max() > 1.1  # the normals are no unit vectors: the call's normalize is in the test
    if name == "two_lamps":
        # a lamp that faces away stands in front of one that lights the point, on the same stream — often
        first, second = det["light"] == 0, det["light"] == 1
        assert (first.sum(), second.sum()) == (DC.N_POINTS * 16,) * 2
        assert ((det["cosv"][first] <= 0.0) & det["adds"][second]).mean() >= 0.10
