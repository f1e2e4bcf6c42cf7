"""rptgpu_bake_lightmap without a GPU: the two symbols, detected the way a binding detects them, and both structs' layouts
against the header; every refusal that comes before the device — through the host and the device entry point, with its code,
its detail and the arrays untouched —; what GpuScene.bake_lightmap lowers its arguments to; the YARDSTICK of
tests/test_gpu_lightmap.py, tests/lightmap_model.py, against closed forms (the quad's 196 centres and its diagonal, dyadic
barycentrics, a dilation by hand); rpt_amd.lightmap.load_obj_texcoords on an OBJ written here; the sizing header
(rpt_amd/csrc/lightmap_plan.h) in a stand-alone program (tests/cpp/lightmap_plan_check.cpp), plain and under
AddressSanitizer + UBSan."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi, lightmap

import lightmap_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_bake_lightmap", "rptgpu_bake_lightmap_device")
QUERY_FIELDS = ("struct_size", "channels", "width", "height", "samples", "max_bounces", "dilate", "stream_base", "seed",
                "sample_index_base", "offset", "max_distance", "precision_mode", "flags")
ARRAY_FIELDS = ("struct_size", "reserved", "irradiance", "ao", "owner", "barycentric", "position", "normal")
BITS = (("irradiance", _abi.RPT_LIGHTMAP_IRRADIANCE), ("ao", _abi.RPT_LIGHTMAP_AO), ("owner", _abi.RPT_LIGHTMAP_OWNER),
        ("barycentric", _abi.RPT_LIGHTMAP_BARYCENTRIC), ("position", _abi.RPT_LIGHTMAP_POSITION),
        ("normal", _abi.RPT_LIGHTMAP_NORMAL))


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and _abi.lightmap_supported(lib)
    assert tuple(s[0] for s in _abi.LIGHTMAP_SYMBOLS) == NAMES and not set(NAMES) & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7

    class Older:  # a library without the two: still ABI 7, and the detection says so
        rptgpu_bake_probes = None
    assert not _abi.lightmap_supported(Older())
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptLightmapQuery));' + \
          "".join('printf(" %%zu", offsetof(RptLightmapQuery, %s));' % f for f in QUERY_FIELDS) + \
          'printf(" %zu", sizeof(RptLightmapArrays));' + \
          "".join('printf(" %%zu", offsetof(RptLightmapArrays, %s));' % f for f in ARRAY_FIELDS) + \
          'printf(" %u %u %u %u %u %u", RPT_LIGHTMAP_IRRADIANCE, RPT_LIGHTMAP_AO, RPT_LIGHTMAP_OWNER, RPT_LIGHTMAP_BARYCENTRIC, ' \
          'RPT_LIGHTMAP_POSITION, RPT_LIGHTMAP_NORMAL);printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    q, a, bits = nums[:15], nums[15:24], nums[24:]
    assert C.sizeof(_abi.RptLightmapQuery) == q[0] == 72
    assert [getattr(_abi.RptLightmapQuery, f).offset for f in QUERY_FIELDS] == q[1:] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 68]
    assert [f for f, _ in _abi.RptLightmapQuery._fields_] == list(QUERY_FIELDS)
    assert C.sizeof(_abi.RptLightmapArrays) == a[0] == 56
    assert [getattr(_abi.RptLightmapArrays, f).offset for f in ARRAY_FIELDS] == a[1:] == [0, 4, 8, 16, 24, 32, 40, 48]
    assert [f for f, _ in _abi.RptLightmapArrays._fields_] == list(ARRAY_FIELDS)
    assert bits == [b for _, b in BITS] == [1, 2, 4, 8, 16, 32] and _abi.RPT_LIGHTMAP_ALL == 63
    assert rpt_amd.RPT_LIGHTMAP_OWNER == 4 and rpt_amd.lightmap is lightmap


W, H, N_TRIS = 4, 2, 2


def query(**kw):
    q = _abi.RptLightmapQuery()
    q.struct_size, q.channels = C.sizeof(_abi.RptLightmapQuery), _abi.RPT_LIGHTMAP_ALL
    q.width, q.height, q.samples, q.max_bounces, q.max_distance = W, H, 4, 2, float("inf")
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a lightmap's gathers run the probe "
              "and the ambient-occlusion calls' drivers").encode()
MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
Q_SIZE = b"RptLightmapQuery: struct_size is not sizeof(RptLightmapQuery)"
A_SIZE = b"RptLightmapArrays: struct_size is not sizeof(RptLightmapArrays)"
UNKNOWN = b"RptLightmapQuery: channels names an unknown RPT_LIGHTMAP_* bit"
NO_SIZE = b"RptLightmapQuery: width == 0 or height == 0"
STREAMS = b"RptLightmapQuery: width * height + stream_base > 2^32 (a texel's stream id has 32 bits)"
NO_SAMPLES = b"RptLightmapQuery: samples == 0 with RPT_LIGHTMAP_IRRADIANCE or RPT_LIGHTMAP_AO named"
OFFSET = b"RptLightmapQuery: offset is not finite"
RAW = _abi.RPT_LIGHTMAP_OWNER | _abi.RPT_LIGHTMAP_BARYCENTRIC | _abi.RPT_LIGHTMAP_POSITION | _abi.RPT_LIGHTMAP_NORMAL
# (what is passed: q, the arrays struct's fields, which arrays are NULL, n_tris) -> the detail
REFUSALS = [
    ("no query", dict(q=None), b"null RptLightmapQuery"),
    ("no arrays struct", dict(arrays=None), b"null RptLightmapArrays"),
    ("query size 0", dict(q=query(struct_size=0)), Q_SIZE),
    ("query size 64", dict(q=query(struct_size=64)), Q_SIZE),
    ("query size 80", dict(q=query(struct_size=80)), Q_SIZE),
    ("arrays size 0", dict(a_size=0), A_SIZE),
    ("arrays size 48", dict(a_size=48), A_SIZE),
    ("arrays size 64", dict(a_size=64), A_SIZE),
    ("no channel", dict(q=query(channels=0)), b"RptLightmapQuery: channels == 0 (name at least one RPT_LIGHTMAP_* channel)"),
    ("unknown bit", dict(q=query(channels=64 | _abi.RPT_LIGHTMAP_OWNER)), UNKNOWN),
    ("high bit", dict(q=query(channels=1 << 31)), UNKNOWN),
    ("reserved", dict(reserved=1), b"RptLightmapArrays: reserved != 0"),
    ("irradiance", dict(irradiance=False), b"RptLightmapArrays: RPT_LIGHTMAP_IRRADIANCE is named but irradiance is NULL"),
    ("ao", dict(ao=False), b"RptLightmapArrays: RPT_LIGHTMAP_AO is named but ao is NULL"),
    ("owner", dict(owner=False), b"RptLightmapArrays: RPT_LIGHTMAP_OWNER is named but owner is NULL"),
    ("barycentric", dict(barycentric=False), b"RptLightmapArrays: RPT_LIGHTMAP_BARYCENTRIC is named but barycentric is NULL"),
    ("position", dict(position=False), b"RptLightmapArrays: RPT_LIGHTMAP_POSITION is named but position is NULL"),
    ("normal", dict(normal=False), b"RptLightmapArrays: RPT_LIGHTMAP_NORMAL is named but normal is NULL"),
    ("width 0", dict(q=query(width=0)), NO_SIZE),
    ("height 0", dict(q=query(height=0)), NO_SIZE),
    ("2^32 texels and a base", dict(q=query(width=65536, height=65536, stream_base=1)), STREAMS),
    ("a base at the top", dict(q=query(stream_base=0xFFFFFFFF - W * H + 2)), STREAMS),
    ("more than 2^32 texels", dict(q=query(width=0xFFFFFFFF, height=2)), STREAMS),
    ("no samples, irradiance", dict(q=query(samples=0, channels=_abi.RPT_LIGHTMAP_IRRADIANCE | RAW)), NO_SAMPLES),
    ("no samples, ao", dict(q=query(samples=0, channels=_abi.RPT_LIGHTMAP_AO)), NO_SAMPLES),
    ("bounces", dict(q=query(max_bounces=255)), b"RptLightmapQuery: max_bounces > 254"),
    ("offset nan", dict(q=query(offset=float("nan"))), OFFSET),
    ("offset inf", dict(q=query(offset=float("-inf"))), OFFSET),
    ("mode", dict(q=query(precision_mode=1)), MODE),
    ("persistent", dict(q=query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("rays persistent | wavefront", dict(q=query(flags=_abi.RPT_FLAG_RAYS_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)),
     b"RptLightmapQuery: RPT_FLAG_RAYS_PERSISTENT | RPT_FLAG_WAVEFRONT \xe2\x80\x94 the two flags name different routes"),
    ("too many triangles", dict(n=1 << 31), b"more than 2^31 - 1 triangles (an owner is an int32)"),
    ("positions", dict(positions=False), b"null argument"),
    ("uvs", dict(uvs=False), b"null argument"),
    ("handle", dict(), b"null handle"),
    ("handle, no normals", dict(normals=False), b"null handle"),
    ("handle, raw channels and no samples", dict(q=query(samples=0, channels=RAW), irradiance=False, ao=False), b"null handle"),
    ("handle, one channel and only its array", dict(q=query(channels=_abi.RPT_LIGHTMAP_AO), irradiance=False, owner=False,
                                                     barycentric=False, position=False, normal=False), b"null handle"),
    ("handle, no triangles", dict(n=0, positions=False, normals=False, uvs=False), b"null handle"),
    ("handle, rays persistent alone", dict(q=query(flags=_abi.RPT_FLAG_RAYS_PERSISTENT)), b"null handle"),
    ("handle, the last stream id", dict(q=query(stream_base=0xFFFFFFFF - W * H + 1)), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_bake_lightmap_refuses_before_the_device(row, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    ins = {"positions": np.full(9 * N_TRIS, 7.0), "normals": np.full(9 * N_TRIS, 7.0), "uvs": np.full(6 * N_TRIS, 7.0)}
    n = W * H
    outs = {"irradiance": np.full(3 * n, 7.0), "ao": np.full(n, 7.0), "owner": np.full(n, 7, dtype=np.int32),
            "barycentric": np.full(3 * n, 7.0), "position": np.full(3 * n, 7.0), "normal": np.full(3 * n, 7.0)}
    q = kw.get("q", query())
    a = _abi.RptLightmapArrays()
    a.struct_size, a.reserved = kw.get("a_size", C.sizeof(_abi.RptLightmapArrays)), kw.get("reserved", 0)
    types = dict(_abi.RptLightmapArrays._fields_)
    for name, arr in outs.items():  # (device: pointers that are never followed — every row is refused before the device)
        if kw.get(name, True):
            setattr(a, name, arr.ctypes.data_as(types[name]))
    ap = C.byref(a) if kw.get("arrays", True) is not None else None
    qp = C.byref(q) if q is not None else None
    use = lambda name: ins[name] if kw.get(name, True) else None
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    if device:
        p = lambda arr: C.c_void_p(arr.ctypes.data) if arr is not None else None
        rc = lib.rptgpu_bake_lightmap_device(None, kw.get("n", N_TRIS), p(use("positions")), p(use("normals")), p(use("uvs")), qp, ap, None)
    else:
        p = lambda arr: arr.ctypes.data_as(PD) if arr is not None else None
        rc = lib.rptgpu_bake_lightmap(None, kw.get("n", N_TRIS), p(use("positions")), p(use("normals")), p(use("uvs")), qp, ap)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert all((arr == 7).all() for arr in ins.values()) and all((arr == 7).all() for arr in outs.values())


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


def test_what_the_python_call_lowers_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    rows = np.arange(3 * 18, dtype=np.float64).reshape(3, 18)          # a Mesh's rows: positions and normals in one
    uvs = np.arange(18, dtype=np.float64).reshape(3, 3, 2) / 32.0
    out = g.bake_lightmap(rows, uvs, 5, 3, samples=8, max_bounces=3, seed=77, offset=0.25, dilate=2, channels=_abi.RPT_LIGHTMAP_ALL,
                          max_distance=9.0, stream_base=11, sample_index_base=6, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, pp, pn, pu, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert name == "rptgpu_bake_lightmap" and h is g.handle and n == 3
    assert [getattr(q, f) for f in QUERY_FIELDS] == [72, 63, 5, 3, 8, 3, 2, 11, 77, 6, 0.25, 9.0, _abi.RPT_PRECISION_F64_STRICT,
                                                     _abi.RPT_FLAG_GENERAL_TRAVERSAL]
    assert (a.struct_size, a.reserved) == (56, 0)
    floats = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
    address = lambda p: C.cast(p, C.c_void_p).value
    assert (floats(pp, 27) == rows[:, :9].ravel()).all() and (floats(pn, 27) == rows[:, 9:].ravel()).all()
    assert (floats(pu, 18) == uvs.ravel()).all()
    assert sorted(out) == ["ao", "barycentric", "irradiance", "normal", "owner", "position"]
    assert out["ao"].shape == (3, 5) and out["owner"].shape == (3, 5) and out["owner"].dtype == np.int32
    for k in ("irradiance", "barycentric", "position", "normal"):
        assert out[k].shape == (3, 5, 3) and out[k].dtype == np.float64
    for k, v in out.items():
        assert address(getattr(a, k)) == v.ctypes.data
    # positions alone, flat normals, the default channels: the other pointers stay NULL
    out = g.bake_lightmap(rows[:, :9].reshape(3, 3, 3), uvs, 5, 3, samples=4, seed=1)
    name, (h, n, pp, pn, pu, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert pn is None and sorted(out) == ["irradiance", "owner"] and q.channels == 5 and q.max_distance == float("inf")
    assert (q.dilate, q.stream_base, q.max_bounces, q.offset, q.flags) == (0, 0, 0, 0.0, 0)
    assert not a.ao and not a.barycentric and not a.position and not a.normal and address(a.owner) == out["owner"].ctypes.data
    # ... and with normals of their own
    g.bake_lightmap(rows[:, :9].reshape(3, 3, 3), uvs, 5, 3, normals=rows[:, 9:].reshape(3, 3, 3), samples=4, seed=1)
    name, (h, n, pp, pn, pu, q, a) = g.lib.calls.pop()
    assert (floats(pn, 27) == rows[:, 9:].ravel()).all()
    assert not g.lib.calls
    z = np.zeros((3, 3, 3))
    for bad, word in ((lambda: g.bake_lightmap(rows, uvs, 5, 3, normals=z, seed=1), "hold their normals"),
                      (lambda: g.bake_lightmap(z, uvs[:2], 5, 3, seed=1), "2 uvs for 3 triangles"),
                      (lambda: g.bake_lightmap(z, uvs, 5, 3, normals=z[:1], seed=1), "1 normals for 3 triangles"),
                      (lambda: g.bake_lightmap(z.astype(np.float32), uvs, 5, 3, seed=1), r"triangles must be an \(n, 3, 3\) float64"),
                      (lambda: g.bake_lightmap(z, uvs.reshape(3, 6), 5, 3, seed=1), r"uvs must be an \(n, 3, 2\) float64")):
        with pytest.raises(ValueError, match=word):
            bad()
    g.handle = None


# ---- the yardstick against closed forms
def quad(lo=1.0 / 16.0, hi=15.0 / 16.0):
    """two triangles over the uv square [lo, hi]^2, sharing the diagonal from (lo, lo) to (hi, hi)"""
    return np.array([[[lo, lo], [hi, lo], [hi, hi]], [[lo, lo], [hi, hi], [lo, hi]]])


def test_the_model_owns_the_quads_196_centres_and_gives_the_diagonal_to_triangle_0():
    owner, bary = M.raster(quad(), 16, 16)      # texel space [1, 15]^2
    inside = np.zeros((16, 16), dtype=bool)
    inside[1:15, 1:15] = True                     # centres 1.5 .. 14.5 in both axes
    assert ((owner >= 0) == inside).all() and int((owner >= 0).sum()) == 196
    covers, e, area = M.coverage(quad(), 16, 16)
    i = np.arange(1, 15)
    assert covers[0][i, i].all() and covers[1][i, i].all()   # the diagonal's centres (i + 0.5, i + 0.5): both cover them
    assert (owner[i, i] == 0).all()
    y, x = np.mgrid[0:16, 0:16]
    assert (owner[inside & (x > y)] == 0).all() and (owner[inside & (x < y)] == 1).all()
    assert (area == 196.0).all() and int(covers[0].sum()) + int(covers[1].sum()) == 196 + 14
    # three rounded quotients e / 196 (not 1 - b1 - b2): they sum to one within their roundings, and are +0.0 outside
    assert (np.abs(bary[inside].sum(axis=1) - 1.0) <= 4 * 2.0 ** -53).all() and (bary[~inside] == 0.0).all()
    assert (bary[inside] >= 0.0).all() and (bary[i, i][:, 1] == 0.0).all()   # the diagonal is triangle 0's edge A3 A1
    # mirrored: the same coverage from area < 0
    m_owner, m_bary = M.raster(quad()[:, ::-1], 16, 16)
    assert M.coverage(quad()[:, ::-1], 16, 16)[2].tolist() == [-196.0, -196.0] and ((m_owner >= 0) == inside).all()
    assert np.array_equal(m_bary, bary[:, :, ::-1])  # (values: a zero's sign follows its edge's direction)


def test_barycentrics_on_a_vertex_aligned_lattice_are_exact_dyadic_fractions():
    """a right triangle with legs of 8 texels from the corner (0, 0): e / area = multiples of 8 / 64, and the position they
    interpolate is the affine map of the centre, exactly"""
    uv = np.array([[[0.0, 0.0], [0.5, 0.0], [0.0, 0.5]]])
    owner, bary = M.raster(uv, 16, 16)
    y, x = np.mgrid[0:16, 0:16]
    cx, cy = x + 0.5, y + 0.5
    inside = cx + cy <= 8.0
    assert ((owner == 0) == inside).all() and int(inside.sum()) == 36   # 8 + 7 + ... + 1, the hypotenuse's centres included
    assert (owner[(cx + cy) == 8.0] == 0).all()                          # ... (edges are inclusive)
    want = np.stack([(8.0 - cx - cy) / 8.0, cx / 8.0, cy / 8.0], axis=-1)
    assert M.same(bary[inside], want[inside]) and (bary[inside] * 16.0 == np.round(bary[inside] * 16.0)).all()
    pos = np.array([[[1.0, 2.0, 3.0], [9.0, 2.0, 3.0], [1.0, 2.0, 19.0]]])  # x = 1 + cx, z = 3 + 2 cy
    g, n = M.surface(owner, bary, pos, None, 0.5)
    assert (n[inside] == np.array([0.0, -1.0, 0.0])).all()                 # (8, 0, 0) x (0, 0, 16) = (0, -128, 0)
    assert (g[inside] == np.stack([1.0 + cx, np.full_like(cx, 1.5), 3.0 + 2.0 * cy], axis=-1)[inside]).all()
    assert (g[~inside] == 0.0).all() and (n[~inside] == 0.0).all()
    g2, n2 = M.surface(owner, bary, pos, np.broadcast_to(np.array([0.0, 0.0, 2.0]), (1, 3, 3)), 0.0)
    assert (n2[inside] == np.array([0.0, 0.0, 1.0])).all() and (g2[inside][:, 1] == 2.0).all()


def test_the_models_degenerate_triangles_cover_nothing_and_the_lowest_index_wins():
    nan = float("nan")
    uv = np.array([[[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]],          # zero area
                   [[0.1, 0.1], [nan, 0.2], [0.3, 0.9]],          # a NaN vertex
                   [[1.5, 1.5], [2.5, 1.5], [1.5, 2.5]],          # wholly outside
                   [[-4.0, -4.0], [9.0, -4.0], [-4.0, 9.0]],      # much larger than the map
                   [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]])         # overlaps it everywhere it goes
    covers, e, area = M.coverage(uv, 8, 8)
    assert not covers[:3].any() and covers[3].all() and covers[4].any()
    owner, _ = M.raster(uv, 8, 8)
    assert (owner == 3).all()
    owner, _ = M.raster(uv[::-1], 8, 8)
    assert set(owner.ravel().tolist()) == {0, 1} and ((owner == 0) == covers[4]).all()
    assert (M.raster(uv[:3], 8, 8)[0] == -1).all() and (M.raster(uv[:0], 3, 2)[0] == -1).all()


def test_the_dilation_by_hand_on_a_5x5_map():
    v = np.zeros((5, 5))
    f = np.zeros((5, 5), dtype=bool)
    v[2, 2], f[2, 2] = 8.0, True
    v[0, 0], f[0, 0] = 2.0, True
    v1, f1 = M.dilate(v, f, 1)
    ring = np.zeros((5, 5), dtype=bool)
    ring[1:4, 1:4] = True
    assert (f1 == (ring | np.array([[1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0] * 5, [0] * 5, [0] * 5], dtype=bool))).all()
    assert v1[1, 1] == 5.0                      # both sources: (2 + 8) / 2, in the order dy = -1 first
    assert v1[0, 1] == 2.0 and v1[1, 0] == 2.0 and v1[1, 2] == 8.0 and v1[3, 3] == 8.0 and v1[2, 2] == 8.0 and v1[0, 0] == 2.0
    assert (v1[~f1] == 0.0).all() and v1[0, 2] == 0.0
    # the second round reads the FIRST round's state only: (0, 2) sees (0, 1) = 2, (1, 1) = 5, (1, 2) = 8, (1, 3) = 8
    v2, f2 = M.dilate(v, f, 2)
    assert f2.all() and v2[0, 2] == ((2.0 + 5.0) + 8.0 + 8.0) / 4.0
    assert v2[4, 4] == 8.0 and v2[4, 0] == 8.0 and v2[0, 4] == 8.0   # from (3, 3), (3, 1), (1, 3) alone
    assert M.same(M.dilate(v1, f1, 1)[0], v2)                         # rounds compose
    # a model that read its own writes would carry 2.0 along row 0 in ONE round; this one does not
    assert v1[0, 3] == 0.0 and not f1[0, 3]
    v9, f9 = M.dilate(v, f, 9)
    assert M.same(v9, v2)                                              # nothing left to fill: further rounds change nothing
    # the order of the sum, to the bit: three neighbours whose sum depends on it
    w = np.zeros((3, 3))
    g = np.zeros((3, 3), dtype=bool)
    w[0, 0], w[0, 2], w[2, 1] = 1e16, 1.0, -1e16
    g[0, 0] = g[0, 2] = g[2, 1] = True
    assert M.dilate(w, g, 1)[0][1, 1] == ((0.0 + 1e16) + 1.0 + -1e16) / 3.0 == 0.0
    # vectors dilate per component, and an empty map stays empty
    v3 = np.stack([v, 2.0 * v, -v], axis=-1)
    assert M.same(M.dilate(v3, f, 2)[0], np.stack([v2, 2.0 * v2, -v2], axis=-1))
    assert not M.dilate(np.zeros((4, 3)), np.zeros((4, 3), dtype=bool), 3)[1].any()


OBJ = """# a quad and a pentagon
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vn 0 0 1
vt 0.0 0.0
vt 0.5 0.0 0.0
vt 0.5 0.5
vt 0.0 0.5
f 1/1/1 2/2/1 3/3/1 4/4/1
v 2 0 0
v 3 0 0
v 3.5 1 0
v 2.5 2 0
v 1.5 1 0
vt 0.6 0.1
vt 0.9 0.1
vt 1.0 0.5
vt 0.75 0.9
vt 0.5 0.5
f -5/-5/-1 -4/-4/-1 -3/-3/-1 -2/-2/-1 -1/-1/-1
f 1/9 2/8 3/7
"""


def test_load_obj_texcoords_follows_load_objs_fan_and_index_rules():
    uv = lightmap.load_obj_texcoords(io.StringIO(OBJ))
    mesh = rpt_amd.load_obj(io.StringIO(OBJ))
    vt = [(0.0, 0.0), (0.5, 0.0), (0.5, 0.5), (0.0, 0.5), (0.6, 0.1), (0.9, 0.1), (1.0, 0.5), (0.75, 0.9), (0.5, 0.5)]
    want = [(vt[0], vt[1], vt[2]), (vt[0], vt[2], vt[3]),                              # the quad's fan
            (vt[4], vt[5], vt[6]), (vt[4], vt[6], vt[7]), (vt[4], vt[7], vt[8]),       # the pentagon's, by negative indices
            (vt[8], vt[7], vt[6])]                                                      # v/vt without a normal
    assert uv.shape == (6, 3, 2) and uv.dtype == np.float64 and (uv == np.array(want)).all()
    assert len(mesh.triangles) == len(uv)                                               # one row per triangle load_obj makes
    assert (mesh.triangles[2, :9] == np.array([2, 0, 0, 3, 0, 0, 3.5, 1, 0], dtype=np.float64)).all()
    with pytest.raises(ValueError, match="has no vt index"):
        lightmap.load_obj_texcoords(io.StringIO(OBJ + "f 1//1 2//1 3//1\n"))
    with pytest.raises(ValueError, match="has no vt index"):
        lightmap.load_obj_texcoords(io.StringIO(OBJ + "f 1 2 3\n"))
    with pytest.raises(IndexError):
        lightmap.load_obj_texcoords(io.StringIO(OBJ + "f 1/10 2/1 3/1\n"))             # a vt that was never read
    assert lightmap.load_obj_texcoords(io.StringIO("v 0 0 0\n")).shape == (0, 3, 2)
    rgb = lightmap.to_rgb8(np.array([[[0.0, np.pi, 4.0 * np.pi]]]), (1.0, 1.0, 0.25), 0.0)
    assert rgb.shape == (1, 1, 3) and rgb.dtype == np.uint8 and rgb[0, 0, 0] == 0 and rgb[0, 0, 1] == 255 and rgb[0, 0, 2] == 255
    assert (lightmap.to_rgb8(np.full((2, 2, 3), np.pi), (1.0, 1.0, 1.0), -1.0) == rpt_amd.color_bytes(np.full((2, 2, 3), 0.5))).all()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lightmap_plan_" + request.param) / "lightmap_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "lightmap_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["clamp", "cover", "pieces", "slivers"])
def test_lightmap_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
