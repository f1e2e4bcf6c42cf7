"""rptgpu_lookup_lightmap without a GPU: the two symbols, detected the way a binding detects them, and the three structs' layouts
against the header; every refusal that comes before the device — through the host and the device entry point, with its code,
its detail and the arrays untouched —; what GpuScene.lookup_lightmap lowers its arguments to; the numpy restatement of the
header's rule (tests/lightmap_lookup_model.py) against closed forms; the sizing header (rpt_amd/csrc/lightmap_lookup_plan.h) in
a stand-alone program (tests/cpp/lightmap_lookup_plan_check.cpp), plain and under AddressSanitizer + UBSan; and the round
trip of tests/test_gpu_lightmap_lookup.py run through the oracle and the models, which shows that its rays stay within the
cap the issue sets: at most 10 % of the floor's hits have a tap that is not valid."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi, lightmap

import lightmap_lookup_model as L
import lightmap_model
import surface_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_lookup_lightmap", "rptgpu_lookup_lightmap_device")
BINDING_FIELDS = ("struct_size", "object", "n_tris", "width", "height", "components", "reserved", "uvs", "map", "valid")
QUERY_FIELDS = ("struct_size", "channels", "filter", "fallback", "precision_mode", "flags")
ARRAY_FIELDS = ("struct_size", "reserved", "t", "object", "binding", "covered", "uv", "value")
BITS = (("t", _abi.RPT_LOOKUP_T), ("object", _abi.RPT_LOOKUP_OBJECT), ("binding", _abi.RPT_LOOKUP_BINDING),
        ("covered", _abi.RPT_LOOKUP_COVERED), ("uv", _abi.RPT_LOOKUP_UV), ("value", _abi.RPT_LOOKUP_VALUE))


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and _abi.lightmap_lookup_supported(lib)
    assert tuple(s[0] for s in _abi.LIGHTMAP_LOOKUP_SYMBOLS)[:2] == NAMES and not set(NAMES) & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7

    class Older:  # a library without the two: still ABI 7, and the detection says so
        rptgpu_hit_surface = None
    assert not _abi.lightmap_lookup_supported(Older())
    structs = (("RptLightmapBinding", BINDING_FIELDS), ("RptLookupQuery", QUERY_FIELDS), ("RptLookupArrays", ARRAY_FIELDS))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){' + \
          "".join('printf("%%zu ", sizeof(%s));' % s + "".join('printf("%%zu ", offsetof(%s, %s));' % (s, f) for f in fs)
                  for s, fs in structs) + \
          'printf("%u %u %u %u %u %u %u %u", RPT_LOOKUP_T, RPT_LOOKUP_OBJECT, RPT_LOOKUP_BINDING, RPT_LOOKUP_COVERED, RPT_LOOKUP_UV, ' \
          'RPT_LOOKUP_VALUE, RPT_LOOKUP_NEAREST, RPT_LOOKUP_BILINEAR);printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = {"RptLightmapBinding": (56, [0, 4, 8, 12, 16, 20, 24, 32, 40, 48]), "RptLookupQuery": (48, [0, 4, 8, 16, 40, 44]),
            "RptLookupArrays": (56, [0, 4, 8, 16, 24, 32, 40, 48])}
    at = 0
    for name, fields in structs:
        cls = getattr(_abi, name)
        size, offsets = nums[at], nums[at + 1:at + 1 + len(fields)]
        at += 1 + len(fields)
        assert C.sizeof(cls) == size == want[name][0]
        assert [getattr(cls, f).offset for f in fields] == offsets == want[name][1]
        assert [f for f, _ in cls._fields_] == list(fields)
    assert nums[at:] == [b for _, b in BITS] + [0, 1] == [1, 2, 4, 8, 16, 32, 0, 1] and _abi.RPT_LOOKUP_ALL == 63
    assert (_abi.RPT_LOOKUP_NEAREST, _abi.RPT_LOOKUP_BILINEAR) == (0, 1)
    assert rpt_amd.RPT_LOOKUP_VALUE == 32 and rpt_amd.lightmap.Binding is lightmap.Binding


def query(**kw):
    q = _abi.RptLookupQuery()
    q.struct_size, q.channels, q.filter = C.sizeof(_abi.RptLookupQuery), _abi.RPT_LOOKUP_ALL, _abi.RPT_LOOKUP_BILINEAR
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a lightmap lookup runs the closest-hit "
              "query, a resolve walk and a fetch only").encode()
MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
Q_SIZE = b"RptLookupQuery: struct_size is not sizeof(RptLookupQuery)"
A_SIZE = b"RptLookupArrays: struct_size is not sizeof(RptLookupArrays)"
UNKNOWN = b"RptLookupQuery: channels names an unknown RPT_LOOKUP_* bit"
# (what is passed: q, the arrays struct's fields, which arrays are NULL, n, the bindings' fields) -> the detail.  In the order
# the header gives: the query, the arrays, the bindings, the handle
REFUSALS = [
    ("no query", dict(q=None), b"null RptLookupQuery"),
    ("query size 0", dict(q=query(struct_size=0)), Q_SIZE),
    ("query size 40", dict(q=query(struct_size=40)), Q_SIZE),
    ("query size 56", dict(q=query(struct_size=56)), Q_SIZE),
    ("no channel", dict(q=query(channels=0)), b"RptLookupQuery: channels == 0 (name at least one RPT_LOOKUP_* channel)"),
    ("unknown bit", dict(q=query(channels=64 | _abi.RPT_LOOKUP_T)), UNKNOWN),
    ("high bit", dict(q=query(channels=1 << 31)), UNKNOWN),
    ("filter 2", dict(q=query(filter=2)), b"RptLookupQuery: filter is neither RPT_LOOKUP_NEAREST nor RPT_LOOKUP_BILINEAR"),
    ("mode", dict(q=query(precision_mode=1)), MODE),
    ("persistent", dict(q=query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("the query before the arrays", dict(q=query(filter=7), arrays=None), b"RptLookupQuery: filter is neither RPT_LOOKUP_NEAREST nor RPT_LOOKUP_BILINEAR"),
    ("no arrays struct", dict(arrays=None), b"null RptLookupArrays"),
    ("arrays size 0", dict(a_size=0), A_SIZE),
    ("arrays size 48", dict(a_size=48), A_SIZE),
    ("arrays size 64", dict(a_size=64), A_SIZE),
    ("reserved", dict(reserved=1), b"RptLookupArrays: reserved != 0"),
    ("t", dict(t=False), b"RptLookupArrays: RPT_LOOKUP_T is named but t is NULL"),
    ("object", dict(object=False), b"RptLookupArrays: RPT_LOOKUP_OBJECT is named but object is NULL"),
    ("binding", dict(binding=False), b"RptLookupArrays: RPT_LOOKUP_BINDING is named but binding is NULL"),
    ("covered", dict(covered=False), b"RptLookupArrays: RPT_LOOKUP_COVERED is named but covered is NULL"),
    ("uv", dict(uv=False), b"RptLookupArrays: RPT_LOOKUP_UV is named but uv is NULL"),
    ("value", dict(value=False), b"RptLookupArrays: RPT_LOOKUP_VALUE is named but value is NULL"),
    ("origins", dict(origins=False), b"null argument"),
    ("dirs", dict(dirs=False), b"null argument"),
    ("the arrays before the bindings", dict(value=False, b1=dict(width=0)), b"RptLookupArrays: RPT_LOOKUP_VALUE is named but value is NULL"),
    ("null bindings", dict(bindings=None), b"null bindings with n_bindings > 0"),
    ("binding size", dict(b1=dict(struct_size=48)), b"binding 1: struct_size is not sizeof(RptLightmapBinding)"),
    ("binding reserved", dict(b0=dict(reserved=3)), b"binding 0: reserved != 0"),
    ("width 0", dict(b1=dict(width=0)), b"binding 1: width or height is 0"),
    ("height 0", dict(b0=dict(height=0)), b"binding 0: width or height is 0"),
    ("components 2", dict(b0=dict(components=2)), b"binding 0: components is neither 1 nor 3"),
    ("components 0", dict(b1=dict(components=0)), b"binding 1: components is neither 1 nor 3"),
    ("null uvs", dict(b1=dict(uvs=None)), b"binding 1: uvs is NULL"),
    ("null map", dict(b0=dict(map=None)), b"binding 0: map is NULL"),
    ("one object twice", dict(b1=dict(object=3)), b"two bindings name object 3"),
    ("the bindings before the handle", dict(b0=dict(components=5)), b"binding 0: components is neither 1 nor 3"),
    ("handle", dict(), b"null handle"),
    ("handle, a null valid map is legal", dict(b0=dict(valid=None)), b"null handle"),
    ("handle, one channel and only its array", dict(q=query(channels=_abi.RPT_LOOKUP_VALUE), t=False, object=False, binding=False,
                                                     covered=False, uv=False), b"null handle"),
    ("handle, no rays", dict(n=0, origins=False, dirs=False), b"null handle"),
    ("handle, no bindings", dict(n_bindings=0, bindings=None), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_lookup_lightmap_refuses_before_the_device(row, device):
    """... so every refusal that needs no scene is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    o, d = np.full(12, 7.0), np.full(12, 7.0)
    outs = {"t": np.full(4, 7.0), "object": np.full(4, 7, dtype=np.int32), "binding": np.full(4, 7, dtype=np.int32),
            "covered": np.full(4, 7, dtype=np.uint8), "uv": np.full(8, 7.0), "value": np.full(12, 7.0)}
    ins = {"uvs": np.full(12, 7.0), "map": np.full(6, 7.0), "valid": np.full(6, 7, dtype=np.uint8)}
    q = kw.get("q", query())
    a = _abi.RptLookupArrays()
    a.struct_size, a.reserved = kw.get("a_size", C.sizeof(_abi.RptLookupArrays)), kw.get("reserved", 0)
    types = dict(_abi.RptLookupArrays._fields_)
    for name, arr in outs.items():  # (device: pointers that are never followed — every row is refused before the device)
        if kw.get(name, True):
            setattr(a, name, arr.ctypes.data_as(types[name]))
    recs = (_abi.RptLightmapBinding * 2)()
    btypes = dict(_abi.RptLightmapBinding._fields_)
    for k, r in enumerate(recs):
        fields = dict(struct_size=C.sizeof(r), object=3 + 2 * k, n_tris=2, width=3, height=2, components=1, reserved=0,
                      uvs=ins["uvs"], map=ins["map"], valid=ins["valid"])
        fields.update(kw.get("b%d" % k, {}))
        for name, v in fields.items():
            if isinstance(v, np.ndarray):
                v = v.ctypes.data_as(btypes[name])
            setattr(r, name, v)
    bp = recs if kw.get("bindings", True) is not None else None
    ap = C.byref(a) if kw.get("arrays", True) is not None else None
    qp = C.byref(q) if q is not None else None
    use = lambda name, arr: arr if kw.get(name, True) else None
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    if device:
        p = lambda arr: C.c_void_p(arr.ctypes.data) if arr is not None else None
        rc = lib.rptgpu_lookup_lightmap_device(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)),
                                               kw.get("n_bindings", 2), bp, qp, ap, None)
    else:
        p = lambda arr: arr.ctypes.data_as(PD) if arr is not None else None
        rc = lib.rptgpu_lookup_lightmap(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), kw.get("n_bindings", 2),
                                        bp, qp, ap)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and all((arr == 7).all() for arr in list(outs.values()) + list(ins.values()))


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
    o = np.arange(12.0).reshape(4, 3)
    d = o[::-1] * 0.5            # not contiguous: the call sees a contiguous copy
    uvs = np.arange(12.0).reshape(2, 3, 2) / 12.0
    rgb, grey = np.arange(90.0).reshape(5, 6, 3), np.arange(6.0).reshape(2, 3)
    valid = np.arange(30).reshape(5, 6) % 2 == 0
    b = [lightmap.Binding(4, uvs, rgb, valid), lightmap.Binding(1, uvs[:1], grey)]
    out = g.lookup_lightmap(o, d, b, filter="nearest", fallback=(1.0, 2.0, 3.0), flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, po, pd, nb, recs, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert name == "rptgpu_lookup_lightmap" and h is g.handle and n == 4 and nb == 2
    assert (q.struct_size, q.channels, q.filter, tuple(q.fallback), q.precision_mode, q.flags) == \
        (48, 63, _abi.RPT_LOOKUP_NEAREST, (1.0, 2.0, 3.0), _abi.RPT_PRECISION_F64_STRICT, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert (a.struct_size, a.reserved) == (56, 0)
    floats = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
    address = lambda p: C.cast(p, C.c_void_p).value
    assert (floats(po, 12) == o.ravel()).all() and (floats(pd, 12) == d.ravel()).all()
    r0, r1 = recs[0], recs[1]
    assert (r0.struct_size, r0.object, r0.n_tris, r0.width, r0.height, r0.components, r0.reserved) == (56, 4, 2, 6, 5, 3, 0)
    assert (r1.struct_size, r1.object, r1.n_tris, r1.width, r1.height, r1.components, r1.reserved) == (56, 1, 1, 3, 2, 1, 0)
    assert address(r0.uvs) == uvs.ctypes.data and address(r0.map) == rgb.ctypes.data and not r1.valid
    assert (np.ctypeslib.as_array(r0.valid, shape=(30,)) == valid.ravel()).all()  # bools as bytes
    assert (floats(r1.map, 6) == grey.ravel()).all()
    assert sorted(out) == ["binding", "covered", "object", "t", "uv", "value"]
    assert out["uv"].shape == (4, 2) and out["value"].shape == (4, 3) and out["covered"].dtype == np.uint8
    assert out["binding"].dtype == np.int32 and out["t"].shape == (4,)
    for k, v in out.items():
        assert address(getattr(a, k)) == v.ctypes.data
    # two channels, no bindings: the other pointers stay NULL, and the default filter is bilinear
    out = g.lookup_lightmap(o, d, [], channels=_abi.RPT_LOOKUP_VALUE | _abi.RPT_LOOKUP_COVERED)
    name, (h, n, po, pd, nb, recs, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert sorted(out) == ["covered", "value"] and (q.channels, q.filter, q.flags, nb, recs) == (40, _abi.RPT_LOOKUP_BILINEAR, 0, 0, None)
    assert not a.t and not a.object and not a.uv and address(a.value) == out["value"].ctypes.data
    assert not g.lib.calls
    g.handle = None


def test_the_python_call_checks_its_shapes_and_dtypes():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    z, uvs, tex = np.zeros((3, 3)), np.zeros((2, 3, 2)), np.zeros((4, 4, 3))
    B = lightmap.Binding
    for call, word in ((lambda: g.lookup_lightmap(np.zeros((3, 2)), z, []), r"origins must be an \(n, 3\) float64 array"),
                       (lambda: g.lookup_lightmap(z, np.zeros((2, 3)), []), "3 origins for 2 directions"),
                       (lambda: g.lookup_lightmap(z, z, [], filter="trilinear"), 'filter must be "nearest" or "bilinear"'),
                       (lambda: g.lookup_lightmap(z, z, [B(0, np.zeros((2, 3, 3)), tex)]), r"bindings\[0\].uvs must be an \(n, 3, 2\)"),
                       (lambda: g.lookup_lightmap(z, z, [B(0, uvs, np.zeros((4, 4, 2)))]), r"bindings\[0\].map must be an \(H, W\) or"),
                       (lambda: g.lookup_lightmap(z, z, [B(0, uvs, tex.astype(np.float32))]), r"bindings\[0\].map must be a C-contiguous"),
                       (lambda: g.lookup_lightmap(z, z, [B(0, uvs, tex), B(1, uvs, tex, np.zeros((4, 5), dtype=bool))]),
                        r"bindings\[1\].valid must be a \(4, 4\) uint8 or bool")):
        with pytest.raises(ValueError, match=word):
            call()
    for call, word in ((lambda: g.lookup_lightmap(z, z, [B(0, uvs, tex)]), "null handle"),  # well-formed arrays: the library speaks
                       (lambda: g.lookup_lightmap(z, z, [], channels=0), "channels == 0"),
                       (lambda: g.lookup_lightmap(z, z, [B(2, uvs, tex), B(2, uvs, tex)]), "two bindings name object 2")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call()
        assert e.value.code == E and word in str(e.value)
    g.handle = None


# ---- the model against closed forms
def one(tex, uv, filter, valid=None, fallback=(-1.0, -2.0, -3.0)):
    """the rule for rays that all hit triangle 0 of object 0 at its first vertex, whose uv is given per ray"""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n = len(uv)
    uvs = np.zeros((n, 3, 2))
    uvs[:, 0] = uv
    b = lightmap.Binding(0, uvs, np.asarray(tex, dtype=np.float64), valid)
    bary = np.tile(np.array([1.0, 0.0, 0.0]), (n, 1))
    return L.lookup(np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32), bary, [b], filter, fallback)


TEX35 = np.random.RandomState(35).uniform(-4.0, 4.0, (5, 3, 3))   # H = 5, W = 3


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (5, 3)], ids=["1x1", "2x1", "1x2", "3x5"])
def test_a_uv_at_a_texel_centre_returns_that_texels_bits(shape):
    H, W = shape
    tex = np.random.RandomState(H * 8 + W).uniform(0.5, 4.0, (H, W, 3)) * np.array([1.0, -1.0, 1e-300])
    ys, xs = np.divmod(np.arange(H * W), W)
    uv = np.stack([(xs + 0.5) / W, (ys + 0.5) / H], axis=1)
    for filter in (L.NEAREST, L.BILINEAR):
        got = one(tex, uv, filter)
        assert (got["covered"] == 1).all() and (got["binding"] == 0).all() and M.same(got["uv"], uv)
        assert M.same(got["value"], tex[ys, xs])


def test_bilinear_against_exact_arithmetic():
    """weights that are dyadic fractions and integer texels: every product and sum is exact, so the closed form is the value"""
    tex = np.arange(15.0).reshape(5, 3)                                  # components == 1: the scalar three times
    got = one(tex, [[1.0 / 3.0 + 0.25 / 3.0, 0.3 + 0.5 / 5.0]], L.BILINEAR)  # s = 0.75 (+- an ulp), t = 1.5
    fx, fy = got["uv"][0, 0] * 3.0 - 0.5, got["uv"][0, 1] * 5.0 - 0.5 - 1.0
    want = ((1 - fx) * (1 - fy) * tex[1, 0] + fx * (1 - fy) * tex[1, 1]) + (1 - fx) * fy * tex[2, 0] + fx * fy * tex[2, 1]
    assert got["covered"][0] == 1 and abs(got["value"][0, 0] - want) <= 1e-13 and M.same(got["value"][0], np.repeat(got["value"][0, 0], 3))
    exact = one(tex, [[0.5, 0.5], [0.75 / 3.0 + 0.5 / 3.0, 0.25 / 5.0 + 0.5 / 5.0]], L.BILINEAR)
    assert M.same(exact["value"][0], np.repeat(tex[2, 1], 3))
    # U * 3 - 0.5 and V * 5 - 0.5 round, so hold the second to the rule's own weights
    s, t = exact["uv"][1, 0] * 3.0 - 0.5, exact["uv"][1, 1] * 5.0 - 0.5
    fx, fy = s - np.floor(s), t - np.floor(t)
    gx, gy = 1.0 - fx, 1.0 - fy
    w = (gx * gy, fx * gy, gx * fy, fx * fy)
    want = (((w[0] * tex[0, 0] + w[1] * tex[0, 1]) + w[2] * tex[1, 0]) + w[3] * tex[1, 1]) / (((w[0] + w[1]) + w[2]) + w[3])
    assert M.same(exact["value"][1], np.repeat(want, 3))


def test_uvs_at_the_edges_outside_and_nan():
    inf, nan = float("inf"), float("nan")
    uv = [[0.0, 0.0], [1.0, 1.0], [-3.0, 0.5], [7.0, 0.5], [0.5, -1e300], [0.5, 1e300], [nan, 0.5], [0.5, nan], [inf, 0.5], [0.5, -inf]]
    for filter in (L.NEAREST, L.BILINEAR):
        got = one(TEX35, uv, filter)
        assert list(got["covered"]) == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0] and (got["binding"] == 0).all()
        assert M.same(got["uv"], np.array(uv))                        # UV is what was computed, covered or not
        assert M.same(got["value"][6:], np.tile([-1.0, -2.0, -3.0], (4, 1)))
        # clamp to edge: the corners and the middles of the edges, bit for bit under NEAREST
        corners = [TEX35[0, 0], TEX35[4, 2], TEX35[2, 0], TEX35[2, 2], TEX35[0, 1], TEX35[4, 1]]
        if filter == L.NEAREST:
            assert M.same(got["value"][:6], np.array(corners))
        else:
            assert np.abs(got["value"][:6] - np.array(corners)).max() <= 1e-14
    # a map of one texel: whatever the uv, that texel
    lone = one(TEX35[:1, :1], uv[:6], L.BILINEAR)
    assert (lone["covered"] == 1).all() and np.abs(lone["value"] - TEX35[0, 0]).max() <= 1e-15


@pytest.mark.parametrize("mask", range(16))
def test_zero_to_four_valid_taps(mask):
    """uv between the four texels of a 2 x 2 map: the valid taps' weights renormalised; none valid: the fallback"""
    tex = np.array([[[1.0, 10.0, 100.0], [2.0, 20.0, 200.0]], [[4.0, 40.0, 400.0], [8.0, 80.0, 800.0]]])
    valid = np.array([[mask & 1, mask >> 1 & 1], [mask >> 2 & 1, mask >> 3 & 1]], dtype=np.uint8)
    got = one(tex, [[0.5 + 0.125, 0.5 - 0.0625]], L.BILINEAR, valid)   # fx = 0.75, fy = 0.375: exact
    w = np.array([[0.25 * 0.625, 0.75 * 0.625], [0.25 * 0.375, 0.75 * 0.375]]) * valid
    assert L.valid_taps(lightmap.Binding(0, None, tex, valid), got["uv"])[0] == bin(mask).count("1")
    if not mask:
        assert got["covered"][0] == 0 and M.same(got["value"][0], np.array([-1.0, -2.0, -3.0]))
        return
    want = (w[..., None] * tex).sum(axis=(0, 1)) / w.sum()
    assert got["covered"][0] == 1 and np.abs(got["value"][0] - want).max() <= 1e-13 * 800
    if bin(mask).count("1") == 1:  # one valid tap: w * m / w
        y, x = np.argwhere(valid)[0]
        assert np.abs(got["value"][0] - tex[y, x]).max() <= 1e-13 * 800
    near = one(tex, [[0.5 + 0.125, 0.5 - 0.0625]], L.NEAREST, valid)  # texel (1, 0)
    assert near["covered"][0] == (mask >> 1 & 1) and M.same(near["value"][0], tex[0, 1] if mask >> 1 & 1 else np.array([-1.0, -2.0, -3.0]))


def test_a_nan_texel_reaches_every_value_whose_taps_include_it():
    """a tap of weight +0.0 still enters the sum: 0.0 * NaN is NaN, valid or not — and a texel two away does not"""
    tex = np.ones((1, 4, 3))
    tex[0, 1] = np.nan
    valid = np.array([[1, 0, 1, 1]], dtype=np.uint8)
    got = one(tex, [[0.5 / 4, 0.5], [1.0 / 4, 0.5], [2.9 / 4, 0.5], [3.5 / 4, 0.5]], L.BILINEAR, valid)
    assert (got["covered"] == 1).all()
    assert np.isnan(got["value"][:2]).all() and M.same(got["value"][2:], np.ones((2, 3)))
    assert M.same(one(tex, [[0.5 / 4, 0.5]], L.NEAREST, valid)["value"], np.ones((1, 3)))


def test_unbound_rays_and_two_bindings():
    rs = np.random.RandomState(8)
    uvs = rs.uniform(0.0, 1.0, (3, 3, 2))
    b = [lightmap.Binding(5, uvs, rs.uniform(0, 1, (4, 4, 3))), lightmap.Binding(2, uvs[:2], rs.uniform(0, 1, (2, 3)))]
    obj = np.array([5, 2, 2, -1, 7, 5], dtype=np.int32)
    prim = np.array([2, 1, -1, -1, 0, 0], dtype=np.int32)      # object 2 once without a triangle: a group's sphere, say
    bary = rs.dirichlet((1.0, 1.0, 1.0), 6)
    got = L.lookup(obj, prim, bary, b, L.BILINEAR, (9.0, 8.0, 7.0))
    assert list(got["binding"]) == [0, 1, -1, -1, -1, 0] and list(got["covered"]) == [1, 1, 0, 0, 0, 1]
    assert M.same(got["uv"][2:5], np.zeros((3, 2))) and M.same(got["value"][2:5], np.tile([9.0, 8.0, 7.0], (3, 1)))
    t = uvs[2]
    assert M.same(got["uv"][0], (bary[0, 0] * t[0] + bary[0, 1] * t[1]) + bary[0, 2] * t[2])
    assert M.same(got["value"][1], np.repeat(got["value"][1, 0], 3))
    none = L.lookup(obj, prim, bary, [], L.NEAREST, (9.0, 8.0, 7.0))
    assert (none["binding"] == -1).all() and not none["covered"].any()


# ---- the sizing header
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lightmap_lookup_plan_" + request.param) / "lightmap_lookup_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "lightmap_lookup_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover"])
def test_lightmap_lookup_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr


# ---- the round trip, through the oracle and the models
def test_the_round_trips_rays_stay_within_the_cap():
    """tests/test_gpu_lightmap_lookup.py bakes POSITION | OWNER over cornell's floor and looks the positions up again.  Here the
    same through the oracle's hits, surface_model's barycentrics and lightmap_model's bake: at most 10 % of the floor's hits
    have a tap that is not valid, and where all four are, the bilinear value is the hit point to 1e-9 of the floor's extent"""
    from oracle import oracle_ffi
    import small_scenes
    ob, rows, uvs, o, d, extent = L.round_trip_case()
    t, nrm, obj = oracle_ffi.OracleScene(small_scenes.small("cornell")[0]).closest_hit(o, d)
    on = np.flatnonzero(obj == ob)
    assert len(on) >= 100  # (the two boxes stand on the floor and take many of the rays: enough hits for a proportion)
    prim = np.full(len(o), -1, dtype=np.int32)
    bary = np.zeros((len(o), 3))
    for k in range(len(rows)):  # the triangle whose record is the oracle's
        time, uvw, _ = M.tri_records(np.repeat(rows[k:k + 1], len(on), 0), o[on], d[on])
        hit = (M.bits(time) == M.bits(t[on])) & (uvw >= 0.0).all(axis=1) & (prim[on] < 0)
        prim[on[hit]], bary[on[hit]] = k, uvw[hit]
    assert (prim[on] >= 0).all()
    size = L.ROUND_TRIP_SIZE
    baked = lightmap_model.raw(rows[:, :9].reshape(-1, 3, 3), None, uvs, size, size, 0.0)
    b = lightmap.Binding(ob, uvs, baked["position"], baked["owner"] >= 0)
    got = L.lookup(obj, prim, bary, [b], L.BILINEAR)
    full = L.valid_taps(b, got["uv"][on]) == 4
    assert (got["binding"][on] == 0).all() and full.mean() >= 0.9
    point = o[on] + t[on, None] * d[on]
    assert np.abs(got["value"][on][full] - point[full]).max() <= 1e-9 * extent


# ---- rptgpu_render_views_lightmapped without a GPU
VIEW_NAMES = ("rptgpu_render_views_lightmapped", "rptgpu_render_views_lightmapped_device")


def test_the_views_forms_symbols_and_struct_layout(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in VIEW_NAMES)
    assert tuple(s[0] for s in _abi.LIGHTMAP_LOOKUP_SYMBOLS) == NAMES + VIEW_NAMES
    fields = ("struct_size", "filter", "unbound_irradiance")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptViewsLightmapQuery));' + \
          "".join('printf(" %%zu", offsetof(RptViewsLightmapQuery, %s));' % f for f in fields) + 'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    cls = _abi.RptViewsLightmapQuery
    assert C.sizeof(cls) == nums[0] == 32 and [getattr(cls, f).offset for f in fields] == nums[1:] == [0, 4, 8]
    assert [f for f, _ in cls._fields_] == list(fields)


def view_query(**kw):
    q = _abi.RptViewQuery()
    q.struct_size, q.width, q.height, q.iterations = C.sizeof(q), 4, 3, 1
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def views_query(**kw):
    q = _abi.RptViewsLightmapQuery()
    q.struct_size, q.filter = C.sizeof(q), _abi.RPT_LOOKUP_BILINEAR
    for k, v in kw.items():
        setattr(q, k, v)
    return q


VQ_SIZE = b"RptViewsLightmapQuery: struct_size is not sizeof(RptViewsLightmapQuery)"
# rptgpu_render_views' refusals of the RptViewQuery first, then this call's query, out and the views, each view, the bindings, the handle
VIEW_REFUSALS = [
    ("no view query", dict(qv=None), b"null RptViewQuery"),
    ("view query size", dict(qv=view_query(struct_size=8)), b"RptViewQuery: struct_size is not sizeof(RptViewQuery)"),
    ("zero width", dict(qv=view_query(width=0)), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("zero iterations", dict(qv=view_query(iterations=0)), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("mode", dict(qv=view_query(precision_mode=1)), MODE),
    ("persistent", dict(qv=view_query(flags=_abi.RPT_FLAG_PERSISTENT)), b"RptViewQuery: RPT_FLAG_PERSISTENT"),
    ("views persistent", dict(qv=view_query(flags=_abi.RPT_FLAG_VIEWS_PERSISTENT)), b"RptViewQuery: RPT_FLAG_VIEWS_PERSISTENT"),
    ("the view query before this call's", dict(qv=view_query(height=0), q=None), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("no query", dict(q=None), b"null RptViewsLightmapQuery"),
    ("query size 0", dict(q=views_query(struct_size=0)), VQ_SIZE),
    ("query size 40", dict(q=views_query(struct_size=40)), VQ_SIZE),
    ("filter 2", dict(q=views_query(filter=2)), b"RptViewsLightmapQuery: filter is neither RPT_LOOKUP_NEAREST nor RPT_LOOKUP_BILINEAR"),
    ("no out", dict(out=False), b"null out"),
    ("no views", dict(views=False), b"null argument"),
    ("too many views", dict(n_views=1 << 60), b"n_views * width * height does not fit"),
    ("unknown projection", dict(projection=9), b"RptView: unknown projection"),
    ("ortho scale", dict(projection=_abi.RPT_VIEW_ORTHOGRAPHIC), b"RptView: RPT_VIEW_ORTHOGRAPHIC needs a finite ortho_scale > 0"),
    ("the views before the bindings", dict(projection=9, b1=dict(width=0)), b"RptView: unknown projection"),
    ("null bindings", dict(bindings=None), b"null bindings with n_bindings > 0"),
    ("binding size", dict(b1=dict(struct_size=48)), b"binding 1: struct_size is not sizeof(RptLightmapBinding)"),
    ("width 0", dict(b1=dict(width=0)), b"binding 1: width or height is 0"),
    ("components 2", dict(b0=dict(components=2)), b"binding 0: components is neither 1 nor 3"),
    ("null uvs", dict(b1=dict(uvs=None)), b"binding 1: uvs is NULL"),
    ("null map", dict(b0=dict(map=None)), b"binding 0: map is NULL"),
    ("one object twice", dict(b1=dict(object=3)), b"two bindings name object 3"),
    ("handle", dict(), b"null handle"),
    ("handle, no views", dict(n_views=0, views=False), b"null handle"),
    ("handle, no bindings", dict(n_bindings=0, bindings=None), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(VIEW_REFUSALS)), ids=[r[0] for r in VIEW_REFUSALS])
def test_render_views_lightmapped_refuses_before_the_device(row, device):
    _, kw, detail = VIEW_REFUSALS[row]
    lib = _abi.load_library()
    out = np.full(2 * 3 * 4 * 3, 7.0)
    ins = {"uvs": np.full(12, 7.0), "map": np.full(6, 7.0), "valid": np.full(6, 7, dtype=np.uint8)}
    views = (_abi.RptView * 2)()
    for v in views:
        v.camera.direction[2], v.camera.up[1], v.camera.fov = -1.0, 1.0, 0.7
    views[1].projection = kw.get("projection", 0)
    recs = (_abi.RptLightmapBinding * 2)()
    btypes = dict(_abi.RptLightmapBinding._fields_)
    for k, r in enumerate(recs):
        fields = dict(struct_size=C.sizeof(r), object=3 + 2 * k, n_tris=2, width=3, height=2, components=1, reserved=0,
                      uvs=ins["uvs"], map=ins["map"], valid=ins["valid"])
        fields.update(kw.get("b%d" % k, {}))
        for name, val in fields.items():
            setattr(r, name, val.ctypes.data_as(btypes[name]) if isinstance(val, np.ndarray) else val)
    qv, q = kw.get("qv", view_query()), kw.get("q", views_query())
    args = [None, kw.get("n_views", 2), views if kw.get("views", True) else None, C.byref(qv) if qv is not None else None,
            kw.get("n_bindings", 2), recs if kw.get("bindings", True) is not None else None, C.byref(q) if q is not None else None]
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    if device:
        rc = lib.rptgpu_render_views_lightmapped_device(*args, C.c_void_p(out.ctypes.data) if kw.get("out", True) else None, None)
    else:
        rc = lib.rptgpu_render_views_lightmapped(*args, out.ctypes.data_as(PD) if kw.get("out", True) else None)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None).startswith(detail)
    assert (out == 7).all() and all((arr == 7).all() for arr in ins.values())


def test_what_render_views_lightmapped_lowers_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    cam = rpt_amd.Camera.look_at((0.0, 1.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.7)
    views = [cam, rpt_amd.View.orthographic(cam, 2.0), rpt_amd.View.panorama((0.0, 1.0, 0.0))]
    uvs, grey = np.arange(12.0).reshape(2, 3, 2) / 12.0, np.arange(6.0).reshape(2, 3)
    out = g.render_views_lightmapped(views, 8, 6, [lightmap.Binding(4, uvs, grey)], samples=3, seed=11, seed_stride=2,
                                     sample_index_base=5, exposure_value=1.5, filter="nearest", unbound_irradiance=(1.0, 2.0, 3.0),
                                     flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, arr, qv, nb, recs, q, po) = g.lib.calls.pop()
    qv, q = qv._obj, q._obj
    assert name == "rptgpu_render_views_lightmapped" and h is g.handle and n == 3 and nb == 1 and not g.lib.calls
    assert (qv.width, qv.height, qv.iterations, qv.seed, qv.seed_stride, qv.sample_index_base, qv.exposure_value, qv.flags) == \
        (8, 6, 3, 11, 2, 5, 1.5, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert (q.struct_size, q.filter, tuple(q.unbound_irradiance)) == (32, _abi.RPT_LOOKUP_NEAREST, (1.0, 2.0, 3.0))
    assert [arr[k].projection for k in range(3)] == [_abi.RPT_VIEW_PERSPECTIVE, _abi.RPT_VIEW_ORTHOGRAPHIC, _abi.RPT_VIEW_PANORAMA]
    assert (recs[0].object, recs[0].n_tris, recs[0].width, recs[0].height, recs[0].components) == (4, 2, 3, 2, 1)
    assert out.shape == (3, 6, 8, 3) and out.dtype == np.float64 and C.cast(po, C.c_void_p).value == out.ctypes.data
    with pytest.raises(ValueError, match='filter must be "nearest" or "bilinear"'):
        g.render_views_lightmapped(views, 8, 6, [], seed=1, filter="cubic")
    g.handle = None


def test_the_shading_and_the_fold_against_closed_forms():
    """albedo / pi * I with I = pi and no emission is the albedo; an emitter adds emittance * color; a miss is the environment;
    a hit that is not covered takes unbound_irradiance; the fold is the mean in sample order times 2^EV — and the product with the
    albedo taken after the sample sum is something else when the samples of a pixel see different albedos"""
    hit = np.array([True, True, False, True])
    albedo = np.array([[0.5, 0.25, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5]])
    env = np.tile([9.0, 8.0, 7.0], (4, 1))
    emit = np.array([0.0, 2.0, 0.0, 0.0])
    covered = np.array([1, 1, 0, 0], dtype=np.uint8)
    value = np.full((4, 3), L.PI)
    one = L.shade(hit, env, albedo, emit, covered, value, (2.0 * L.PI, 0.0, L.PI))
    assert M.same(one[0], albedo[0] / L.PI * L.PI) and np.abs(one[0] - albedo[0]).max() <= 1e-15
    assert M.same(one[1], 2.0 * albedo[1] + albedo[1] / L.PI * L.PI) and M.same(one[2], env[2])
    assert np.abs(one[3] - np.array([1.0, 0.0, 0.5])).max() <= 1e-15
    two = L.shade(hit, env, albedo[::-1], emit, covered, 3.0 * value, (0.0, 0.0, 0.0))
    assert M.same(L.fold([one]), one) and M.same(L.fold([one, two], 1.0), (np.zeros_like(one) + one + two) / 2.0 * 2.0)
    assert M.same(L.fold([one, two, one], -1.0), ((one + two) + one) / 3.0 * 0.5)
    after = albedo / L.PI * ((value + 3.0 * value) / 2.0)          # mutant (d) for the pixels without emission
    assert np.abs(L.fold([one, two])[0] - after[0]).max() > 0.1
