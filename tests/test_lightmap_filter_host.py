"""rptgpu_filter_lightmap without a GPU: the two symbols, detected the way a binding detects them, and both structs' layouts
against the header; every refusal that comes before the device — through the host and the device entry point, with its code,
its detail and the arrays untouched —; what GpuScene.filter_lightmap lowers its arguments to; the sizing header
(rpt_amd/csrc/lightmap_filter_plan.h) in a stand-alone program (tests/cpp/lightmap_filter_plan_check.cpp), plain and under
AddressSanitizer + UBSan; rpt_amd.lightmap's texel_extent and batch_variance on closed forms; the YARDSTICK of
tests/test_gpu_lightmap_filter.py, tests/lightmap_filter_model.py, by hand on small maps; and the quality condition of the
filter on one synthetic map of two charts."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi, lightmap

import lightmap_filter_model as F
import lightmap_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
NAMES = ("rptgpu_filter_lightmap", "rptgpu_filter_lightmap_device")
FILTER_FIELDS = ("struct_size", "width", "height", "words", "levels", "dilate", "sigma_normal", "sigma_plane", "sigma_distance",
                 "sigma_color")
ARRAY_FIELDS = ("struct_size", "reserved", "owner", "position", "normal", "values", "variance", "out", "out_variance")


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and _abi.lightmap_filter_supported(lib)
    assert tuple(s[0] for s in _abi.LIGHTMAP_FILTER_SYMBOLS) == NAMES and not set(NAMES) & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7

    class Older:  # a library without the two: still ABI 7, and the detection says so
        rptgpu_bake_lightmap = None
    assert not _abi.lightmap_filter_supported(Older())
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptLightmapFilter));' + \
          "".join('printf(" %%zu", offsetof(RptLightmapFilter, %s));' % f for f in FILTER_FIELDS) + \
          'printf(" %zu", sizeof(RptLightmapFilterArrays));' + \
          "".join('printf(" %%zu", offsetof(RptLightmapFilterArrays, %s));' % f for f in ARRAY_FIELDS) + \
          'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    f, a = nums[:11], nums[11:]
    assert C.sizeof(_abi.RptLightmapFilter) == f[0] == 56
    assert [getattr(_abi.RptLightmapFilter, n).offset for n in FILTER_FIELDS] == f[1:] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48]
    assert [n for n, _ in _abi.RptLightmapFilter._fields_] == list(FILTER_FIELDS)
    assert C.sizeof(_abi.RptLightmapFilterArrays) == a[0] == 64
    assert [getattr(_abi.RptLightmapFilterArrays, n).offset for n in ARRAY_FIELDS] == a[1:] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert [n for n, _ in _abi.RptLightmapFilterArrays._fields_] == list(ARRAY_FIELDS)
    # the header is rpt_gpu.h's: alone it refuses to compile
    lone = tmp_path / "lone.c"
    lone.write_text('#include <stdint.h>\n#include "rpt_gpu_lightmap_filter.h"\nint main(void){return 0;}\n')
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-c", str(lone), "-o", str(tmp_path / "lone.o")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "include rpt_gpu.h" in r.stderr


W, H = 4, 2


def filt(**kw):
    f = _abi.RptLightmapFilter()
    f.struct_size, f.width, f.height, f.words, f.levels, f.dilate = C.sizeof(_abi.RptLightmapFilter), W, H, 3, 3, 1
    f.sigma_normal, f.sigma_plane, f.sigma_distance, f.sigma_color = 0.1, 0.05, 0.4, 2.0
    for k, v in kw.items():
        setattr(f, k, v)
    return f


NAN, INF = float("nan"), float("inf")
F_SIZE = b"RptLightmapFilter: struct_size is not sizeof(RptLightmapFilter)"
A_SIZE = b"RptLightmapFilterArrays: struct_size is not sizeof(RptLightmapFilterArrays)"
NO_SIZE = b"RptLightmapFilter: width == 0 or height == 0"
TOO_MANY = b"RptLightmapFilter: width * height > 2^32"
WORDS = b"RptLightmapFilter: words is neither 1 nor 3"
S_NORMAL = b"RptLightmapFilter: sigma_normal is not finite and > 0"
S_PLANE = b"RptLightmapFilter: sigma_plane is not finite and > 0"
S_DISTANCE = b"RptLightmapFilter: sigma_distance is not finite and > 0"
S_COLOR = b"RptLightmapFilter: sigma_color is not finite and > 0 (variance is given)"
# (what is passed: f, the arrays struct's fields, which arrays are NULL) -> the detail
REFUSALS = [
    ("no filter", dict(f=None), b"null RptLightmapFilter"),
    ("no arrays struct", dict(arrays=None), b"null RptLightmapFilterArrays"),
    ("filter size 0", dict(f=filt(struct_size=0)), F_SIZE),
    ("filter size 48", dict(f=filt(struct_size=48)), F_SIZE),
    ("filter size 64", dict(f=filt(struct_size=64)), F_SIZE),
    ("arrays size 0", dict(a_size=0), A_SIZE),
    ("arrays size 56", dict(a_size=56), A_SIZE),
    ("arrays size 72", dict(a_size=72), A_SIZE),
    ("width 0", dict(f=filt(width=0)), NO_SIZE),
    ("height 0", dict(f=filt(height=0)), NO_SIZE),
    ("2^32 + 65536 texels", dict(f=filt(width=65536, height=65537)), TOO_MANY),
    ("nearly 2^33 texels", dict(f=filt(width=0xFFFFFFFF, height=2)), TOO_MANY),
    ("words 0", dict(f=filt(words=0)), WORDS),
    ("words 2", dict(f=filt(words=2)), WORDS),
    ("words 4", dict(f=filt(words=4)), WORDS),
    ("levels 9", dict(f=filt(levels=9)), b"RptLightmapFilter: levels > 8"),
    ("sigma_normal 0", dict(f=filt(sigma_normal=0.0)), S_NORMAL),
    ("sigma_normal nan", dict(f=filt(sigma_normal=NAN)), S_NORMAL),
    ("sigma_plane negative", dict(f=filt(sigma_plane=-1.0)), S_PLANE),
    ("sigma_plane inf", dict(f=filt(sigma_plane=INF)), S_PLANE),
    ("sigma_distance 0", dict(f=filt(sigma_distance=-0.0)), S_DISTANCE),
    ("sigma_distance nan", dict(f=filt(sigma_distance=NAN)), S_DISTANCE),
    ("sigma_color 0 with a variance", dict(f=filt(sigma_color=0.0)), S_COLOR),
    ("sigma_color nan with a variance", dict(f=filt(sigma_color=NAN)), S_COLOR),
    ("sigma_color inf with a variance", dict(f=filt(sigma_color=INF)), S_COLOR),
    ("the filter before the arrays", dict(f=filt(levels=9), arrays=None), b"RptLightmapFilter: levels > 8"),
    ("the arrays before sigma_color", dict(f=filt(sigma_color=0.0), owner=False), b"RptLightmapFilterArrays: owner is NULL"),
    ("reserved", dict(reserved=1), b"RptLightmapFilterArrays: reserved != 0"),
    ("owner", dict(owner=False), b"RptLightmapFilterArrays: owner is NULL"),
    ("position", dict(position=False), b"RptLightmapFilterArrays: position is NULL"),
    ("normal", dict(normal=False), b"RptLightmapFilterArrays: normal is NULL"),
    ("values", dict(values=False), b"RptLightmapFilterArrays: values is NULL"),
    ("out", dict(out=False), b"RptLightmapFilterArrays: out is NULL"),
    ("out_variance without variance", dict(variance=False), b"RptLightmapFilterArrays: out_variance without variance"),
    ("handle", dict(), b"null handle"),
    ("handle, 2^32 texels", dict(f=filt(width=65536, height=65536)), b"null handle"),
    ("handle, no variance and a sigma_color that is not read", dict(f=filt(sigma_color=NAN), variance=False, out_variance=False),
     b"null handle"),
    ("handle, a variance and no out_variance", dict(out_variance=False), b"null handle"),
    ("handle, no level", dict(f=filt(levels=0, words=1, dilate=0xFFFFFFFF)), b"null handle"),
    ("handle, eight levels", dict(f=filt(levels=8)), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_filter_lightmap_refuses_before_the_device(row, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    n = W * H
    arrays = {"owner": np.full(n, 7, dtype=np.int32), "position": np.full(3 * n, 7.0), "normal": np.full(3 * n, 7.0),
              "values": np.full(3 * n, 7.0), "variance": np.full(n, 7.0), "out": np.full(3 * n, 7.0), "out_variance": np.full(n, 7.0)}
    f = kw.get("f", filt())
    a = _abi.RptLightmapFilterArrays()
    a.struct_size, a.reserved = kw.get("a_size", C.sizeof(_abi.RptLightmapFilterArrays)), kw.get("reserved", 0)
    types = dict(_abi.RptLightmapFilterArrays._fields_)
    for name, arr in arrays.items():  # (device: pointers that are never followed — every row is refused before the device)
        if kw.get(name, True):
            setattr(a, name, arr.ctypes.data_as(types[name]))
    ap = C.byref(a) if kw.get("arrays", True) is not None else None
    fp = C.byref(f) if f is not None else None
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    rc = lib.rptgpu_filter_lightmap_device(None, fp, ap, None) if device else lib.rptgpu_filter_lightmap(None, fp, ap)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert all((arr == 7).all() for arr in arrays.values())


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
    address = lambda p: C.cast(p, C.c_void_p).value
    owner = np.arange(15, dtype=np.int32).reshape(3, 5) - 2
    position, normal = np.arange(45, dtype=np.float64).reshape(3, 5, 3), np.ones((3, 5, 3))
    values, variance = np.arange(45, dtype=np.float64).reshape(3, 5, 3) / 8.0, np.full((3, 5), 0.5)
    out = g.filter_lightmap(values, owner, position, normal, sigma_distance=0.4, sigma_plane=0.05)
    name, (h, f, a) = g.lib.calls.pop()
    f, a = f._obj, a._obj
    assert name == "rptgpu_filter_lightmap" and h is g.handle
    assert [getattr(f, n) for n in FILTER_FIELDS] == [56, 5, 3, 3, 3, 0, 0.1, 0.05, 0.4, 2.0]   # the defaults
    assert (a.struct_size, a.reserved) == (64, 0)
    assert isinstance(out, np.ndarray) and out.shape == (3, 5, 3) and out.dtype == np.float64 and address(a.out) == out.ctypes.data
    assert address(a.owner) == owner.ctypes.data and address(a.position) == position.ctypes.data    # read where they lie
    assert address(a.normal) == normal.ctypes.data and address(a.values) == values.ctypes.data
    assert not a.variance and not a.out_variance
    # one word, a variance, every keyword
    out, out_v = g.filter_lightmap(values[..., 0].copy(), owner, position, normal, sigma_distance=0.25, sigma_plane=0.5, sigma_normal=0.75,
                                   levels=5, variance=variance, sigma_color=1.5, dilate=9)
    name, (h, f, a) = g.lib.calls.pop()
    f, a = f._obj, a._obj
    assert [getattr(f, n) for n in FILTER_FIELDS] == [56, 5, 3, 1, 5, 9, 0.75, 0.5, 0.25, 1.5]
    assert out.shape == (3, 5) and out_v.shape == (3, 5) and address(a.out) == out.ctypes.data
    assert address(a.out_variance) == out_v.ctypes.data and address(a.variance) == variance.ctypes.data
    assert not g.lib.calls
    for bad, word in ((lambda: g.filter_lightmap(values, owner.astype(np.int64), position, normal, sigma_distance=1.0, sigma_plane=1.0), "owner must be"),
                      (lambda: g.filter_lightmap(values, owner.ravel(), position, normal, sigma_distance=1.0, sigma_plane=1.0), "owner must be"),
                      (lambda: g.filter_lightmap(values, owner, position[:2], normal, sigma_distance=1.0, sigma_plane=1.0), "position must be"),
                      (lambda: g.filter_lightmap(values, owner, position, normal[:, :, :2], sigma_distance=1.0, sigma_plane=1.0), "normal must be"),
                      (lambda: g.filter_lightmap(values[:, :, :2], owner, position, normal, sigma_distance=1.0, sigma_plane=1.0), "values must be"),
                      (lambda: g.filter_lightmap(values.astype(np.float32), owner, position, normal, sigma_distance=1.0, sigma_plane=1.0), "values must be"),
                      (lambda: g.filter_lightmap(values, owner, position, normal, variance=variance[:2], sigma_distance=1.0, sigma_plane=1.0),
                       "variance must be")):
        with pytest.raises(ValueError, match=word):
            bad()
    assert not g.lib.calls

    class Older(Recorder):  # a library without the symbols
        def __getattr__(self, name):
            if name.startswith("rptgpu_filter_lightmap"):
                raise AttributeError(name)
            return Recorder.__getattr__(self, name)
    g.lib = Older()
    with pytest.raises(_abi.RptGpuError, match="this library does not export rptgpu_filter_lightmap"):
        g.filter_lightmap(values, owner, position, normal, sigma_distance=1.0, sigma_plane=1.0)
    g.handle = None


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lightmap_filter_plan_" + request.param) / "lightmap_filter_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "lightmap_filter_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["limits", "workspace", "staging", "launches"])
def test_lightmap_filter_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr


# ---- the helpers beside the call
def test_texel_extent_is_the_median_distance_between_owned_row_neighbours():
    y, x = np.mgrid[0:4, 0:6]
    position = np.stack([0.25 * x, np.zeros_like(x, dtype=np.float64), 0.5 * y], axis=-1)   # 0.25 along a row, exactly
    owner = np.zeros((4, 6), dtype=np.int32)
    assert lightmap.texel_extent(position, owner) == 0.25
    # unowned texels' positions (+0.0 in a bake) are not read: a gutter column between two charts
    owner[:, 2] = -1
    position[:, 2] = 0.0
    assert lightmap.texel_extent(position, owner) == 0.25
    # the median, not the mean: one stretched row among four
    position[0, 3:, 0] = position[0, 3:, 0] * 64.0
    assert lightmap.texel_extent(position, owner) == 0.25
    # a 3-4-5 step
    p = np.zeros((1, 2, 3))
    p[0, 1] = (3.0, 4.0, 0.0)
    assert lightmap.texel_extent(p, np.zeros((1, 2), dtype=np.int32)) == 5.0
    for lonely in (np.array([[0, -1, 0]]), np.array([[0], [0]]), np.full((2, 2), -1)):
        with pytest.raises(ValueError, match="no two owned texels"):
            lightmap.texel_extent(np.zeros(lonely.shape + (3,)), lonely)


def test_batch_variance_is_welfords_variance_of_the_mean():
    # two bakes: mean (a + b) / 2, sample variance (a - b)^2 / 2, of the mean (a - b)^2 / 4
    a, b = np.full((2, 3), 1.0), np.full((2, 3), 3.0)
    mean, var = lightmap.batch_variance([a, b])
    assert mean.shape == (2, 3) and (mean == 2.0).all() and var.shape == (2, 3) and (var == 1.0).all()
    # three words: the components' variances add up — (1, 2, 0) and (3, 6, 0): 1 + 4 + 0
    a3, b3 = np.broadcast_to([1.0, 2.0, 0.0], (2, 3, 3)), np.broadcast_to([3.0, 6.0, 0.0], (2, 3, 3))
    mean, var = lightmap.batch_variance([a3, b3])
    assert mean.shape == (2, 3, 3) and (mean == np.array([2.0, 4.0, 0.0])).all() and (var == 5.0).all()
    # four bakes 0, 2, 4, 6 (dyadic, so exact): mean 3, M2 = 20, / 3 / 4
    mean, var = lightmap.batch_variance([np.full((1, 1), v) for v in (0.0, 2.0, 4.0, 6.0)])
    assert mean[0, 0] == 3.0 and var[0, 0] == (20.0 / 3.0) / 4.0
    # equal bakes: no variance; against numpy on random ones
    assert (lightmap.batch_variance([a3, a3, a3])[1] == 0.0).all()
    rng = np.random.default_rng(5)
    bakes = rng.normal(size=(6, 4, 5, 3))
    mean, var = lightmap.batch_variance(list(bakes))
    assert np.allclose(mean, bakes.mean(axis=0), rtol=0, atol=1e-15)
    assert np.allclose(var, bakes.var(axis=0, ddof=1).sum(axis=-1) / 6.0, rtol=1e-13, atol=0)
    with pytest.raises(ValueError, match="two bakes"):
        lightmap.batch_variance([a])


# ---- the yardstick by hand
def flat(h, w, texel=0.1):
    """a map of one chart: a floor y = 0, texel (x, y) at (x, 0, y) * texel, normal +y"""
    yy, xx = np.mgrid[0:h, 0:w]
    position = np.stack([xx * texel, np.zeros((h, w)), yy * texel], axis=-1)
    normal = np.broadcast_to([0.0, 1.0, 0.0], (h, w, 3)).copy()
    return np.zeros((h, w), dtype=np.int32), position, normal


SIG = dict(sigma_normal=0.1, sigma_plane=0.05, sigma_distance=0.4)


def test_the_model_weighs_one_tap_as_the_contract_writes_it():
    """two texels in a row, 0 and 1: texel 0 takes its own centre tap, k(0) k(0) = 0.140625, and its neighbour at
    (dx, dy) = (1, 0), k(1) k(0) exp(-e), e = ((0 + 0) + 0.1^2 / 0.4^2)"""
    owner, position, normal = flat(1, 2)
    values = np.array([[0.0, 1.0]])
    out = F.filter_lightmap(values, owner, position, normal, levels=1, **SIG)
    d2 = position[0, 1, 0] * position[0, 1, 0]
    e = d2 / (0.4 * 0.4)
    w = 0.09375 * float(F.rpt_exp(np.array([-e]))[0])
    assert out[0, 0] == (0.0 + w * 1.0) / (0.140625 + w) and out[0, 1] == (w * 0.0 + 0.140625 * 1.0) / (w + 0.140625)
    assert abs(w - 0.09375 * math.exp(-e)) <= 1e-16
    # level 1 has twice the spacing and twice the sigma: no tap at offset 2 in a map of two — the centre alone
    c1, _ = F.level(values[..., None], None, owner >= 0, normal, position, 2, 0.1, 0.05, 0.4, 2.0)
    assert M.same(c1[..., 0], (0.140625 * values) / 0.140625)
    # with a variance: the colour term on top, |d|^2 = 1 over (4 * (v_p + v_q) + 1e-12), and V = sum w^2 v
    variance = np.array([[0.25, 0.25]])      # its prefilter: (0.25 * 0.25 + 0.125 * 0.25) / 0.375 = 0.25 (dyadic)
    out, out_v = F.filter_lightmap(values, owner, position, normal, levels=1, variance=variance, sigma_color=2.0, **SIG)
    ec = e + 1.0 / ((2.0 * 2.0) * (0.25 + 0.25) + 1e-12)
    wc = 0.09375 * float(F.rpt_exp(np.array([-ec]))[0])
    assert out[0, 0] == (0.0 + wc * 1.0) / (0.140625 + wc)
    assert out_v[0, 0] == ((0.140625 * 0.140625) * 0.25 + (wc * wc) * 0.25) / ((0.140625 + wc) * (0.140625 + wc))
    # one word and three words of the same value agree per component when no colour term is read
    out3 = F.filter_lightmap(np.stack([values, 2.0 * values, values], axis=-1), owner, position, normal, levels=1, **SIG)
    assert M.same(out3[..., 0], F.filter_lightmap(values, owner, position, normal, levels=1, **SIG))


def test_a_step_beyond_the_map_leaves_the_centre_tap():
    owner, position, normal = flat(5, 5)
    values = np.random.default_rng(1).normal(size=(5, 5, 3))
    variance = np.full((5, 5), 0.5)
    c1, v1 = F.level(values, variance, owner >= 0, normal, position, 8, 0.1, 0.05, 0.4, 2.0)
    assert M.same(c1, (0.140625 * values) / 0.140625)
    assert M.same(v1, ((0.140625 * 0.140625) * variance) / (0.140625 * 0.140625))
    ones = np.ones((5, 5))
    assert (F.level(ones[..., None], None, owner >= 0, normal, position, 128, 0.1, 0.05, 0.4, 2.0)[0][..., 0] == 1.0).all()
    # step 4 in a map of five: the corners still see each other
    c4, _ = F.level(np.eye(5)[..., None], None, owner >= 0, normal, position, 4, 0.1, 0.05, 0.4, 2.0)
    assert c4[0, 0, 0] < 1.0 and c4[2, 2, 0] == 1.0


@pytest.mark.parametrize("with_variance", [False, True], ids=["plain", "variance"])
@pytest.mark.parametrize("odd", [NAN, INF, -INF], ids=["nan", "inf", "-inf"])
def test_a_nan_or_infinite_texel_keeps_its_value_and_never_spreads(odd, with_variance):
    owner, position, normal = flat(5, 5)
    kw = dict(variance=np.full((5, 5), 0.01), sigma_color=2.0) if with_variance else {}
    for words in (1, 3):
        values = np.ones((5, 5, 3)) if words == 3 else np.ones((5, 5))
        if words == 3:
            values[2, 2, 1] = odd
        else:
            values[2, 2] = odd
        res = F.filter_lightmap(values, owner, position, normal, levels=3, **SIG, **kw)
        out = res[0] if with_variance else res
        others = np.ones((5, 5), dtype=bool)
        others[2, 2] = False
        assert (out[others] == 1.0).all()                       # sums of w * 1.0 over their own w: exactly 1.0
        assert M.same(out[2, 2], values[2, 2])                  # the texel itself: its value, the finite components too
        if with_variance:
            assert np.isfinite(res[1]).all() and (res[1] > 0.0).all()


def test_a_texel_that_is_not_valid_keeps_its_bits_and_gives_nothing():
    owner, position, normal = flat(5, 5)
    values = np.ones((5, 5, 3))
    variance = np.full((5, 5), 0.25)
    owner[1, 1], values[1, 1], variance[1, 1] = -1, (1e30, -0.0, NAN), 7.0
    owner[3, 2], values[3, 2], variance[3, 2] = -5, (INF, 2.0, -3.0), NAN
    position[1, 1], normal[3, 2] = NAN, NAN                       # its guides are not read either
    keep = owner < 0
    for levels in (0, 1, 3):
        out = F.filter_lightmap(values, owner, position, normal, levels=levels, **SIG)
        assert M.same(out[keep], values[keep]) and (out[~keep] == 1.0).all()
        out, out_v = F.filter_lightmap(values, owner, position, normal, levels=levels, variance=variance, **SIG)
        assert M.same(out[keep], values[keep]) and (out[~keep] == 1.0).all()
        assert M.same(out_v[keep], variance[keep]) and np.isfinite(out_v[~keep]).all()
    # levels == 0: out_variance is the prefilter's result — 0.25 everywhere it is valid, the invalid neighbours left out
    assert (F.filter_lightmap(values, owner, position, normal, levels=0, variance=variance, **SIG)[1][~keep] == 0.25).all()
    # the dilation fills them afterwards, from the filtered valid texels alone
    out = F.filter_lightmap(values, owner, position, normal, levels=2, dilate=1, **SIG)
    assert (out == 1.0).all()
    # one word, and the gutter's value is not read: whatever it holds, the valid texels come out the same
    v1 = np.random.default_rng(2).normal(size=(5, 5))
    a = F.filter_lightmap(v1, owner, position, normal, levels=2, **SIG)
    v2 = v1.copy()
    v2[keep] = (123.0, NAN)
    b = F.filter_lightmap(v2, owner, position, normal, levels=2, **SIG)
    assert M.same(a[~keep], b[~keep]) and M.same(b[keep], v2[keep])


# ---- the quality condition, on one stated map
def two_charts(far=False):
    """48 x 48 texels of 0.1 world units.  Chart A: a floor y = 0 on columns 2..21; chart B: a wall x = 0 with normal +x on
    columns 26..45; both on rows 2..45, row r at z = 0.1 (r + 0.5).  The two meet in a crease along x = 0, y = 0: A's column
    21 and B's column 26 are the texels next to it.  far: B instead on A's plane, 100 units further along x."""
    h = w = 48
    owner = np.full((h, w), -1, dtype=np.int32)
    position, normal = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    rows = np.arange(2, 46)
    z = 0.1 * (rows + 0.5)
    for col in range(2, 22):
        owner[rows, col] = 0
        position[rows, col] = np.stack([np.full(z.shape, 0.1 * (21 - col + 0.5)), np.zeros(z.shape), z], axis=-1)
        normal[rows, col] = (0.0, 1.0, 0.0)
    for col in range(26, 46):
        owner[rows, col] = 1
        u = 0.1 * (col - 26 + 0.5)
        if far:
            position[rows, col] = np.stack([np.full(z.shape, 100.0 + u), np.zeros(z.shape), z], axis=-1)
            normal[rows, col] = (0.0, 1.0, 0.0)
        else:
            position[rows, col] = np.stack([np.zeros(z.shape), np.full(z.shape, u), z], axis=-1)
            normal[rows, col] = (1.0, 0.0, 0.0)
    return owner, position, normal


def test_the_filter_halves_the_noise_on_each_chart_and_keeps_the_charts_apart():
    """The map, the field and the settings are the ones the feature was specified with: values = a smooth field per chart +
    default_rng(0x4C46).normal(0, 0.2), sigma_normal 0.1, sigma_plane 0.05, sigma_distance 0.4, 2 levels.  Measured here with
    rpt_exp and this test's fields: RMSE to the clean field 0.0523 against 0.1989 unfiltered on A, 0.0450 against 0.1972 on
    B; the bound is half.

    At 2 levels the widest tap offset is 2 * 2 = 4 texels and the gutter between the charts is 4 texels wide (column 21 to
    column 26 is 5), so no tap of this map crosses it: the two conditions on what reaches A hold with exactly 0, and a map
    on which the distance term is switched off (sigma_distance 1e9) shows no leak either.  They are therefore ALSO held at 3
    levels, where the offset 8 crosses the gutter: across the crease at most 1e-4; B on A's plane 100 units away: A stays
    exactly +0.0 — and not with sigma_distance 1e9, which shows the term doing the work.  Measured at 3 levels: 1.5e-6 across
    the crease, +0.0 and 0.083."""
    owner, position, normal = two_charts()
    a, b = owner == 0, owner == 1
    assert int(a.sum()) == int(b.sum()) == 44 * 20
    clean = np.where(a, 1.0 + 0.5 * np.sin(2.0 * position[..., 0]) * np.cos(position[..., 2]),
                     np.where(b, 2.0 + 0.3 * position[..., 1] - 0.1 * position[..., 2] * position[..., 2], 0.0))
    noisy = np.where(owner >= 0, clean + np.random.default_rng(0x4C46).normal(0.0, 0.2, size=clean.shape), 0.0)
    out = F.filter_lightmap(noisy, owner, position, normal, levels=2, **SIG)
    rmse = lambda x, m: float(np.sqrt(np.mean((x[m] - clean[m]) ** 2)))
    for m, name in ((a, "A"), (b, "B")):
        before, after = rmse(noisy, m), rmse(out, m)
        print("chart %s: rmse %.4f unfiltered, %.4f filtered" % (name, before, after))
        assert after <= 0.5 * before
    assert M.same(out[owner < 0], noisy[owner < 0])

    step = np.where(b, 1.0, 0.0)                 # A at 0, B at 1, no noise
    for levels in (2, 3):
        leak = float(np.abs(F.filter_lightmap(step, owner, position, normal, levels=levels, **SIG)[a]).max())
        print("crease, %d levels: the largest value on A %.3e" % (levels, leak))
        assert leak <= 1e-4
    owner_f, position_f, normal_f = two_charts(far=True)
    for levels in (2, 3):
        out = F.filter_lightmap(step, owner_f, position_f, normal_f, levels=levels, **SIG)
        assert M.same(out[a], np.zeros(int(a.sum())))          # exactly +0.0
    loose = F.filter_lightmap(step, owner_f, position_f, normal_f, levels=3, sigma_normal=0.1, sigma_plane=0.05, sigma_distance=1e9)
    leak = float(loose[a].max())
    print("B on A's plane 100 units away, sigma_distance 1e9, 3 levels: the largest value on A %.3f" % leak)
    assert leak > 0.01
