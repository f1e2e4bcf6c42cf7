"""rptgpu_first_hits and rptgpu_render_views_aov without a GPU: the four symbols and both new structs' layouts against the
header, every refusal that comes before the device — through the host and the device entry points, with its code, its detail
and the output arrays untouched —, no CPU fallback, what GpuScene.first_hits / GpuScene.render_views_aov lower their
arguments to, and the piece planner (rpt_amd/csrc/render_plan.h hits_piece) in a stand-alone program
(tests/cpp/hits_piece_check.cpp), plain and under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import Camera, View, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_first_hits", "rptgpu_first_hits_device", "rptgpu_render_views_aov", "rptgpu_render_views_aov_device")
QUERY_FIELDS = ("struct_size", "channels", "precision_mode", "flags")
ARRAY_FIELDS = ("struct_size", "reserved", "t", "normal", "object", "position", "albedo")
HIT_BITS = (("t", _abi.RPT_HIT_T), ("normal", _abi.RPT_HIT_NORMAL), ("object", _abi.RPT_HIT_OBJECT),
            ("position", _abi.RPT_HIT_POSITION), ("albedo", _abi.RPT_HIT_ALBEDO))


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES)
    assert set(NAMES) <= {s[0] for s in _abi.SYMBOLS} and len(_abi.SYMBOLS) == 62
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptHitQuery));' + \
          "".join('printf(" %%zu", offsetof(RptHitQuery, %s));' % f for f in QUERY_FIELDS) + \
          'printf(" %zu", sizeof(RptHitArrays));' + \
          "".join('printf(" %%zu", offsetof(RptHitArrays, %s));' % f for f in ARRAY_FIELDS) + \
          'printf(" %u %u %u %u %u", RPT_HIT_T, RPT_HIT_NORMAL, RPT_HIT_OBJECT, RPT_HIT_POSITION, RPT_HIT_ALBEDO);' + \
          'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    q, a, bits = nums[:5], nums[5:13], nums[13:]
    assert C.sizeof(_abi.RptHitQuery) == q[0] == 16
    assert [getattr(_abi.RptHitQuery, f).offset for f in QUERY_FIELDS] == q[1:] == [0, 4, 8, 12]
    assert [f for f, _ in _abi.RptHitQuery._fields_] == list(QUERY_FIELDS)
    assert C.sizeof(_abi.RptHitArrays) == a[0] == 48
    assert [getattr(_abi.RptHitArrays, f).offset for f in ARRAY_FIELDS] == a[1:] == [0, 4, 8, 16, 24, 32, 40]
    assert [f for f, _ in _abi.RptHitArrays._fields_] == list(ARRAY_FIELDS)
    assert bits == [b for _, b in HIT_BITS] == [1, 2, 4, 8, 16] and _abi.RPT_HIT_ALL == 31


def hit_query(**kw):
    q = _abi.RptHitQuery()
    q.struct_size, q.channels = C.sizeof(_abi.RptHitQuery), _abi.RPT_HIT_ALL
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; first hits run the closest-hit query "
              "only").encode()
MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
Q_SIZE = b"RptHitQuery: struct_size is not sizeof(RptHitQuery)"
A_SIZE = b"RptHitArrays: struct_size is not sizeof(RptHitArrays)"
# (what is passed: q, the arrays struct's fields, which arrays are NULL, n) -> the detail
HIT_REFUSALS = [
    ("no query", dict(q=None), b"null RptHitQuery"),
    ("no arrays struct", dict(arrays=None), b"null RptHitArrays"),
    ("query size 0", dict(q=hit_query(struct_size=0)), Q_SIZE),
    ("query size 12", dict(q=hit_query(struct_size=12)), Q_SIZE),
    ("query size 24", dict(q=hit_query(struct_size=24)), Q_SIZE),
    ("arrays size 0", dict(a_size=0), A_SIZE),
    ("arrays size 40", dict(a_size=40), A_SIZE),
    ("arrays size 56", dict(a_size=56), A_SIZE),
    ("no channel", dict(q=hit_query(channels=0)), b"RptHitQuery: channels == 0 (name at least one RPT_HIT_* channel)"),
    ("unknown bit", dict(q=hit_query(channels=32 | _abi.RPT_HIT_T)), b"RptHitQuery: channels names an unknown RPT_HIT_* bit"),
    ("high bit", dict(q=hit_query(channels=1 << 31)), b"RptHitQuery: channels names an unknown RPT_HIT_* bit"),
    ("reserved", dict(reserved=1), b"RptHitArrays: reserved != 0"),
    ("t", dict(t=False), b"RptHitArrays: RPT_HIT_T is named but t is NULL"),
    ("normal", dict(normal=False), b"RptHitArrays: RPT_HIT_NORMAL is named but normal is NULL"),
    ("object", dict(object=False), b"RptHitArrays: RPT_HIT_OBJECT is named but object is NULL"),
    ("position", dict(position=False), b"RptHitArrays: RPT_HIT_POSITION is named but position is NULL"),
    ("albedo", dict(albedo=False), b"RptHitArrays: RPT_HIT_ALBEDO is named but albedo is NULL"),
    ("mode", dict(q=hit_query(precision_mode=1)), MODE),
    ("persistent", dict(q=hit_query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=hit_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("origins", dict(origins=False), b"null argument"),
    ("dirs", dict(dirs=False), b"null argument"),
    ("handle", dict(), b"null handle"),
    ("handle, one channel and only its array", dict(q=hit_query(channels=_abi.RPT_HIT_OBJECT), t=False, normal=False,
                                                     position=False, albedo=False), b"null handle"),
    ("handle, no rays", dict(n=0, origins=False, dirs=False), b"null handle"),
]


def _another_detail_first(lib):
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(HIT_REFUSALS)), ids=[r[0] for r in HIT_REFUSALS])
def test_first_hits_refuses_before_the_device(row, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    _, kw, detail = HIT_REFUSALS[row]
    lib = _abi.load_library()
    o, d = np.full(12, 7.0), np.full(12, 7.0)
    outs = {"t": np.full(4, 7.0), "normal": np.full(12, 7.0), "object": np.full(4, 7, dtype=np.int32),
            "position": np.full(12, 7.0), "albedo": np.full(12, 7.0)}
    q = kw.get("q", hit_query())
    a = _abi.RptHitArrays()
    a.struct_size, a.reserved = kw.get("a_size", C.sizeof(_abi.RptHitArrays)), kw.get("reserved", 0)
    types = dict(_abi.RptHitArrays._fields_)
    for name, arr in outs.items():  # (device: pointers that are never followed — every row is refused before the device)
        if kw.get(name, True):
            setattr(a, name, arr.ctypes.data_as(types[name]))
    ap = C.byref(a) if kw.get("arrays", True) is not None else None
    qp = C.byref(q) if q is not None else None
    use = lambda name, arr: arr if kw.get(name, True) else None
    _another_detail_first(lib)
    if device:
        p = lambda arr: C.c_void_p(arr.ctypes.data) if arr is not None else None
        rc = lib.rptgpu_first_hits_device(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), qp, ap, None)
    else:
        p = lambda arr: arr.ctypes.data_as(PD) if arr is not None else None
        rc = lib.rptgpu_first_hits(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), qp, ap)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and all((arr == 7).all() for arr in outs.values())


def view_query(**kw):
    q = _abi.RptViewQuery()
    q.struct_size, q.width, q.height, q.iterations, q.seed = C.sizeof(_abi.RptViewQuery), 2, 2, 1, 1
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _view(projection=_abi.RPT_VIEW_PERSPECTIVE, aperture=0.0, ortho_scale=1.0):
    v = _abi.RptView()
    v.camera = Camera((0.0, 0.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.8, aperture, 1.0).lower()
    v.projection, v.ortho_scale = projection, ortho_scale
    return v


V_SIZE = b"RptViewQuery: struct_size is not sizeof(RptViewQuery)"
VIEWS_PERSISTENT = ("RptViewQuery: RPT_FLAG_PERSISTENT — the persistent kernel renders one camera's frame; a batch of views runs "
                    "the wavefront pipeline only").encode()
B_SIZE = b"RptAovBuffers: struct_size is not sizeof(RptAovBuffers)"
# rptgpu_render_views' refusals for the query and the views, rptgpu_render_aov's for the buffers
VIEWS_REFUSALS = [
    ("no query", dict(q=None), b"null RptViewQuery"),
    ("query size 0", dict(q=view_query(struct_size=0)), V_SIZE),
    ("query size 56", dict(q=view_query(struct_size=56)), V_SIZE),
    ("width", dict(q=view_query(width=0)), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("height", dict(q=view_query(height=0)), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("iterations", dict(q=view_query(iterations=0)), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("bounces", dict(q=view_query(max_bounces=255)), b"RptViewQuery: max_bounces > 254"),
    ("mode", dict(q=view_query(precision_mode=1)), MODE),
    ("persistent", dict(q=view_query(flags=_abi.RPT_FLAG_PERSISTENT)), VIEWS_PERSISTENT),
    ("no buffers struct", dict(buffers=None), b"null RptAovBuffers"),
    ("buffers size 0", dict(b_size=0), B_SIZE),
    ("buffers size 48", dict(b_size=48), B_SIZE),
    ("unknown channel", dict(channels=32), b"RptAovBuffers: channels names an unknown RPT_AOV_* bit"),
    ("hits", dict(hits=False), b"RptAovBuffers: hits is NULL (it is always written)"),
    ("depth", dict(depth=False), b"RptAovBuffers: RPT_AOV_DEPTH is named but depth is NULL"),
    ("normal", dict(normal=False), b"RptAovBuffers: RPT_AOV_NORMAL is named but normal is NULL"),
    ("albedo", dict(albedo=False), b"RptAovBuffers: RPT_AOV_ALBEDO is named but albedo is NULL"),
    ("position", dict(position=False), b"RptAovBuffers: RPT_AOV_POSITION is named but position is NULL"),
    ("object", dict(object=False), b"RptAovBuffers: RPT_AOV_OBJECT is named but object is NULL"),
    ("no views", dict(views=None), b"null argument"),
    ("too many views", dict(n=1 << 60), b"n_views * width * height does not fit: the frames would not fit any memory"),
    ("projection", dict(views=[_view(), _view(projection=3)]),
     b"RptView: unknown projection (RPT_VIEW_PERSPECTIVE = 0, RPT_VIEW_ORTHOGRAPHIC = 1, RPT_VIEW_PANORAMA = 2)"),
    ("ortho scale 0", dict(views=[_view(_abi.RPT_VIEW_ORTHOGRAPHIC, ortho_scale=0.0), _view()]),
     b"RptView: RPT_VIEW_ORTHOGRAPHIC needs a finite ortho_scale > 0"),
    ("ortho scale nan", dict(views=[_view(), _view(_abi.RPT_VIEW_ORTHOGRAPHIC, ortho_scale=float("nan"))]),
     b"RptView: RPT_VIEW_ORTHOGRAPHIC needs a finite ortho_scale > 0"),
    ("ortho lens", dict(views=[_view(_abi.RPT_VIEW_ORTHOGRAPHIC, aperture=0.1), _view()]),
     b"RptView: aperture > 0 \xe2\x80\x94 only RPT_VIEW_PERSPECTIVE has a lens"),
    ("panorama lens", dict(views=[_view(), _view(_abi.RPT_VIEW_PANORAMA, aperture=0.1)]),
     b"RptView: aperture > 0 \xe2\x80\x94 only RPT_VIEW_PERSPECTIVE has a lens"),
    ("panorama width 1", dict(q=view_query(width=1, height=4), views=[_view(_abi.RPT_VIEW_PANORAMA), _view()]),
     b"RptView: RPT_VIEW_PANORAMA needs width >= 2 and height >= 2"),
    ("handle", dict(), b"null handle"),
    ("handle, hits only", dict(channels=0, depth=False, normal=False, albedo=False, position=False, object=False), b"null handle"),
    ("handle, no views", dict(n=0, views=None), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(VIEWS_REFUSALS)), ids=[r[0] for r in VIEWS_REFUSALS])
def test_render_views_aov_refuses_before_the_device(row, device):
    _, kw, detail = VIEWS_REFUSALS[row]
    lib = _abi.load_library()
    n_pix = 2 * 4  # two views of 2 x 2
    outs = {"hits": np.full(n_pix, 7, dtype=np.uint32), "depth": np.full(n_pix, 7.0), "normal": np.full(3 * n_pix, 7.0),
            "albedo": np.full(3 * n_pix, 7.0), "position": np.full(3 * n_pix, 7.0), "object": np.full(n_pix, 7, dtype=np.int32)}
    q = kw.get("q", view_query())
    b = _abi.RptAovBuffers()
    b.struct_size, b.channels = kw.get("b_size", C.sizeof(_abi.RptAovBuffers)), kw.get("channels", _abi.RPT_AOV_ALL)
    types = dict(_abi.RptAovBuffers._fields_)
    for name, arr in outs.items():
        if kw.get(name, True):
            setattr(b, name, arr.ctypes.data_as(types[name]))
    views = kw.get("views", [_view(), _view()])
    arr = (_abi.RptView * 2)(*views) if views is not None else None
    bp = C.byref(b) if kw.get("buffers", True) is not None else None
    qp = C.byref(q) if q is not None else None
    _another_detail_first(lib)
    if device:
        rc = lib.rptgpu_render_views_aov_device(None, kw.get("n", 2), arr, qp, bp, None)
    else:
        rc = lib.rptgpu_render_views_aov(None, kw.get("n", 2), arr, qp, bp)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert all((a == 7).all() for a in outs.values())


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never an answer from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    o = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1))
    if gpu_available:
        g = rpt_amd.GpuScene(scene)
        hit = g.first_hits(o, d)
        assert (hit["object"] >= 0).all() and np.isfinite(hit["t"]).all()
        assert (g.first_hits(o, -d, channels=_abi.RPT_HIT_OBJECT)["object"] == -1).all()
        aov = g.render_views_aov([camera], 4, 3, samples=2, seed=1)
        assert aov["hits"].shape == (1, 3, 4) and aov["hits"].max() <= 2
        return
    for call in (lambda g: g.first_hits(o, d), lambda g: g.render_views_aov([camera], 4, 3, samples=2, seed=1)):
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


def _address(p):
    return C.cast(p, C.c_void_p).value


def test_what_the_python_calls_lower_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    o = np.arange(12.0).reshape(4, 3)
    d = o[::-1] * 0.5            # not contiguous: the call sees a contiguous copy
    out = g.first_hits(o, d, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, po, pd, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert name == "rptgpu_first_hits" and h is g.handle and n == 4
    assert (q.struct_size, q.channels, q.precision_mode, q.flags) == (16, 31, _abi.RPT_PRECISION_F64_STRICT, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert (a.struct_size, a.reserved) == (48, 0)
    assert (_floats(po, 12) == o.ravel()).all() and (_floats(pd, 12) == d.ravel()).all()
    assert sorted(out) == ["albedo", "normal", "object", "position", "t"]
    assert out["t"].shape == (4,) and out["t"].dtype == np.float64 and out["object"].shape == (4,) and out["object"].dtype == np.int32
    for k in ("normal", "position", "albedo"):
        assert out[k].shape == (4, 3) and out[k].dtype == np.float64
    for k, v in out.items():
        assert _address(getattr(a, k)) == v.ctypes.data
    # one channel: the other pointers stay NULL
    out = g.first_hits(o, d, channels=_abi.RPT_HIT_T | _abi.RPT_HIT_OBJECT)
    name, (h, n, po, pd, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert sorted(out) == ["object", "t"] and (q.channels, q.flags) == (5, 0)
    assert not a.normal and not a.position and not a.albedo and _address(a.t) == out["t"].ctypes.data

    cam = Camera((0.0, 1.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.8, 0.0, 0.0)
    views = [cam, View.orthographic(cam, 2.5), View.panorama((1.0, 2.0, 3.0))]
    aov = g.render_views_aov(views, 5, 4, samples=3, seed=(1 << 63) + 5, seed_stride=7, sample_index_base=1 << 40,
                             channels=_abi.RPT_AOV_DEPTH | _abi.RPT_AOV_OBJECT, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, arr, q, b) = g.lib.calls.pop()
    q, b = q._obj, b._obj
    assert name == "rptgpu_render_views_aov" and h is g.handle and n == 3
    assert (q.struct_size, q.width, q.height, q.max_bounces, q.iterations) == (64, 5, 4, 0, 3)
    assert (q.seed, q.seed_stride, q.sample_index_base, q.exposure_value) == ((1 << 63) + 5, 7, 1 << 40, 0.0)
    assert (q.precision_mode, q.flags) == (0, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert [arr[i].projection for i in range(3)] == [_abi.RPT_VIEW_PERSPECTIVE, _abi.RPT_VIEW_ORTHOGRAPHIC, _abi.RPT_VIEW_PANORAMA]
    assert arr[1].ortho_scale == 2.5 and list(arr[2].camera.eye) == [1.0, 2.0, 3.0]
    assert (b.struct_size, b.channels) == (56, _abi.RPT_AOV_DEPTH | _abi.RPT_AOV_OBJECT)
    assert sorted(aov) == ["depth", "hits", "object"]
    assert aov["hits"].shape == (3, 4, 5) and aov["hits"].dtype == np.uint32
    assert aov["depth"].shape == (3, 4, 5) and aov["object"].dtype == np.int32
    for k, v in aov.items():
        assert _address(getattr(b, k)) == v.ctypes.data
    assert not b.normal and not b.albedo and not b.position
    mine = {"hits": np.zeros((1, 4, 5), dtype=np.uint32), "depth": np.zeros((1, 4, 5))}
    assert g.render_views_aov(views[:1], 5, 4, channels=_abi.RPT_AOV_DEPTH, out=mine)["depth"] is mine["depth"]
    name, (h, n, arr, q, b) = g.lib.calls.pop()
    assert name == "rptgpu_render_views_aov" and _address(b._obj.depth) == mine["depth"].ctypes.data
    with pytest.raises(ValueError, match="exactly the keys"):
        g.render_views_aov(views[:1], 5, 4, channels=_abi.RPT_AOV_DEPTH, out={"hits": mine["hits"]})
    with pytest.raises(ValueError, match="C-contiguous"):
        g.render_views_aov(views[:1], 5, 4, channels=0, out={"hits": np.zeros((1, 4, 5), dtype=np.int32)})
    aov = g.render_views_aov(views[:1], 5, 4)
    name, (h, n, arr, q, b) = g.lib.calls.pop()
    assert n == 1 and b._obj.channels == _abi.RPT_AOV_ALL and aov["normal"].shape == (1, 4, 5, 3)
    assert (q._obj.iterations, q._obj.seed, q._obj.seed_stride) == (1, 0x52505447, 0)
    assert not g.lib.calls
    g.handle = None


def test_the_python_calls_check_their_shapes_and_dtypes():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    z = np.zeros((3, 3))
    with pytest.raises(ValueError, match=r"origins must be an \(n, 3\) float64 array"):
        g.first_hits(np.zeros((3, 2)), z)
    with pytest.raises(ValueError, match=r"dirs must be an \(n, 3\) float64 array"):
        g.first_hits(z, z.astype(np.float32))
    with pytest.raises(ValueError, match="3 origins for 2 directions"):
        g.first_hits(z, np.zeros((2, 3)))
    with pytest.raises(TypeError, match="view 0 is a float"):
        g.render_views_aov([1.0], 4, 4)
    with pytest.raises(ValueError, match='out must be None, "torch" or a dict'):
        g.render_views_aov([], 4, 4, out="numpy")
    for call, word in ((lambda: g.first_hits(z, z), "null handle"),  # well-formed arrays: the library speaks
                       (lambda: g.first_hits(z, z, channels=0), "channels == 0"),
                       (lambda: g.first_hits(z, z, channels=64), "unknown RPT_HIT_"),
                       (lambda: g.render_views_aov([], 4, 4), "null handle"),
                       (lambda: g.render_views_aov([], 4, 4, samples=0), "must be non-zero")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call()
        assert e.value.code == E and word in str(e.value)
    g.handle = None


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hits_piece_" + request.param) / "hits_piece_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "hits_piece_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover", "planned"])
def test_hits_piece(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
