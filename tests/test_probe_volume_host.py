"""The probe volume without a GPU (include/rpt_gpu_probe_volume.h): the six symbols, detected the way a binding
detects them, and the four structs' layouts against the compiled header; every refusal that comes before the device — through
the host and the device form of all three entry points, with its code, its detail and every array untouched —; no CPU
fallback; what the Python methods lower their arguments to and their own shape and dtype checks; the host header
(rpt_amd/csrc/probe_volume_plan.h) in a stand-alone program (tests/cpp/probe_volume_plan_check.cpp), plain and under
AddressSanitizer + UBSan; and the numpy restatement of the header's rule (tests/probe_volume_model.py) against closed forms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import ProbeVolume, _abi, sh9_irradiance

import probe_volume_model as PV
import surface_model as M
from test_lightmap_lookup_host import MODE, Recorder, view_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_sample_probe_volume", "rptgpu_sample_probe_volume_device", "rptgpu_lookup_probe_volume",
         "rptgpu_lookup_probe_volume_device", "rptgpu_render_views_probe_lit", "rptgpu_render_views_probe_lit_device")
STRUCTS = (("RptProbeVolume", ("struct_size", "nx", "ny", "nz", "reserved", "origin", "spacing", "coeffs", "valid")),
           ("RptVolumeQuery", ("struct_size", "channels", "normal_bias", "fallback", "precision_mode", "flags")),
           ("RptVolumeArrays", ("struct_size", "reserved", "t", "object", "position", "normal", "value", "covered", "inside")),
           ("RptViewsProbeLitQuery", ("struct_size", "filter", "normal_bias", "unbound_irradiance")))
BITS = ("RPT_VOLUME_T", "RPT_VOLUME_OBJECT", "RPT_VOLUME_POSITION", "RPT_VOLUME_NORMAL", "RPT_VOLUME_VALUE", "RPT_VOLUME_COVERED",
        "RPT_VOLUME_INSIDE")


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and _abi.probe_volume_supported(lib)
    assert tuple(s[0] for s in _abi.PROBE_VOLUME_SYMBOLS) == NAMES and not set(NAMES) & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7

    class Older:  # a library without the six: still ABI 7, and the detection says so
        rptgpu_lookup_lightmap = None
    assert not _abi.probe_volume_supported(Older())
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){' + \
          "".join('printf("%%zu ", sizeof(%s));' % s + "".join('printf("%%zu ", offsetof(%s, %s));' % (s, f) for f in fs)
                  for s, fs in STRUCTS) + "".join('printf("%%u ", %s);' % b for b in BITS) + 'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = {"RptProbeVolume": (88, [0, 4, 8, 12, 16, 24, 48, 72, 80]), "RptVolumeQuery": (48, [0, 4, 8, 16, 40, 44]),
            "RptVolumeArrays": (64, [0, 4, 8, 16, 24, 32, 40, 48, 56]), "RptViewsProbeLitQuery": (40, [0, 4, 8, 16])}
    at = 0
    for name, fields in STRUCTS:
        cls = getattr(_abi, name)
        size, offsets = nums[at], nums[at + 1:at + 1 + len(fields)]
        at += 1 + len(fields)
        assert C.sizeof(cls) == size == want[name][0], name
        assert [getattr(cls, f).offset for f in fields] == offsets == want[name][1], name
        assert [f for f, _ in cls._fields_] == list(fields)
    assert nums[at:] == [getattr(_abi, b) for b in BITS] == [1, 2, 4, 8, 16, 32, 64]
    assert _abi.RPT_VOLUME_ALL == 127 and _abi.RPT_VOLUME_POINT == 16 | 32 | 64
    assert rpt_amd.RPT_VOLUME_VALUE == 16 and rpt_amd.probes.ProbeVolume is ProbeVolume


# ---- the refusals
def query(**kw):
    q = _abi.RptVolumeQuery()
    q.struct_size, q.channels = C.sizeof(q), _abi.RPT_VOLUME_POINT
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a probe volume is read at points or "
              "behind the closest-hit query only").encode()
Q_SIZE = b"RptVolumeQuery: struct_size is not sizeof(RptVolumeQuery)"
V_SIZE = b"RptProbeVolume: struct_size is not sizeof(RptProbeVolume)"
A_SIZE = b"RptVolumeArrays: struct_size is not sizeof(RptVolumeArrays)"
SPACING = b"RptProbeVolume: spacing is not finite and positive"
NAN, INF = float("nan"), float("inf")
# the volume's refusals, shared by all three entry points: (what is passed) -> the detail
VOLUME_REFUSALS = [
    ("no volume", dict(volume=None), b"null RptProbeVolume"),
    ("volume size 0", dict(v=dict(struct_size=0)), V_SIZE),
    ("volume size 80", dict(v=dict(struct_size=80)), V_SIZE),
    ("volume reserved", dict(v=dict(reserved=2)), b"RptProbeVolume: reserved != 0"),
    ("nx 0", dict(v=dict(nx=0)), b"RptProbeVolume: a count of 0 (nx, ny and nz are each >= 1)"),
    ("nz 0", dict(v=dict(nz=0)), b"RptProbeVolume: a count of 0 (nx, ny and nz are each >= 1)"),
    ("reserved before the counts", dict(v=dict(reserved=1, ny=0)), b"RptProbeVolume: reserved != 0"),
    ("spacing 0", dict(spacing=(1.0, 0.0, 1.0)), SPACING),
    ("spacing negative", dict(spacing=(-1.0, 1.0, 1.0)), SPACING),
    ("spacing inf", dict(spacing=(1.0, 1.0, INF)), SPACING),
    ("spacing nan", dict(spacing=(NAN, 1.0, 1.0)), SPACING),
    ("origin inf", dict(origin=(0.0, -INF, 0.0)), b"RptProbeVolume: origin is not finite"),
    ("origin nan", dict(origin=(0.0, 0.0, NAN)), b"RptProbeVolume: origin is not finite"),
    ("the counts before the spacing", dict(v=dict(nx=0), spacing=(0.0, 1.0, 1.0)), b"RptProbeVolume: a count of 0 (nx, ny and nz are each >= 1)"),
    ("null coeffs", dict(v=dict(coeffs=None)), b"RptProbeVolume: coeffs is NULL"),
    ("too many probes", dict(v=dict(nx=0xffffffff, ny=0xffffffff, nz=0xffffffff)),
     b"RptProbeVolume: nx * ny * nz probes do not fit: no allocation holds their coefficients"),
]
REFUSALS = [
    ("no query", dict(q=None), b"null RptVolumeQuery"),
    ("query size 0", dict(q=query(struct_size=0)), Q_SIZE),
    ("query size 56", dict(q=query(struct_size=56)), Q_SIZE),
    ("no channel", dict(q=query(channels=0)), b"RptVolumeQuery: channels == 0 (name at least one RPT_VOLUME_* channel)"),
    ("unknown bit", dict(q=query(channels=128 | _abi.RPT_VOLUME_VALUE)), b"RptVolumeQuery: channels names an unknown RPT_VOLUME_* bit"),
    ("high bit", dict(q=query(channels=1 << 31)), b"RptVolumeQuery: channels names an unknown RPT_VOLUME_* bit"),
    ("bias nan", dict(q=query(normal_bias=NAN)), b"RptVolumeQuery: normal_bias is not finite"),
    ("bias inf", dict(q=query(normal_bias=-INF)), b"RptVolumeQuery: normal_bias is not finite"),
    ("mode", dict(q=query(precision_mode=1)), MODE),
    ("persistent", dict(q=query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("the query before the volume", dict(q=query(channels=0), volume=None), b"RptVolumeQuery: channels == 0 (name at least one RPT_VOLUME_* channel)"),
] + VOLUME_REFUSALS + [
    ("the volume before the arrays", dict(v=dict(nx=0), arrays=None), b"RptProbeVolume: a count of 0 (nx, ny and nz are each >= 1)"),
    ("no arrays struct", dict(arrays=None), b"null RptVolumeArrays"),
    ("arrays size 0", dict(a_size=0), A_SIZE),
    ("arrays size 56", dict(a_size=56), A_SIZE),
    ("arrays reserved", dict(a_reserved=1), b"RptVolumeArrays: reserved != 0"),
    ("value", dict(value=False), b"RptVolumeArrays: RPT_VOLUME_VALUE is named but value is NULL"),
    ("covered", dict(covered=False), b"RptVolumeArrays: RPT_VOLUME_COVERED is named but covered is NULL"),
    ("inside", dict(inside=False), b"RptVolumeArrays: RPT_VOLUME_INSIDE is named but inside is NULL"),
    ("first input", dict(a=False), b"null argument"),
    ("second input", dict(b=False), b"null argument"),
    ("handle", dict(), b"null handle"),
    ("handle, a null valid mask is legal", dict(v=dict(valid=None)), b"null handle"),
    ("handle, one channel and only its array", dict(q=query(channels=_abi.RPT_VOLUME_VALUE), covered=False, inside=False), b"null handle"),
    ("handle, nothing to do", dict(n=0, a=False, b=False), b"null handle"),
]
# the ray form alone: its four hit channels
RAY_REFUSALS = [
    ("t", dict(q=query(channels=_abi.RPT_VOLUME_ALL), t=False), b"RptVolumeArrays: RPT_VOLUME_T is named but t is NULL"),
    ("object", dict(q=query(channels=_abi.RPT_VOLUME_ALL), object=False), b"RptVolumeArrays: RPT_VOLUME_OBJECT is named but object is NULL"),
    ("position", dict(q=query(channels=_abi.RPT_VOLUME_ALL), position=False), b"RptVolumeArrays: RPT_VOLUME_POSITION is named but position is NULL"),
    ("normal", dict(q=query(channels=_abi.RPT_VOLUME_ALL), normal=False), b"RptVolumeArrays: RPT_VOLUME_NORMAL is named but normal is NULL"),
    ("handle, all seven", dict(q=query(channels=_abi.RPT_VOLUME_ALL)), b"null handle"),
]
POINT_REFUSALS = [
    ("a ray channel", dict(q=query(channels=_abi.RPT_VOLUME_VALUE | _abi.RPT_VOLUME_T)),
     b"RptVolumeQuery: channels names a channel of the ray form (a point has VALUE, COVERED and INSIDE only)"),
    ("all seven", dict(q=query(channels=_abi.RPT_VOLUME_ALL)),
     b"RptVolumeQuery: channels names a channel of the ray form (a point has VALUE, COVERED and INSIDE only)"),
]


def volume_record(kw, ins):
    """an RptProbeVolume of 3 x 2 x 1 probes over the sentinel arrays `ins`, with kw's overrides"""
    r = _abi.RptProbeVolume()
    types = dict(_abi.RptProbeVolume._fields_)
    fields = dict(struct_size=C.sizeof(r), nx=3, ny=2, nz=1, reserved=0, coeffs=ins["coeffs"], valid=ins["valid"])
    fields.update(kw.get("v", {}))
    for name, v in fields.items():
        setattr(r, name, v.ctypes.data_as(types[name]) if isinstance(v, np.ndarray) else v)
    r.origin, r.spacing = _abi.V3(*kw.get("origin", (0.0, 0.0, 0.0))), _abi.V3(*kw.get("spacing", (1.0, 2.0, 0.5)))
    return r


def a_detail_of_another_call(lib):
    """a call with another detail first: the text checked afterwards is the call's own"""
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"


CASES = [("sample", r) for r in REFUSALS + POINT_REFUSALS] + [("lookup", r) for r in REFUSALS + RAY_REFUSALS]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s: %s" % (f, r[0]) for f, r in CASES])
def test_the_point_and_ray_forms_refuse_before_the_device(case, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    form, (_, kw, detail) = CASES[case]
    lib = _abi.load_library()
    a, b = np.full(12, 7.0), np.full(12, 7.0)
    outs = {"t": np.full(4, 7.0), "object": np.full(4, 7, dtype=np.int32), "position": np.full(12, 7.0), "normal": np.full(12, 7.0),
            "value": np.full(12, 7.0), "covered": np.full(4, 7, dtype=np.uint8), "inside": np.full(4, 7, dtype=np.uint8)}
    ins = {"coeffs": np.full(6 * 27, 7.0), "valid": np.full(6, 7, dtype=np.uint8)}
    q = kw.get("q", query())
    arr = _abi.RptVolumeArrays()
    arr.struct_size, arr.reserved = kw.get("a_size", C.sizeof(arr)), kw.get("a_reserved", 0)
    types = dict(_abi.RptVolumeArrays._fields_)
    for name, o in outs.items():  # (device: pointers that are never followed — every row is refused before the device)
        if kw.get(name, True):
            setattr(arr, name, o.ctypes.data_as(types[name]))
    rec = volume_record(kw, ins)
    vp = C.byref(rec) if kw.get("volume", True) is not None else None
    ap = C.byref(arr) if kw.get("arrays", True) is not None else None
    qp = C.byref(q) if q is not None else None
    use = lambda name, x: x if kw.get(name, True) else None
    a_detail_of_another_call(lib)
    fn = getattr(lib, "rptgpu_%s_probe_volume%s" % (form, "_device" if device else ""))
    if device:
        p = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None
        rc = fn(None, kw.get("n", 4), p(use("a", a)), p(use("b", b)), vp, qp, ap, None)
    else:
        p = lambda x: x.ctypes.data_as(PD) if x is not None else None
        rc = fn(None, kw.get("n", 4), p(use("a", a)), p(use("b", b)), vp, qp, ap)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (a == 7).all() and (b == 7).all() and all((x == 7).all() for x in list(outs.values()) + list(ins.values()))


def views_query(**kw):
    q = _abi.RptViewsProbeLitQuery()
    q.struct_size, q.filter = C.sizeof(q), _abi.RPT_LOOKUP_BILINEAR
    for k, v in kw.items():
        setattr(q, k, v)
    return q


VQ_SIZE = b"RptViewsProbeLitQuery: struct_size is not sizeof(RptViewsProbeLitQuery)"
# rptgpu_render_views' refusals of the RptViewQuery first, then this call's query, the volume, out and the views, each view, the
# bindings, the handle
VIEW_REFUSALS = [
    ("no view query", dict(qv=None), b"null RptViewQuery"),
    ("zero width", dict(qv=view_query(width=0)), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("views persistent", dict(qv=view_query(flags=_abi.RPT_FLAG_VIEWS_PERSISTENT)), b"RptViewQuery: RPT_FLAG_VIEWS_PERSISTENT"),
    ("the view query before this call's", dict(qv=view_query(height=0), q=None), b"RptViewQuery: width, height and iterations must be non-zero"),
    ("no query", dict(q=None), b"null RptViewsProbeLitQuery"),
    ("query size 0", dict(q=views_query(struct_size=0)), VQ_SIZE),
    ("query size 32", dict(q=views_query(struct_size=32)), VQ_SIZE),
    ("filter 2", dict(q=views_query(filter=2)), b"RptViewsProbeLitQuery: filter is neither RPT_LOOKUP_NEAREST nor RPT_LOOKUP_BILINEAR"),
    ("bias nan", dict(q=views_query(normal_bias=NAN)), b"RptViewsProbeLitQuery: normal_bias is not finite"),
    ("the query before the volume", dict(q=views_query(filter=9), volume=None), b"RptViewsProbeLitQuery: filter is neither"),
] + VOLUME_REFUSALS + [
    ("the volume before out", dict(v=dict(nz=0), out=False), b"RptProbeVolume: a count of 0"),
    ("no out", dict(out=False), b"null out"),
    ("no views", dict(views=False), b"null argument"),
    ("too many views", dict(n_views=1 << 60), b"n_views * width * height does not fit"),
    ("unknown projection", dict(projection=9), b"RptView: unknown projection"),
    ("the views before the bindings", dict(projection=9, b0=dict(width=0)), b"RptView: unknown projection"),
    ("null bindings", dict(bindings=None), b"null bindings with n_bindings > 0"),
    ("width 0", dict(b0=dict(width=0)), b"binding 0: width or height is 0"),
    ("null map", dict(b0=dict(map=None)), b"binding 0: map is NULL"),
    ("handle", dict(), b"null handle"),
    ("handle, no views", dict(n_views=0, views=False), b"null handle"),
    ("handle, no bindings", dict(n_bindings=0, bindings=None), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(VIEW_REFUSALS)), ids=[r[0] for r in VIEW_REFUSALS])
def test_render_views_probe_lit_refuses_before_the_device(row, device):
    _, kw, detail = VIEW_REFUSALS[row]
    lib = _abi.load_library()
    out = np.full(2 * 3 * 4 * 3, 7.0)
    ins = {"uvs": np.full(12, 7.0), "map": np.full(6, 7.0), "mask": np.full(6, 7, dtype=np.uint8), "coeffs": np.full(6 * 27, 7.0),
           "valid": np.full(6, 7, dtype=np.uint8)}
    views = (_abi.RptView * 2)()
    for v in views:
        v.camera.direction[2], v.camera.up[1], v.camera.fov = -1.0, 1.0, 0.7
    views[1].projection = kw.get("projection", 0)
    recs = (_abi.RptLightmapBinding * 1)()
    btypes = dict(_abi.RptLightmapBinding._fields_)
    fields = dict(struct_size=C.sizeof(recs[0]), object=3, n_tris=2, width=3, height=2, components=1, reserved=0, uvs=ins["uvs"],
                  map=ins["map"], valid=ins["mask"])
    fields.update(kw.get("b0", {}))
    for name, val in fields.items():
        setattr(recs[0], name, val.ctypes.data_as(btypes[name]) if isinstance(val, np.ndarray) else val)
    rec = volume_record(kw, ins)
    qv, q = kw.get("qv", view_query()), kw.get("q", views_query())
    args = [None, kw.get("n_views", 2), views if kw.get("views", True) else None, C.byref(qv) if qv is not None else None,
            kw.get("n_bindings", 1), recs if kw.get("bindings", True) is not None else None,
            C.byref(rec) if kw.get("volume", True) is not None else None, C.byref(q) if q is not None else None]
    a_detail_of_another_call(lib)
    if device:
        rc = lib.rptgpu_render_views_probe_lit_device(*args, C.c_void_p(out.ctypes.data) if kw.get("out", True) else None, None)
    else:
        rc = lib.rptgpu_render_views_probe_lit(*args, out.ctypes.data_as(PD) if kw.get("out", True) else None)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None).startswith(detail)
    assert (out == 7).all() and all((x == 7).all() for x in ins.values())


def test_there_is_no_cpu_fallback():
    """with well-formed arguments and no handle the calls say so, and never compute: a machine without a device gets no value"""
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    vol = ProbeVolume((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), np.ones((8, 9, 3)))
    z = np.zeros((3, 3))
    cam = rpt_amd.Camera.look_at((0.0, 1.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.7)
    for call in (lambda: g.sample_probe_volume(z, z, vol), lambda: g.lookup_probe_volume(z, z, vol),
                 lambda: g.render_views_probe_lit([cam], 4, 3, [], vol, seed=1)):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call()
        assert e.value.code == E and "null handle" in str(e.value)
    # the no-device code exists and no symbol of a host implementation does
    assert _abi.RPTGPU_E_NO_DEVICE != 0 and not any("cpu" in s[0] or "host" in s[0] for s in _abi.PROBE_VOLUME_SYMBOLS)
    g.handle = None


# ---- the Python methods
def test_what_the_python_calls_lower_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    address = lambda p: C.cast(p, C.c_void_p).value
    floats = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
    o = np.arange(12.0).reshape(4, 3)
    d = o[::-1] * 0.5            # not contiguous: the call sees a contiguous copy
    coeffs = np.arange(12 * 27.0).reshape(2, 2, 3, 9, 3)
    valid = np.arange(12).reshape(2, 2, 3) % 2 == 0
    vol = ProbeVolume((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), (3, 2, 2), coeffs, valid)
    out = g.sample_probe_volume(o, d, vol, normal_bias=0.125, fallback=(1.0, 2.0, 3.0))
    name, (h, n, pa, pb, rec, q, a) = g.lib.calls.pop()
    rec, q, a = rec._obj, q._obj, a._obj
    assert name == "rptgpu_sample_probe_volume" and h is g.handle and n == 4
    assert (q.struct_size, q.channels, q.normal_bias, tuple(q.fallback), q.precision_mode, q.flags) == \
        (48, _abi.RPT_VOLUME_POINT, 0.125, (1.0, 2.0, 3.0), _abi.RPT_PRECISION_F64_STRICT, 0)
    assert (rec.struct_size, rec.nx, rec.ny, rec.nz, rec.reserved, tuple(rec.origin), tuple(rec.spacing)) == \
        (88, 3, 2, 2, 0, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0))
    assert address(rec.coeffs) == coeffs.ctypes.data and (np.ctypeslib.as_array(rec.valid, shape=(12,)) == valid.ravel()).all()
    assert (floats(pa, 12) == o.ravel()).all() and (floats(pb, 12) == d.ravel()).all()
    assert sorted(out) == ["covered", "inside", "value"] and out["value"].shape == (4, 3) and out["inside"].dtype == np.uint8
    assert not a.t and not a.normal and all(address(getattr(a, k)) == v.ctypes.data for k, v in out.items())
    # the ray form: all seven channels, the flags, coefficients in index order, no mask
    flat = ProbeVolume(vol.origin, vol.spacing, vol.counts, coeffs.reshape(12, 9, 3))
    out = g.lookup_probe_volume(o, d, flat, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, pa, pb, rec, q, a) = g.lib.calls.pop()
    rec, q, a = rec._obj, q._obj, a._obj
    assert name == "rptgpu_lookup_probe_volume" and (q.channels, q.flags, q.normal_bias) == (127, _abi.RPT_FLAG_GENERAL_TRAVERSAL, 0.0)
    assert address(rec.coeffs) == coeffs.ctypes.data and not rec.valid
    assert sorted(out) == ["covered", "inside", "normal", "object", "position", "t", "value"]
    assert out["object"].dtype == np.int32 and out["normal"].shape == (4, 3) and out["t"].shape == (4,)
    # the views form
    cam = rpt_amd.Camera.look_at((0.0, 1.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.7)
    uvs, grey = np.arange(12.0).reshape(2, 3, 2) / 12.0, np.arange(6.0).reshape(2, 3)
    frames = g.render_views_probe_lit([cam, rpt_amd.View.panorama((0.0, 1.0, 0.0))], 8, 6, [rpt_amd.lightmap.Binding(4, uvs, grey)], vol,
                                      samples=3, seed=11, seed_stride=2, sample_index_base=5, exposure_value=1.5, filter="nearest",
                                      normal_bias=0.5, unbound_irradiance=(1.0, 2.0, 3.0))
    name, (h, n, arr, qv, nb, recs, rec, q, po) = g.lib.calls.pop()
    qv, q, rec = qv._obj, q._obj, rec._obj
    assert name == "rptgpu_render_views_probe_lit" and n == 2 and nb == 1 and not g.lib.calls
    assert (qv.width, qv.height, qv.iterations, qv.seed, qv.seed_stride, qv.sample_index_base, qv.exposure_value) == (8, 6, 3, 11, 2, 5, 1.5)
    assert (q.struct_size, q.filter, q.normal_bias, tuple(q.unbound_irradiance)) == (40, _abi.RPT_LOOKUP_NEAREST, 0.5, (1.0, 2.0, 3.0))
    assert (rec.nx, rec.ny, rec.nz) == (3, 2, 2) and recs[0].object == 4
    assert frames.shape == (2, 6, 8, 3) and address(po) == frames.ctypes.data
    g.handle = None


def test_the_python_calls_check_their_shapes_and_dtypes():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    z, c = np.zeros((3, 3)), np.zeros((2, 2, 3, 9, 3))
    V = lambda coeffs, valid=None, counts=(3, 2, 2): ProbeVolume((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), counts, coeffs, valid)
    cam = rpt_amd.Camera.look_at((0.0, 1.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.7)
    for call, word in ((lambda: g.sample_probe_volume(np.zeros((3, 2)), z, V(c)), r"positions must be an \(n, 3\) float64 array"),
                       (lambda: g.sample_probe_volume(z, np.zeros((2, 3)), V(c)), "2 normals for 3 positions"),
                       (lambda: g.lookup_probe_volume(z, np.zeros((2, 3)), V(c)), "3 origins for 2 directions"),
                       (lambda: g.lookup_probe_volume(z.astype(np.float32), z, V(c)), r"origins must be an \(n, 3\) float64 array"),
                       (lambda: g.sample_probe_volume(z, z, V(np.zeros((3, 2, 2, 9, 3)))), r"volume.coeffs must be a \(nz, ny, nx, 9, 3\)"),
                       (lambda: g.sample_probe_volume(z, z, V(np.zeros((12, 27)))), r"volume.coeffs must be a \(nz, ny, nx, 9, 3\)"),
                       (lambda: g.sample_probe_volume(z, z, V(c.astype(np.float32))), "volume.coeffs must be a C-contiguous"),
                       (lambda: g.lookup_probe_volume(z, z, V(c, np.zeros((3, 2, 2), dtype=bool))), r"volume.valid must be a \(nz, ny, nx\)"),
                       (lambda: g.lookup_probe_volume(z, z, V(c, np.zeros((2, 2, 3)))), r"volume.valid must be a \(2, 2, 3\) uint8 or bool"),
                       (lambda: g.render_views_probe_lit([cam], 4, 3, [], V(c), seed=1, filter="cubic"), 'filter must be "nearest" or "bilinear"'),
                       (lambda: g.render_views_probe_lit([cam], 4, 3, [], V(np.zeros((5, 9, 3))), seed=1), "volume.coeffs must be a")):
        with pytest.raises(ValueError, match=word):
            call()
    with pytest.raises(ValueError, match="three entries each"):
        ProbeVolume((0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), c)
    for call, word in ((lambda: g.sample_probe_volume(z, z, V(c)), "null handle"),  # well-formed arrays: the library speaks
                       (lambda: g.sample_probe_volume(z, z, V(c), channels=0), "channels == 0"),
                       (lambda: g.sample_probe_volume(z, z, V(np.zeros((0, 9, 3)), counts=(0, 2, 2))), "a count of 0")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call()
        assert e.value.code == E and word in str(e.value)
    g.handle = None


# ---- the host header
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe_volume_plan_" + request.param) / "probe_volume_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "probe_volume_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover"])
def test_probe_volume_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr


# ---- the model against closed forms
def unit(rs, n):
    v = rs.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_positions_follow_the_index_rule():
    origin, spacing, counts = (-1.0, 0.5, 2.0), (0.7, 1.3, 0.45), (4, 2, 3)
    pos = ProbeVolume.positions(origin, spacing, counts)
    assert pos.shape == (24, 3) and pos.dtype == np.float64
    for k in range(3):
        for j in range(2):
            for i in range(4):
                p = (k * 2 + j) * 4 + i
                assert M.same(pos[p], np.array([origin[0] + i * spacing[0], origin[1] + j * spacing[1], origin[2] + k * spacing[2]]))
    assert ProbeVolume.positions(origin, spacing, (1, 1, 1)).tolist() == [list(origin)]


def test_constant_radiance_gives_pi_times_it_everywhere():
    """coeffs[.][0] = c * sqrt(4 pi), the rest 0: every tap holds the same value, the weights sum to ws and E = A_0 Y_0 c sqrt(4 pi)
    = pi c; the sums' roundings are a few 1e-16"""
    rs = np.random.RandomState(1)
    c = np.array([0.25, 1.0, 3.5])
    coeffs = np.zeros((3, 2, 4, 9, 3))
    coeffs[..., 0, :] = c * np.sqrt(4.0 * np.pi)
    vol = ProbeVolume((-1.0, 0.5, 2.0), (0.7, 1.3, 0.45), (4, 2, 3), coeffs)
    pos = rs.uniform(-3.0, 6.0, (500, 3))       # inside and far outside: clamped
    got = PV.sample(vol, pos, unit(rs, 500), 0.2)
    assert got["covered"].all() and got["inside"].any() and not got["inside"].all()
    assert (np.abs(got["value"] - np.pi * c) <= 1e-14 * np.pi * c).all()


def test_at_a_probes_own_position_the_model_is_sh9_irradiance():
    """bias 0: the probe's own weight is 1 and the others 0 up to the rounding of (o + i h - o) / h, so the value is
    sh9_irradiance of the probe's coefficients up to the order of the nine terms' summation.  The issue's 1e-13 relative is taken
    against the ABSOLUTE SUM of the nine terms |A_j Y_j c_j|, not against the value: two orders of summation differ by roundings
    of the terms, however much of them cancels"""
    rs = np.random.RandomState(2)
    counts = (3, 2, 2)
    coeffs = rs.uniform(-1.0, 1.0, (12, 9, 3))
    origin, spacing = (0.0, -2.0, 1.0), (0.5, 1.0, 0.25)   # (exactly representable steps: the cell's fraction is an exact 0)
    vol = ProbeVolume(origin, spacing, counts, coeffs)
    pos = ProbeVolume.positions(origin, spacing, counts)
    nrm = unit(rs, 12)
    got = PV.sample(vol, pos, nrm, 0.0)
    want = sh9_irradiance(coeffs, nrm)
    terms = np.abs(rpt_amd.sh9_basis(nrm)[:, :, None] * np.array(PV.A)[None, :, None] * coeffs).sum(axis=1)
    assert got["covered"].all() and got["inside"].all()
    assert (np.abs(got["value"] - want) <= 1e-13 * terms).all()
    assert np.abs(want).max() > 0.1


def test_coefficients_affine_in_position_are_reproduced_inside_the_grid():
    """trilinear interpolation is exact for a field affine in position; with N = (0, 0, 1) only Y_0 and Y_2 and Y_6 are non-zero,
    so E = sum_j B_j * (a_j + g_j . P): within 1e-13 of the terms' absolute sum"""
    rs = np.random.RandomState(3)
    origin, spacing, counts = (-1.0, 0.5, 2.0), (0.7, 1.3, 0.45), (4, 3, 5)
    pos = ProbeVolume.positions(origin, spacing, counts)
    a, g = rs.uniform(-1.0, 1.0, (9, 3)), rs.uniform(-1.0, 1.0, (9, 3, 3))
    field = lambda P: a[None] + np.einsum("jcd,nd->njc", g, P)
    vol = ProbeVolume(origin, spacing, counts, field(pos))
    top = np.array(origin) + (np.array(counts) - 1) * np.array(spacing)
    P = rs.uniform(origin, top, (400, 3))
    nrm = unit(rs, 400)
    got = PV.sample(vol, P, nrm, 0.0)
    B = rpt_amd.sh9_basis(nrm) * np.array(PV.A)
    want = np.einsum("nj,njc->nc", B, field(P))
    scale = np.abs(B[:, :, None] * (np.abs(a)[None] + np.einsum("jcd,nd->njc", np.abs(g), np.abs(P)))).sum(axis=1)
    assert got["covered"].all() and got["inside"].all()
    assert (np.abs(got["value"] - want) <= 1e-13 * scale).all()


def test_one_probe_along_x_gives_a_zero_fraction_everywhere():
    rs = np.random.RandomState(4)
    coeffs = rs.uniform(-1.0, 1.0, (3, 2, 1, 9, 3))
    vol = ProbeVolume((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 2, 3), coeffs)
    q = np.concatenate([rs.uniform(-5.0, 5.0, 100), [0.0, np.nan, np.inf, -np.inf]])
    f, i0, i1, inside = PV.cell(q, 0.0, 1.0, 1)
    assert M.same(f, np.zeros(104)) and (i0 == 0).all() and (i1 == 0).all() and inside.sum() == 1
    # ... so x does not matter: the value at (x, y, z) is the value at (0, y, z)
    P = rs.uniform(0.0, 1.0, (50, 3)) * np.array([9.0, 1.0, 2.0])
    nrm = unit(rs, 50)
    assert M.same(PV.sample(vol, P, nrm)["value"], PV.sample(vol, P * np.array([0.0, 1.0, 1.0]), nrm)["value"])


def test_the_masks_the_fallback_the_facing_and_the_cut():
    rs = np.random.RandomState(5)
    coeffs = rs.uniform(-1.0, 1.0, (2, 2, 2, 9, 3))
    P, nrm = rs.uniform(0.1, 0.9, (20, 3)), unit(rs, 20)
    V = lambda valid: ProbeVolume((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), coeffs, valid)
    none = PV.sample(V(np.zeros(8, dtype=np.uint8)), P, nrm, 0.0, (9.0, 8.0, 7.0))
    assert not none["covered"].any() and none["inside"].all() and M.same(none["value"], np.tile([9.0, 8.0, 7.0], (20, 1)))
    one = np.zeros(8, dtype=np.uint8)
    one[5] = 1                                   # one valid tap: w * C / w
    got = PV.sample(V(one), P, nrm)
    c5 = coeffs.reshape(8, 9, 3)[5]
    terms5 = np.abs(rpt_amd.sh9_basis(nrm)[:, :, None] * np.array(PV.A)[None, :, None] * c5[None]).sum(axis=1)
    assert got["covered"].all() and (np.abs(got["value"] - sh9_irradiance(c5, nrm)) <= 1e-13 * terms5).all()
    bad = coeffs.copy()
    bad.reshape(8, 9, 3)[2, 4, 1] = np.nan       # a NaN coefficient reaches every value whose taps include it, valid or not
    sick = ProbeVolume((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), bad, one)
    assert np.isnan(PV.sample(sick, P, nrm)["value"][:, 1]).all()
    assert not PV.sample(V(None), np.array([[np.nan, 0.5, 0.5]]), nrm[:1])["covered"][0]
    # the facing: the normal is negated where it looks along the ray; a miss is zero, not covered, not inside
    n = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    d = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, -2.0], [1.0, 0.0, 0.0]])
    assert M.same(PV.face(n, d), np.array([[-0.0, -0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]))
    hits = {"t": np.array([1.0, np.inf]), "object": np.array([3, -1], dtype=np.int32), "normal": n[:2],
            "position": np.array([[0.5, 0.5, 0.5], [0.0, 0.0, 0.0]])}
    look = PV.lookup(V(None), d[:2], hits, 0.0, (9.0, 8.0, 7.0))
    assert list(look["covered"]) == [1, 0] and list(look["inside"]) == [1, 0] and M.same(look["value"][1], np.array([9.0, 8.0, 7.0]))
    assert M.same(look["normal"], np.array([[-0.0, -0.0, -1.0], [0.0, 0.0, 0.0]])) and M.same(look["position"][1], np.zeros(3))
    # the views' irradiance: the lightmap first, else the volume cut at zero, else neither
    cov, val, branch = PV.irradiance(np.array([1, 0, 0]), np.full((3, 3), 2.0), np.array([1, 1, 0]), np.array([[5.0] * 3, [-1.0, 0.5, -0.0], [4.0] * 3]))
    assert list(cov) == [1, 1, 0] and list(branch) == [0, 1, 2] and M.same(val[:2], np.array([[2.0] * 3, [0.0, 0.5, -0.0]]))
