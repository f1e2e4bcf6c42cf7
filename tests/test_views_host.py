"""rptgpu_render_views without a GPU: the two symbols and the layouts of RptView / RptViewQuery against the header, every
refusal that comes before the device with its code and detail and untouched outputs, no CPU fallback, and what
GpuScene.render_views lowers its arguments to."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import Camera, View, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
Q_FIELDS = ("struct_size", "width", "height", "max_bounces", "iterations", "_pad", "exposure_value", "seed", "seed_stride",
            "sample_index_base", "precision_mode", "flags")
V_FIELDS = ("camera", "projection", "_pad", "ortho_scale")
PERSP, ORTHO, PANO = _abi.RPT_VIEW_PERSPECTIVE, _abi.RPT_VIEW_ORTHOGRAPHIC, _abi.RPT_VIEW_PANORAMA


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert hasattr(lib, "rptgpu_render_views") and hasattr(lib, "rptgpu_render_views_device")
    assert {"rptgpu_render_views", "rptgpu_render_views_device"} <= {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){' \
          'printf("%zu %zu", sizeof(RptView), sizeof(RptViewQuery));' + \
          "".join('printf(" %%zu", offsetof(RptView, %s));' % f for f in V_FIELDS) + \
          "".join('printf(" %%zu", offsetof(RptViewQuery, %s));' % f for f in Q_FIELDS) + \
          'printf(" %d %d %d\\n", RPT_VIEW_PERSPECTIVE, RPT_VIEW_ORTHOGRAPHIC, RPT_VIEW_PANORAMA);return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(_abi.RptView) == nums[0] == 112 and C.sizeof(_abi.RptViewQuery) == nums[1] == 64
    assert [getattr(_abi.RptView, f).offset for f in V_FIELDS] == nums[2:2 + len(V_FIELDS)]
    assert [getattr(_abi.RptViewQuery, f).offset for f in Q_FIELDS] == nums[2 + len(V_FIELDS):-3]
    assert [f for f, _ in _abi.RptView._fields_] == list(V_FIELDS)
    assert [f for f, _ in _abi.RptViewQuery._fields_] == list(Q_FIELDS)
    assert [PERSP, ORTHO, PANO] == nums[-3:] == [0, 1, 2]
    assert (rpt_amd.RPT_VIEW_PERSPECTIVE, rpt_amd.RPT_VIEW_ORTHOGRAPHIC, rpt_amd.RPT_VIEW_PANORAMA) == (0, 1, 2)


def _query(**kw):
    q = _abi.RptViewQuery()
    q.struct_size, q.width, q.height, q.max_bounces, q.iterations = C.sizeof(_abi.RptViewQuery), 5, 3, 2, 4
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _view(projection=PERSP, ortho_scale=0.0, aperture=0.0):
    v = View(Camera(aperture=aperture, focal_distance=1.0), projection, ortho_scale).lower()
    return v


PERSISTENT = ("RptViewQuery: RPT_FLAG_PERSISTENT — the persistent kernel renders one camera's frame; a batch of views runs the "
              "wavefront pipeline only").encode()
SIZE = b"RptViewQuery: struct_size is not sizeof(RptViewQuery)"
ZERO = b"RptViewQuery: width, height and iterations must be non-zero"
PROJ = b"RptView: unknown projection (RPT_VIEW_PERSPECTIVE = 0, RPT_VIEW_ORTHOGRAPHIC = 1, RPT_VIEW_PANORAMA = 2)"
SCALE = b"RptView: RPT_VIEW_ORTHOGRAPHIC needs a finite ortho_scale > 0"
LENS = "RptView: aperture > 0 — only RPT_VIEW_PERSPECTIVE has a lens".encode()
SMALL = b"RptView: RPT_VIEW_PANORAMA needs width >= 2 and height >= 2"
# (name, the call's arguments — q, views: the two views of the call or False for NULL, out: False for NULL, n —, detail)
REFUSALS = [
    ("no query", dict(q=None), b"null RptViewQuery"),
    ("size 0", dict(q=_query(struct_size=0)), SIZE),
    ("size 56", dict(q=_query(struct_size=56)), SIZE),
    ("size 72", dict(q=_query(struct_size=72)), SIZE),
    ("width 0", dict(q=_query(width=0)), ZERO),
    ("height 0", dict(q=_query(height=0)), ZERO),
    ("iterations 0", dict(q=_query(iterations=0)), ZERO),
    ("bounces", dict(q=_query(max_bounces=255)), b"RptViewQuery: max_bounces > 254"),
    ("mode", dict(q=_query(precision_mode=1)),
     b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"),
    ("persistent", dict(q=_query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("projection 3", dict(views=[_view(), _view(3)]), PROJ),
    ("projection 2^32 - 1", dict(views=[_view(0xffffffff), _view()]), PROJ),
    ("ortho, scale 0", dict(views=[_view(), _view(ORTHO, 0.0)]), SCALE),
    ("ortho, scale < 0", dict(views=[_view(ORTHO, -1.0), _view()]), SCALE),
    ("ortho, scale inf", dict(views=[_view(), _view(ORTHO, math.inf)]), SCALE),
    ("ortho, scale nan", dict(views=[_view(), _view(ORTHO, math.nan)]), SCALE),
    ("ortho, lens", dict(views=[_view(), _view(ORTHO, 1.0, aperture=0.1)]), LENS),
    ("panorama, lens", dict(views=[_view(PANO, aperture=0.1), _view()]), LENS),
    ("panorama, width 1", dict(q=_query(width=1), views=[_view(), _view(PANO)]), SMALL),
    ("panorama, height 1", dict(q=_query(height=1), views=[_view(), _view(PANO)]), SMALL),
    ("2^32 + 2^16 pixels", dict(q=_query(width=1 << 16, height=(1 << 16) + 1)),
     b"RptViewQuery: width * height > 2^32 (a pixel is a 32-bit stream id)"),
    ("2^58 views", dict(n=1 << 58), b"n_views * width * height does not fit: the frames would not fit any memory"),
    ("2^64 - 1 views", dict(n=(1 << 64) - 1), b"n_views * width * height does not fit: the frames would not fit any memory"),
    ("views", dict(views=False), b"null argument"),
    ("out", dict(out=False), b"null argument"),
    ("handle", dict(), b"null handle"),
    ("handle, every projection", dict(views=[_view(ORTHO, 2.5), _view(PANO)]), b"null handle"),
    ("handle, a lens", dict(views=[_view(aperture=0.1), _view()]), b"null handle"),
    ("handle, 2^32 pixels", dict(q=_query(width=1 << 16, height=1 << 16), n=0, views=False, out=False), b"null handle"),
    ("handle, no views", dict(n=0, views=False, out=False), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_every_refusal_comes_before_the_device(row, device):
    """... so each of them is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    q = kw.get("q", _query())
    views = kw.get("views", [_view(), _view()])
    arr = (_abi.RptView * 2)(*views) if views else None
    keep = bytes(arr) if arr is not None else None
    out = np.full(2 * 5 * 3 * 3, 7.0) if kw.get("out", True) else None
    n = kw.get("n", 2)
    # a call with another detail first: the text below is this call's
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    qp = C.byref(q) if q is not None else None
    if device:  # (a pointer that is never followed: every row is refused before the device is looked at)
        rc = lib.rptgpu_render_views_device(None, n, arr, qp, C.c_void_p(out.ctypes.data) if out is not None else None, 0, None)
    else:
        rc = lib.rptgpu_render_views(None, n, arr, qp, out.ctypes.data_as(PD) if out is not None else None)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert out is None or (out == 7).all()
    assert arr is None or bytes(arr) == keep


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never frames from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    views = [camera, View.orthographic(camera, 2.0), View.panorama((0.0, 0.0, 5.0))]
    if gpu_available:
        out = rpt_amd.GpuScene(scene).render_views(views, 9, 5, 2, samples=2)
        assert out.shape == (3, 5, 9, 3) and np.isfinite(out).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).render_views(views, 9, 5, 2, samples=2)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


class _Spy:
    """stands where the library stands: keeps what GpuScene.render_views hands rptgpu_render_views"""

    def __init__(self):
        self.calls = []

    def rptgpu_render_views(self, handle, n, arr, q, out):
        q = q._obj
        self.calls.append((handle, n, [bytes(arr[i]) for i in range(n)], {f: getattr(q, f) for f in Q_FIELDS}))
        return 0


def test_python_lowering():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: nothing here reaches a device
    g.lib, g.handle, g.device = _Spy(), None, 0
    cam = Camera.look_at((1.0, 2.0, 3.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 0.6).focus((0.0, 0.5, 0.0), 0.25)
    raw = _abi.RptView()
    raw.camera, raw.projection, raw.ortho_scale = cam.lower(), ORTHO, 1.5
    views = [cam, View(cam), View.orthographic(cam, 3.25), View.panorama((4.0, 5.0, 6.0)), raw]
    out = g.render_views(views, 7, 4, 3, samples=2, seed=11, seed_stride=5, sample_index_base=9, exposure_value=0.5,
                         flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert out.shape == (5, 4, 7, 3) and out.dtype == np.float64
    (_, n, recs, q), = g.lib.calls
    assert n == 5
    got = [_abi.RptView.from_buffer_copy(r) for r in recs]
    assert [v.projection for v in got] == [PERSP, PERSP, ORTHO, PANO, ORTHO]
    assert [v.ortho_scale for v in got] == [0.0, 0.0, 3.25, 0.0, 1.5]
    assert all(v._pad == 0 for v in got)
    assert recs[0] == recs[1]  # a Camera is the perspective view of itself
    for v in (got[0], got[2], got[4]):
        assert bytes(v.camera) == bytes(cam.lower())
    assert list(got[3].camera.eye) == [4.0, 5.0, 6.0] and got[3].camera.aperture == 0.0
    assert q == dict(struct_size=64, width=7, height=4, max_bounces=3, iterations=2, _pad=0, exposure_value=0.5, seed=11,
                     seed_stride=5, sample_index_base=9, precision_mode=_abi.RPT_PRECISION_F64_STRICT,
                     flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    same = np.zeros((5, 4, 7, 3))
    assert g.render_views(views, 7, 4, 3, out=same) is same
    assert g.render_views([], 7, 4, 3).shape == (0, 4, 7, 3)
    with pytest.raises(ValueError, match="out must be"):
        g.render_views(views, 7, 4, 3, out=np.zeros((5, 7, 4, 3)))
    with pytest.raises(ValueError, match="out must be"):
        g.render_views(views, 7, 4, 3, out=np.zeros((5, 4, 7, 3), dtype=np.float32))
    with pytest.raises(TypeError, match="view 1 is a tuple"):
        g.render_views([cam, (1.0, 2.0, 3.0)], 7, 4, 3)
    g.lib = _abi.load_library()  # well-formed arguments: the library speaks (no handle)
    with pytest.raises(rpt_amd.RptGpuError) as e:
        g.render_views([cam, View.orthographic(Camera(), 2.0), View.panorama((0.0, 0.0, 0.0))], 7, 4, 3)
    assert e.value.code == E and "null handle" in str(e.value)
    with pytest.raises(rpt_amd.RptGpuError) as e:  # ... about the views, too: a lens under an orthographic projection
        g.render_views(views, 7, 4, 3)
    assert e.value.code == E and "only RPT_VIEW_PERSPECTIVE has a lens" in str(e.value)
