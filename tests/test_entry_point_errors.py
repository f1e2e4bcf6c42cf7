"""Every way to be refused by an entry point of api_buffer / api_aov / api_render / api_particles / api_scene that needs no
device: null handles and buffers, null and mis-sized structs, bad channel masks, zero sizes.  One table of (call, return
code, rptgpu_last_error_detail text); the drivers behind these entry points share their frame (api_internal.h
guarded()), and this table is what holds the codes and texts still while that frame changes.

A call that returns a bare code without a detail leaves the thread's detail as it was: every row first makes a call
with a known detail (SENTINEL) and expects None where that text is still there afterwards."""
import ctypes as C

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi

OK = _abi.RPTGPU_OK
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
SENTINEL = b"more than RPT_PARTICLES_MAX_N arguments"
N = 64


def _pd(a):
    return a.ctypes.data_as(PD)


class Args:
    """the arguments the rows draw from; every output array starts as 7 and must end as 7"""

    def __init__(self):
        self.cam = _abi.RptCamera()
        self.f64 = np.full(3 * N, 7.0)
        self.u32 = np.full(N, 7, dtype=np.uint32)
        self.i32 = np.full(N, 7, dtype=np.int32)
        self.u8 = np.full(3 * N, 7, dtype=np.uint8)
        self.out_u32 = C.c_uint32(7)
        self.out_ptr = C.c_void_p(None)
        self.tree = _abi.RptKdTree()

    def params(self, **kw):
        p = rpt_amd.make_params(8, 8, 1, 2)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def aov(self, **kw):
        b = _abi.RptAovBuffers()
        b.struct_size, b.channels = C.sizeof(b), _abi.RPT_AOV_ALL
        types = dict(_abi.RptAovBuffers._fields_)
        for name in ("hits", "depth", "normal", "albedo", "position", "object"):
            a = self.i32 if name == "object" else self.u32 if name == "hits" else self.f64
            setattr(b, name, a.ctypes.data_as(types[name]))
        for k, v in kw.items():
            setattr(b, k, v)
        return C.byref(b)

    def adaptive(self, **kw):
        a = _abi.RptAdaptive(C.sizeof(_abi.RptAdaptive), 2, 0.01, 0.05)
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    def denoise(self, **kw):
        d = _abi.RptDenoise(C.sizeof(_abi.RptDenoise), 3, 2.0, 0.1, 0.01, 0.1)
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    def system(self, kind=_abi.RPT_PARTICLES_MARBLES, flags=0):
        return C.byref(_abi.RptParticleSystem(kind, flags, 0.5))

    def untouched(self):
        return ((self.f64 == 7).all() and (self.u32 == 7).all() and (self.i32 == 7).all() and (self.u8 == 7).all()
                and self.out_u32.value == 7)


NAN, INF = float("nan"), float("inf")
BIG = _abi.RPT_PARTICLES_MAX_N + 1
SINGLE, GRID = _abi.RPT_PARTICLES_FLAG_SINGLE_GROUP, _abi.RPT_PARTICLES_FLAG_GRID
AOV_SIZE = b"RptAovBuffers: struct_size is not sizeof(RptAovBuffers)"
ADAPTIVE_TOL = b"RptAdaptive: abs_tol and rel_tol must be finite and >= 0"
DENOISE_SIGMA = b"RptDenoise: every sigma must be finite and > 0"
BAD_MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
NULL_ARRAY = b"NULL array with n > 0"


def _aov_rows(fn, lead):
    """the refusals of bad_aov, which rptgpu_render_aov and rptgpu_buffer_feature_sums make first; lead: the arguments
    in front of the RptAovBuffers"""
    null = lambda t: C.cast(None, dict(_abi.RptAovBuffers._fields_)[t])
    rows = [
        (fn, lambda a: (*lead(a), None), E, b"null RptAovBuffers"),
        (fn, lambda a: (*lead(a), a.aov(struct_size=0)), E, AOV_SIZE),
        (fn, lambda a: (*lead(a), a.aov(struct_size=48)), E, AOV_SIZE),
        (fn, lambda a: (*lead(a), a.aov(struct_size=64)), E, AOV_SIZE),
        (fn, lambda a: (*lead(a), a.aov(channels=32)), E, b"RptAovBuffers: channels names an unknown RPT_AOV_* bit"),
        (fn, lambda a: (*lead(a), a.aov(channels=1 << 31)), E, b"RptAovBuffers: channels names an unknown RPT_AOV_* bit"),
        (fn, lambda a: (*lead(a), a.aov(channels=0, hits=null("hits"))), E, b"RptAovBuffers: hits is NULL (it is always written)"),
    ]
    for name in ("depth", "normal", "albedo", "position", "object"):
        text = ("RptAovBuffers: RPT_AOV_%s is named but %s is NULL" % (name.upper(), name)).encode()
        rows.append((fn, lambda a, name=name: (*lead(a), a.aov(**{name: null(name)})), E, text))
    return rows


ROWS = [
    # ---- api_buffer.cpp
    ("rptgpu_buffer_create", lambda a: (None, 8, 8, 0, C.byref(a.out_ptr)), E, b"bad argument"),
    ("rptgpu_buffer_create", lambda a: (None, 0, 0, 0, None), E, b"bad argument"),
    ("rptgpu_buffer_destroy", lambda a: (None,), None, None),
    ("rptgpu_buffer_sample", lambda a: (None, C.byref(a.cam), a.params()), E, None),
    ("rptgpu_buffer_sample", lambda a: (None, None, None), E, None),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), None, C.byref(a.out_u32)), E, b"null RptAdaptive"),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(struct_size=0), C.byref(a.out_u32)), E,
     b"RptAdaptive: struct_size is not sizeof(RptAdaptive)"),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(struct_size=32), C.byref(a.out_u32)), E,
     b"RptAdaptive: struct_size is not sizeof(RptAdaptive)"),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(min_batches=1), C.byref(a.out_u32)), E,
     b"RptAdaptive: min_batches < 2"),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(min_batches=0), C.byref(a.out_u32)), E,
     b"RptAdaptive: min_batches < 2"),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(abs_tol=NAN), C.byref(a.out_u32)), E, ADAPTIVE_TOL),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(abs_tol=-1.0), C.byref(a.out_u32)), E, ADAPTIVE_TOL),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(rel_tol=INF), C.byref(a.out_u32)), E, ADAPTIVE_TOL),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, C.byref(a.cam), a.params(), a.adaptive(), C.byref(a.out_u32)), E, b"null argument"),
    ("rptgpu_buffer_sample_adaptive", lambda a: (None, None, None, a.adaptive(), None), E, b"null argument"),
    ("rptgpu_buffer_sample_counts", lambda a: (None, a.u32.ctypes.data_as(C.POINTER(C.c_uint32))), E, None),
    ("rptgpu_buffer_sample_counts", lambda a: (None, None), E, None),
    ("rptgpu_buffer_totals", lambda a: (None, _pd(a.f64)), E, None),
    ("rptgpu_buffer_totals", lambda a: (None, None), E, None),
    ("rptgpu_buffer_image", lambda a: (None, a.u8.ctypes.data_as(C.POINTER(C.c_uint8))), E, None),
    ("rptgpu_buffer_image", lambda a: (None, None), E, None),
    ("rptgpu_buffer_variance", lambda a: (None, _pd(a.f64)), E, None),
    ("rptgpu_buffer_variance", lambda a: (None, None), E, None),
    ("rptgpu_buffer_num_batches", lambda a: (None, C.byref(a.out_u32)), E, None),
    ("rptgpu_buffer_num_batches", lambda a: (None, None), E, None),
    ("rptgpu_buffer_features", lambda a: (None, C.byref(a.cam), a.params()), E, b"null buffer"),
    ("rptgpu_buffer_features", lambda a: (None, None, None), E, b"null buffer"),
    *_aov_rows("rptgpu_buffer_feature_sums", lambda a: (None,)),
    ("rptgpu_buffer_feature_sums", lambda a: (None, a.aov()), E,
     b"RptAovBuffers: RPT_AOV_OBJECT is named, but a buffer does not hold `object`"),
    ("rptgpu_buffer_feature_sums", lambda a: (None, a.aov(channels=15)), E, b"null buffer"),
    ("rptgpu_buffer_feature_sums", lambda a: (None, a.aov(channels=0)), E, b"null buffer"),
    ("rptgpu_buffer_denoise", lambda a: (None, None, _pd(a.f64), None), E, b"null RptDenoise"),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(struct_size=0), _pd(a.f64), None), E,
     b"RptDenoise: struct_size is not sizeof(RptDenoise)"),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(struct_size=48), _pd(a.f64), None), E,
     b"RptDenoise: struct_size is not sizeof(RptDenoise)"),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(levels=0), _pd(a.f64), None), E, b"RptDenoise: levels outside 1..8"),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(levels=9), _pd(a.f64), None), E, b"RptDenoise: levels outside 1..8"),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(sigma_color=0.0), _pd(a.f64), None), E, DENOISE_SIGMA),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(sigma_normal=NAN), _pd(a.f64), None), E, DENOISE_SIGMA),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(sigma_depth=-1.0), _pd(a.f64), None), E, DENOISE_SIGMA),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(sigma_albedo=INF), _pd(a.f64), None), E, DENOISE_SIGMA),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(), _pd(a.f64), None), E, b"null buffer"),
    ("rptgpu_buffer_denoise", lambda a: (None, a.denoise(), None, None), E, b"null buffer"),
    # ---- api_aov.cpp: the buffers first, then the parameters, the camera, the handle
    *_aov_rows("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params())),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), None, a.aov()), E, b"null params"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(iterations=0), a.aov()), E, b"iterations == 0"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(width=0), a.aov()), E, b"width * height == 0"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(height=0), a.aov()), E, b"width * height == 0"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(width=65536, height=32768), a.aov()), E, b"frame too large"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(part_count=2, part_index=2), a.aov()), E, b"part_index >= part_count"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(precision_mode=1), a.aov()), E, BAD_MODE),
    ("rptgpu_render_aov", lambda a: (None, None, a.params(), a.aov()), E, b"null camera"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(), a.aov()), E, b"null handle"),
    ("rptgpu_render_aov", lambda a: (None, C.byref(a.cam), a.params(), a.aov(channels=0)), E, b"null handle"),
    # ---- api_render.cpp
    ("rptgpu_render_batch", lambda a: (None, C.byref(a.cam), a.params(), None), E, b"null out_rgb"),
    ("rptgpu_render_batch", lambda a: (None, C.byref(a.cam), a.params(), _pd(a.f64)), E, b"null argument"),
    ("rptgpu_render_batch", lambda a: (None, None, None, _pd(a.f64)), E, b"null argument"),
    ("rptgpu_render_batch_device", lambda a: (None, C.byref(a.cam), a.params(), None, 0, None), E, b"null d_out"),
    ("rptgpu_render_batch_device", lambda a: (None, C.byref(a.cam), a.params(), a.f64.ctypes.data, 0, None), E, b"null argument"),
    ("rptgpu_render_batch_device", lambda a: (None, None, None, a.f64.ctypes.data, 1, None), E, b"null argument"),
    ("rptgpu_closest_hit", lambda a: (None, 4, _pd(a.f64), _pd(a.f64), 0, _pd(a.f64), _pd(a.f64), a.i32.ctypes.data_as(C.POINTER(C.c_int32))),
     E, b"null argument"),
    ("rptgpu_closest_hit", lambda a: (None, 0, None, None, 0, None, None, None), E, b"null argument"),
    ("rptgpu_eval_math", lambda a: (None, 0, 4, _pd(a.f64), _pd(a.f64), _pd(a.f64)), E, b"bad argument"),
    ("rptgpu_eval_math", lambda a: (None, 8, 0, None, None, None), E, b"bad argument"),
    # ---- api_particles.cpp: the system and the size, the schedule, the arrays (all before the device is looked at)
    ("rptgpu_particles_time_derivative", lambda a: (0, None, 4, _pd(a.f64), _pd(a.f64), _pd(a.f64), _pd(a.f64)), E, b"sys is NULL"),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(kind=3), 4, _pd(a.f64), _pd(a.f64), _pd(a.f64), _pd(a.f64)), E,
     b"unknown particle system kind"),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(flags=4), 4, _pd(a.f64), _pd(a.f64), _pd(a.f64), _pd(a.f64)), E,
     b"unknown RPT_PARTICLES_FLAG_* bit"),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(flags=SINGLE | GRID), 4, _pd(a.f64), _pd(a.f64), _pd(a.f64), _pd(a.f64)), E,
     b"both schedules forced (RPT_PARTICLES_FLAG_SINGLE_GROUP | _GRID)"),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(flags=SINGLE), 2049, _pd(a.f64), _pd(a.f64), _pd(a.f64), _pd(a.f64)), E,
     b"the single-workgroup schedule takes at most RPT_PARTICLES_SINGLE_MAX particles"),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(), BIG, _pd(a.f64), _pd(a.f64), _pd(a.f64), _pd(a.f64)), E,
     b"more than RPT_PARTICLES_MAX_N particles (the kernels index 3n in 32 bits)"),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(), 0, None, None, None, None), OK, None),
    ("rptgpu_particles_time_derivative", lambda a: (-5, a.system(), 0, None, None, None, None), OK, None),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(), 4, _pd(a.f64), _pd(a.f64), _pd(a.f64), None), E, NULL_ARRAY),
    ("rptgpu_particles_time_derivative", lambda a: (0, a.system(), 4, None, _pd(a.f64), _pd(a.f64), _pd(a.f64)), E, NULL_ARRAY),
    ("rptgpu_particles_integrate", lambda a: (0, None, 4, _pd(a.f64), _pd(a.f64), 1.0, 0.1), E, b"sys is NULL"),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(kind=7), 4, _pd(a.f64), _pd(a.f64), 1.0, 0.1), E, b"unknown particle system kind"),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 4, _pd(a.f64), _pd(a.f64), NAN, 0.1), E, b"time is not finite"),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 4, _pd(a.f64), _pd(a.f64), INF, 0.1), E, b"time is not finite"),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 4, _pd(a.f64), _pd(a.f64), 1.0, 0.0), E,
     b"step must be finite and > 0 (the reference loops for ever otherwise)"),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 4, _pd(a.f64), _pd(a.f64), 1.0, NAN), E,
     b"step must be finite and > 0 (the reference loops for ever otherwise)"),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 4, _pd(a.f64), _pd(a.f64), 1e17, 1.0), E,
     b"time / step exceeds RPT_PARTICLES_MAX_STEPS"),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 0, None, None, 1.0, 0.1), OK, None),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 4, None, _pd(a.f64), 1.0, 0.1), E, NULL_ARRAY),
    ("rptgpu_particles_integrate", lambda a: (0, a.system(), 4, _pd(a.f64), None, 1.0, 0.1), E, NULL_ARRAY),
    ("rptgpu_monomial_closest_point", lambda a: (0, 1.0, 0, 4, _pd(a.f64), _pd(a.f64)), E, b"steps must be in 1..2^24"),
    ("rptgpu_monomial_closest_point", lambda a: (0, 1.0, (1 << 24) + 1, 4, _pd(a.f64), _pd(a.f64)), E, b"steps must be in 1..2^24"),
    ("rptgpu_monomial_closest_point", lambda a: (0, 1.0, 16, BIG, _pd(a.f64), _pd(a.f64)), E, b"more than RPT_PARTICLES_MAX_N points"),
    ("rptgpu_monomial_closest_point", lambda a: (0, 1.0, 16, 0, None, None), OK, None),
    ("rptgpu_monomial_closest_point", lambda a: (0, 1.0, 16, 4, None, _pd(a.f64)), E, NULL_ARRAY),
    ("rptgpu_monomial_closest_point", lambda a: (0, 1.0, 16, 4, _pd(a.f64), None), E, NULL_ARRAY),
    ("rptgpu_particles_eval_hypot", lambda a: (0, 0, None, None, None), OK, None),
    ("rptgpu_particles_eval_hypot", lambda a: (0, 4, _pd(a.f64), _pd(a.f64), None), E, NULL_ARRAY),
    ("rptgpu_particles_eval_hypot", lambda a: (0, 4, None, _pd(a.f64), _pd(a.f64)), E, NULL_ARRAY),
    # ---- api_scene.cpp: the live updates and the kd-tree builds
    ("rptgpu_scene_set_objects", lambda a: (None, 0, None, None), E, b"rptgpu_scene_set_objects: null handle"),
    ("rptgpu_scene_set_objects", lambda a: (None, 1, a.u32.ctypes.data_as(C.POINTER(C.c_uint32)), None), E,
     b"rptgpu_scene_set_objects: null handle"),
    ("rptgpu_scene_set_lights", lambda a: (None, 0, None, None), E, b"rptgpu_scene_set_lights: null handle"),
    ("rptgpu_scene_set_lights", lambda a: (None, 1, a.u32.ctypes.data_as(C.POINTER(C.c_uint32)), None), E,
     b"rptgpu_scene_set_lights: null handle"),
    ("rptgpu_kdtree_build", lambda a: (None, 1, C.byref(a.tree)), E, None),
    ("rptgpu_kdtree_build", lambda a: (_pd(a.f64), 1, None), E, None),
    ("rptgpu_kdtree_build_device", lambda a: (None, 1, 0, C.byref(a.tree)), E, None),
    ("rptgpu_kdtree_build_device", lambda a: (_pd(a.f64), 1, 0, None), E, None),
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=["%s-%d" % (r[0][len("rptgpu_"):], i) for i, r in enumerate(ROWS)])
def test_code_and_detail(row):
    name, make, code, detail = ROWS[row]
    lib = _abi.load_library()
    a = Args()
    assert lib.rptgpu_particles_eval_hypot(0, BIG, None, None, None) == E
    assert lib.rptgpu_last_error_detail(None) == SENTINEL
    rc = getattr(lib, name)(*make(a))
    got = lib.rptgpu_last_error_detail(None)
    assert rc == code
    assert (None if got == SENTINEL else got) == detail
    assert a.untouched() and not a.out_ptr.value


def test_the_table_names_every_entry_point_of_the_shared_frame():
    """... so that a new entry point of these files comes with its rows"""
    want = {s[0] for s in _abi.SYMBOLS if s[0].startswith(("rptgpu_buffer_", "rptgpu_particles_", "rptgpu_render_aov"))}
    want |= {"rptgpu_render_batch", "rptgpu_render_batch_device", "rptgpu_closest_hit", "rptgpu_eval_math",
             "rptgpu_monomial_closest_point", "rptgpu_scene_set_objects", "rptgpu_scene_set_lights", "rptgpu_kdtree_build",
             "rptgpu_kdtree_build_device"}
    assert {r[0] for r in ROWS} == want
