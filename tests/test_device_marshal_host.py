"""What GpuScene's array-taking methods hand the library, without a GPU: a recording stand-in takes the library's place,
and each method is held to the symbol it calls, the number of its arguments, which pointers are NULL and which are the
addresses of the caller's (or the returned) arrays, every field of its query struct, and the shapes and dtypes it
returns.  The second half holds the refusals of torch tensors that are not on the handle's device: they come before any
library call and before torch's current stream is asked for."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import Camera, GpuScene, KdTree, Object, Scene, View, _abi, cube, make_params, sphere, transform_records
from rpt_amd.scene import geometry_snapshot

STRICT = _abi.RPT_PRECISION_F64_STRICT
HANDLE = 0x1234


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


def _children(n=4):
    return [(cube() if i % 2 else sphere()).scale((0.5, 0.25, 2.0)).translate((float(i), 0.5, -1.0)) for i in range(n)]


def wrapper():
    g = GpuScene.__new__(GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(HANDLE), 0
    s = Scene()
    s.add(Object(sphere()))
    s.add(Object(KdTree(_children())))
    g._geometry = geometry_snapshot(s)
    return g


def the_call(g, name, argc):
    """the one call the method made: its arguments behind the handle"""
    assert len(g.lib.calls) == 1, [c[0] for c in g.lib.calls]
    got, args = g.lib.calls.pop()
    assert got == name and len(args) == argc, (got, len(args))
    assert args[0] is g.handle
    return args[1:]


def address(p):
    """a pointer argument's address, None for NULL"""
    if p is None:
        return None
    return p.value if isinstance(p, C.c_void_p) else C.cast(p, C.c_void_p).value


def fields(s):
    """every field of a struct that is not a pointer (nested structs as dicts)"""
    s = getattr(s, "_obj", s)
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out[name] = fields(v)
        elif not isinstance(v, C._Pointer):
            out[name] = v
    return out


def pointers(s):
    """{name: address or None} of a struct's pointer fields"""
    s = getattr(s, "_obj", s)
    return {name: address(getattr(s, name)) for name, _ in s._fields_ if isinstance(getattr(s, name), C._Pointer)}


def is_array(a, shape, dtype):
    return isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dtype and a.flags.c_contiguous


def held(struct, arrays, names):
    """the struct's pointers: the named arrays' addresses, NULL for the rest"""
    got = pointers(struct)
    assert set(arrays) == set(names)
    for name, at in got.items():
        assert at == (arrays[name].ctypes.data if name in names else None), name


def rays(n):
    rs = np.random.RandomState(n)
    return rs.uniform(-1.0, 1.0, (n, 3)), rs.uniform(-1.0, 1.0, (n, 3))


NS = pytest.mark.parametrize("n", [3, 0])


# ---- the ray and point calls
@NS
def test_closest_hit(n):
    g = wrapper()
    o, d = rays(n)
    t, nrm, obj = g.closest_hit(o, d)
    cnt, po, pd, precision, pt, pn, pobj = the_call(g, "rptgpu_closest_hit", 8)
    assert cnt == n and precision == STRICT
    assert (address(po), address(pd)) == (o.ctypes.data, d.ctypes.data)
    assert (address(pt), address(pn), address(pobj)) == (t.ctypes.data, nrm.ctypes.data, obj.ctypes.data)
    assert is_array(t, (n,), np.float64) and is_array(nrm, (n, 3), np.float64) and is_array(obj, (n,), np.int32)
    # the call's contract: anything that reshapes to (n, 3) doubles is taken
    g.closest_hit(o.astype(np.float32).ravel(), d.tolist(), precision=1)
    cnt, po, pd, precision = the_call(g, "rptgpu_closest_hit", 8)[:4]
    assert cnt == n and precision == 1
    assert (np.ctypeslib.as_array(po, (max(n, 1), 3))[:n] == o.astype(np.float32)).all()


@NS
def test_trace_rays(n):
    g = wrapper()
    o, d = rays(n)
    got = g.trace_rays(o, d, 5)
    cnt, po, pd, pids, q, pout = the_call(g, "rptgpu_trace_rays", 7)
    assert cnt == n and (address(po), address(pd), pids) == (o.ctypes.data, d.ctypes.data, None)
    assert fields(q) == dict(struct_size=48, max_bounces=5, iterations=1, first_draw=0, exposure_value=0.0, seed=0x52505447,
                             sample_index_base=0, precision_mode=STRICT, flags=0)
    assert is_array(got, (n, 3), np.float64) and address(pout) == got.ctypes.data
    ids = np.arange(n, dtype=np.uint32)
    out = np.empty((n, 3))
    assert g.trace_rays(o, d, 2, samples=3, seed=9, sample_index_base=1 << 40, streams=ids, first_draw=2, exposure_value=1.5,
                        flags=_abi.RPT_FLAG_WAVEFRONT, out=out) is out
    cnt, po, pd, pids, q, pout = the_call(g, "rptgpu_trace_rays", 7)
    assert address(pids) == ids.ctypes.data and address(pout) == out.ctypes.data
    assert fields(q) == dict(struct_size=48, max_bounces=2, iterations=3, first_draw=2, exposure_value=1.5, seed=9,
                             sample_index_base=1 << 40, precision_mode=STRICT, flags=_abi.RPT_FLAG_WAVEFRONT)
    # the call's contract: rays of any dtype and shape that reshape to (n, 3), ids of any dtype and shape that flatten to n
    g.trace_rays(o.astype(np.float32).ravel(), d.tolist(), 1, streams=np.arange(n, dtype=np.float64).reshape(n, 1))
    cnt, po, pd, pids = the_call(g, "rptgpu_trace_rays", 7)[:4]
    assert cnt == n and (np.ctypeslib.as_array(pids, (max(n, 1),))[:n] == ids).all()
    for bad in (np.empty((n, 3), dtype=np.float32), np.empty((n + 1, 3)), np.empty((3, n + 5)).T[:n + 1]):
        with pytest.raises(ValueError, match="out must be"):
            g.trace_rays(o, d, 1, out=bad)
    assert not g.lib.calls


@NS
@pytest.mark.parametrize("kind", [_abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE])
def test_bake_probes(kind, n):
    g = wrapper()
    pos, nrm = rays(n)
    nrm = nrm if kind == _abi.RPT_PROBE_IRRADIANCE else None
    shape = (n, 9, 3) if kind == _abi.RPT_PROBE_SH9 else (n, 3)
    got = g.bake_probes(pos, nrm, kind=kind, samples=4, max_bounces=2, seed=7)
    cnt, ppos, pnrm, pids, q, pout = the_call(g, "rptgpu_bake_probes", 7)
    assert cnt == n and address(ppos) == pos.ctypes.data and pids is None
    assert (pnrm is None) if nrm is None else (address(pnrm) == nrm.ctypes.data)
    assert fields(q) == dict(struct_size=40, kind=kind, samples=4, max_bounces=2, seed=7, sample_index_base=0,
                             precision_mode=STRICT, flags=0)
    assert is_array(got, shape, np.float64) and address(pout) == got.ctypes.data
    ids, out = np.arange(n, dtype=np.uint32), np.empty(shape)
    assert g.bake_probes(pos, nrm, kind=kind, samples=1, max_bounces=0, seed=1, sample_index_base=5, streams=ids,
                         flags=_abi.RPT_FLAG_WAVEFRONT, out=out) is out
    cnt, ppos, pnrm, pids, q, pout = the_call(g, "rptgpu_bake_probes", 7)
    assert address(pids) == ids.ctypes.data and address(pout) == out.ctypes.data
    assert fields(q) == dict(struct_size=40, kind=kind, samples=1, max_bounces=0, seed=1, sample_index_base=5,
                             precision_mode=STRICT, flags=_abi.RPT_FLAG_WAVEFRONT)
    g.bake_probes(pos, nrm, kind=kind, samples=1, max_bounces=0, seed=1, streams=np.arange(n, dtype=np.int64) + (1 << 32))
    pids = the_call(g, "rptgpu_bake_probes", 7)[3]
    assert (np.ctypeslib.as_array(pids, (max(n, 1),))[:n] == ids).all()  # any integer dtype: its low 32 bits
    # the call's contract: (n, 3) float64 and one-dimensional integer ids, nothing else
    for bad in (dict(positions=pos.astype(np.float32)), dict(positions=pos.ravel()), dict(streams=ids.astype(np.float64)),
                dict(streams=ids.reshape(n, 1)), dict(out=np.empty(shape, dtype=np.float32)), dict(out=np.empty((n + 1,) + shape[1:]))):
        kw = dict(positions=pos, normals=nrm, kind=kind, samples=1, max_bounces=0, seed=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            g.bake_probes(**kw)
    assert not g.lib.calls


@NS
def test_occluded(n):
    g = wrapper()
    o, d = rays(n)
    got = g.occluded(o, d)
    cnt, po, pd, pmt, q, pout = the_call(g, "rptgpu_occluded", 7)
    assert cnt == n and (address(po), address(pd), pmt) == (o.ctypes.data, d.ctypes.data, None)
    assert fields(q) == dict(struct_size=16, precision_mode=STRICT, flags=0, reserved=0)
    assert is_array(got, (n,), np.uint8) and address(pout) == got.ctypes.data
    mt, out = np.full(n, 2.5), np.empty(n, dtype=np.uint8)
    assert g.occluded(o, d, max_t=mt, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL, out=out) is out
    cnt, po, pd, pmt, q, pout = the_call(g, "rptgpu_occluded", 7)
    assert address(pmt) == mt.ctypes.data and address(pout) == out.ctypes.data
    assert fields(q) == dict(struct_size=16, precision_mode=STRICT, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL, reserved=0)
    for bad in (dict(origins=o.astype(np.float32)), dict(max_t=mt.astype(np.float32)), dict(max_t=np.zeros(n + 1)),
                dict(out=np.empty(n, dtype=np.int32)), dict(out=np.empty(n + 1, dtype=np.uint8))):
        kw = dict(origins=o, dirs=d)
        kw.update(bad)
        with pytest.raises(ValueError):
            g.occluded(**kw)
    assert not g.lib.calls


@NS
@pytest.mark.parametrize("bent", [False, True])
def test_bake_ao(bent, n):
    g = wrapper()
    pos, nrm = rays(n)
    got = g.bake_ao(pos, nrm, samples=4, seed=3, bent_normals=bent)
    cnt, ppos, pnrm, pids, q, pao, pbent = the_call(g, "rptgpu_bake_ao", 8)
    assert cnt == n and (address(ppos), address(pnrm), pids) == (pos.ctypes.data, nrm.ctypes.data, None)
    assert fields(q) == dict(struct_size=40, samples=4, seed=3, sample_index_base=0, max_distance=float("inf"),
                             precision_mode=STRICT, flags=0)
    ao, bn = got if bent else (got, None)
    assert is_array(ao, (n,), np.float64) and address(pao) == ao.ctypes.data
    assert (is_array(bn, (n, 3), np.float64) and address(pbent) == bn.ctypes.data) if bent else pbent is None
    ids = np.arange(n, dtype=np.uint32)
    out = (np.empty(n), np.empty((n, 3))) if bent else np.empty(n)
    got = g.bake_ao(pos, nrm, samples=1, seed=2, max_distance=3.5, sample_index_base=6, streams=ids, bent_normals=bent,
                    flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL, out=out)
    cnt, ppos, pnrm, pids, q, pao, pbent = the_call(g, "rptgpu_bake_ao", 8)
    assert (got[0] is out[0] and got[1] is out[1]) if bent else got is out
    assert address(pids) == ids.ctypes.data and address(pao) == (out[0] if bent else out).ctypes.data
    assert (address(pbent) == out[1].ctypes.data) if bent else pbent is None
    assert fields(q) == dict(struct_size=40, samples=1, seed=2, sample_index_base=6, max_distance=3.5, precision_mode=STRICT,
                             flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    for bad in (dict(normals=nrm.astype(np.float32)), dict(streams=ids.astype(np.float32)), dict(streams=ids.reshape(1, n)),
                dict(out=np.empty(n + 1)), dict(out=np.empty(n, dtype=np.float32))):
        kw = dict(positions=pos, normals=nrm, samples=1, seed=2, bent_normals=bent)
        kw.update(bad)
        with pytest.raises(ValueError):
            g.bake_ao(**kw)
    assert not g.lib.calls


HIT = {"t": ((), np.float64), "normal": ((3,), np.float64), "object": ((), np.int32), "position": ((3,), np.float64),
       "albedo": ((3,), np.float64)}
SURFACE = {"t": ((), np.float64), "object": ((), np.int32), "child": ((), np.int32), "primitive": ((), np.int32),
           "barycentric": ((3,), np.float64)}


@NS
@pytest.mark.parametrize("what, table, sizes, subset", [
    ("first_hits", HIT, (16, 48), {"normal": _abi.RPT_HIT_NORMAL, "object": _abi.RPT_HIT_OBJECT}),
    ("hit_surface", SURFACE, (16, 48), {"primitive": _abi.RPT_SURFACE_PRIMITIVE, "barycentric": _abi.RPT_SURFACE_BARYCENTRIC})])
def test_ray_records(what, table, sizes, subset, n):
    g = wrapper()
    o, d = rays(n)
    for names, kw, channels, flags in ((list(table), {}, 31, 0),
                                       (list(subset), dict(channels=sum(subset.values()), flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL),
                                        sum(subset.values()), _abi.RPT_FLAG_GENERAL_TRAVERSAL)):
        got = getattr(g, what)(o, d, **kw)
        cnt, po, pd, q, a = the_call(g, "rptgpu_" + what, 6)
        assert cnt == n and (address(po), address(pd)) == (o.ctypes.data, d.ctypes.data)
        assert fields(q) == dict(struct_size=sizes[0], channels=channels, precision_mode=STRICT, flags=flags)
        assert fields(a) == dict(struct_size=sizes[1], reserved=0)
        held(a, got, names)
        for name in names:
            assert is_array(got[name], (n,) + table[name][0], table[name][1]), name
    for bad in ((o.astype(np.float32), d), (o, d.ravel()), (o, np.zeros((n + 1, 3)))):
        with pytest.raises(ValueError):
            getattr(g, what)(*bad)
    assert not g.lib.calls


VERTEX = {"length": ("path", (), np.uint32), "t": ("vertex", (), np.float64), "normal": ("vertex", (3,), np.float64),
          "object": ("vertex", (), np.int32), "position": ("vertex", (3,), np.float64),
          "direction": ("vertex", (3,), np.float64), "draw": ("vertex", (), np.uint32), "radiance": ("vertex", (3,), np.float64),
          "bsdf": ("vertex", (3,), np.float64), "inv_pdf": ("vertex", (), np.float64), "abs_cos": ("vertex", (), np.float64),
          "rgb": ("ray", (3,), np.float64)}


@NS
def test_trace_vertices(n):
    g = wrapper()
    o, d = rays(n)
    ids = np.arange(n, dtype=np.uint32)
    sub = _abi.RPT_VERTEX_LENGTH | _abi.RPT_VERTEX_DRAW | _abi.RPT_VERTEX_RGB
    for names, kw, query in (
            (list(VERTEX), {}, dict(max_bounces=3, iterations=1, first_draw=0, exposure_value=0.0, seed=0x52505447,
                                    sample_index_base=0, flags=0, channels=4095)),
            (["length", "draw", "rgb"], dict(channels=sub, streams=ids, samples=2, seed=5, sample_index_base=9, first_draw=2,
                                             exposure_value=-1.0, flags=_abi.RPT_FLAG_WAVEFRONT),
             dict(max_bounces=3, iterations=2, first_draw=2, exposure_value=-1.0, seed=5, sample_index_base=9,
                  flags=_abi.RPT_FLAG_WAVEFRONT, channels=sub))):
        got = g.trace_vertices(o, d, 3, **kw)
        cnt, po, pd, pids, q, a = the_call(g, "rptgpu_trace_vertices", 7)
        assert cnt == n and (address(po), address(pd)) == (o.ctypes.data, d.ctypes.data)
        assert address(pids) == (ids.ctypes.data if "streams" in kw else None)
        assert fields(q) == dict(query, struct_size=56, precision_mode=STRICT, reserved=0)
        assert fields(a) == dict(struct_size=104, reserved=0)
        assert got.channels == query["channels"] and sorted(got.arrays()) == sorted(names)
        held(a, got.arrays(), names)
        heads = {"path": (n, query["iterations"]), "vertex": (n, query["iterations"], 4), "ray": (n,)}
        for name, (kind, tail, dtype) in VERTEX.items():
            v = getattr(got, name)
            assert is_array(v, heads[kind] + tail, dtype) if name in names else v is None, name
    # the call's contract: (n, 3) float64 rays only, but ids of any dtype and shape that flatten to n
    g.trace_vertices(o, d, 1, streams=np.arange(n, dtype=np.float64).reshape(n, 1))
    pids = the_call(g, "rptgpu_trace_vertices", 7)[3]
    assert (np.ctypeslib.as_array(pids, (max(n, 1),))[:n] == ids).all()
    for bad in (dict(origins=o.astype(np.float32)), dict(dirs=d.ravel()), dict(streams=np.zeros(n + 1))):
        kw = dict(origins=o, dirs=d, max_bounces=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            g.trace_vertices(**kw)
    assert not g.lib.calls


# ---- the view calls
def views(n):
    cams = [Camera((1.0 + i, 2.0, 3.0), (0.0, 0.0, -1.0)) for i in range(n)]
    vs = [cams[i] if i == 0 else View(cams[i], _abi.RPT_VIEW_ORTHOGRAPHIC, 2.5) if i == 1 else View(cams[i], _abi.RPT_VIEW_PANORAMA)
          for i in range(n)]
    return cams, vs


def lowered(arr, cams, n):
    """the RptView array the call passed: at least one element, view i the i-th camera under views()' projections"""
    assert isinstance(arr, C.Array) and arr._type_ is _abi.RptView and len(arr) == max(n, 1)
    for i in range(n):
        assert bytes(arr[i].camera) == bytes(cams[i].lower())
        assert (arr[i].projection, arr[i].ortho_scale) == ((0, 0.0), (1, 2.5), (2, 0.0))[i]


def seeds_passed(arr, seeds, n):
    assert isinstance(arr, C.Array) and arr._type_ is C.c_uint64 and len(arr) == max(n, 1) and list(arr[:n]) == seeds


W, H = 5, 4
VIEW_QUERY = dict(struct_size=64, width=W, height=H, _pad=0, precision_mode=STRICT)


@NS
@pytest.mark.parametrize("seeded", [False, True])
def test_render_views(seeded, n):
    g = wrapper()
    cams, vs = views(n)
    seeds = [(1 << 63) + i for i in range(n)] if seeded else None
    name, argc = ("rptgpu_render_views_seeded", 6) if seeded else ("rptgpu_render_views", 5)
    got = g.render_views(vs, W, H, 3, seeds=seeds)
    args = the_call(g, name, argc)
    assert args[0] == n
    lowered(args[1], cams, n)
    assert fields(args[2]) == dict(VIEW_QUERY, max_bounces=3, iterations=1, exposure_value=0.0, seed=0x52505447, seed_stride=0,
                                   sample_index_base=0, flags=0)
    if seeded:
        seeds_passed(args[3], seeds, n)
    assert is_array(got, (n, H, W, 3), np.float64) and address(args[-1]) == got.ctypes.data
    out = np.empty((n, H, W, 3))
    stride = 0 if seeded else 11
    assert g.render_views(vs, W, H, 2, samples=4, seed=6, seed_stride=stride, sample_index_base=8, exposure_value=0.5,
                          flags=_abi.RPT_FLAG_WAVEFRONT, out=out, seeds=np.array(seeds, dtype=np.uint64) if seeded else None) is out
    args = the_call(g, name, argc)
    assert fields(args[2]) == dict(VIEW_QUERY, max_bounces=2, iterations=4, exposure_value=0.5, seed=6, seed_stride=stride,
                                   sample_index_base=8, flags=_abi.RPT_FLAG_WAVEFRONT)
    assert address(args[-1]) == out.ctypes.data
    for bad in (np.empty((n, H, W, 3), dtype=np.float32), np.empty((n, W, H, 3)), np.empty((n + 1, H, W, 3))):
        with pytest.raises(ValueError, match="out must be"):
            g.render_views(vs, W, H, 1, out=bad, seeds=seeds)
    assert not g.lib.calls


AOV = {"hits": ((), np.uint32), "depth": ((), np.float64), "normal": ((3,), np.float64), "albedo": ((3,), np.float64),
       "position": ((3,), np.float64), "object": ((), np.int32)}


@NS
@pytest.mark.parametrize("seeded", [False, True])
def test_render_views_aov(seeded, n):
    g = wrapper()
    cams, vs = views(n)
    seeds = [7 + i for i in range(n)] if seeded else None
    name, argc = ("rptgpu_render_views_aov_seeded", 6) if seeded else ("rptgpu_render_views_aov", 5)
    sub = _abi.RPT_AOV_DEPTH | _abi.RPT_AOV_OBJECT
    for names, kw, channels in ((list(AOV), {}, 31), (["hits", "depth", "object"], dict(channels=sub), sub)):
        got = g.render_views_aov(vs, W, H, seeds=seeds, **kw)
        args = the_call(g, name, argc)
        assert args[0] == n
        lowered(args[1], cams, n)
        assert fields(args[2]) == dict(VIEW_QUERY, max_bounces=0, iterations=1, exposure_value=0.0, seed=0x52505447,
                                       seed_stride=0, sample_index_base=0, flags=0)
        if seeded:
            seeds_passed(args[3], seeds, n)
        assert fields(args[-1]) == dict(struct_size=56, channels=channels)
        held(args[-1], got, names)
        for k in names:
            assert is_array(got[k], (n, H, W) + AOV[k][0], AOV[k][1]) and not got[k].any(), k  # zero-initialised
    out = {k: np.ones((n, H, W) + AOV[k][0], dtype=AOV[k][1]) for k in ("hits", "normal")}
    stride = 0 if seeded else 3
    got = g.render_views_aov(vs, W, H, samples=2, seed=4, seed_stride=stride, sample_index_base=5, channels=_abi.RPT_AOV_NORMAL,
                             flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL, out=out, seeds=seeds)
    args = the_call(g, name, argc)
    assert fields(args[2]) == dict(VIEW_QUERY, max_bounces=0, iterations=2, exposure_value=0.0, seed=4, seed_stride=stride,
                                   sample_index_base=5, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert sorted(got) == ["hits", "normal"] and all(got[k] is out[k] for k in out)
    held(args[-1], out, ["hits", "normal"])
    assert all(v.all() for v in out.values()) or n == 0  # the caller's arrays are not written here
    with pytest.raises(ValueError, match="exactly the keys"):
        g.render_views_aov(vs, W, H, out=out, seeds=seeds)
    with pytest.raises(ValueError, match="C-contiguous"):
        g.render_views_aov(vs, W, H, channels=_abi.RPT_AOV_NORMAL, out=dict(out, hits=out["hits"].astype(np.int32)), seeds=seeds)
    assert not g.lib.calls


DENOISED = {"denoised": ((3,), np.float64), "rgb8": ((3,), np.uint8), "mean": ((3,), np.float64), "variance": ((), np.float64)}


@NS
@pytest.mark.parametrize("seeded", [False, True])
def test_render_views_denoised(seeded, n):
    g = wrapper()
    cams, vs = views(n)
    seeds = [7 + i for i in range(n)] if seeded else None
    filt = dict(struct_size=40, levels=3, sigma_color=2.0, sigma_normal=0.1, sigma_depth=0.01, sigma_albedo=0.1)
    for want, kw in ((("denoised",), {}), (tuple(DENOISED), dict(want=tuple(DENOISED))), (("rgb8", "variance"), dict(want=["rgb8", "variance"]))):
        got = g.render_views_denoised(vs, W, H, 3, 2, 4, seeds=seeds, **kw)
        cnt, arr, q, pseeds, d, o = the_call(g, "rptgpu_render_views_denoised", 7)
        assert cnt == n
        lowered(arr, cams, n)
        assert fields(q) == dict(VIEW_QUERY, max_bounces=3, iterations=2, exposure_value=0.0, seed=0x52505447, seed_stride=0,
                                 sample_index_base=0, flags=0)
        if seeded:
            seeds_passed(pseeds, seeds, n)
        else:
            assert pseeds is None
        assert fields(d) == dict(struct_size=64, batches=4, feature_iterations=4, _pad=0, feature_sample_index_base=0, filter=filt)
        assert fields(o) == dict(struct_size=40, _pad=0)
        held(o, got, want)
        for k in want:
            assert is_array(got[k], (n, H, W) + DENOISED[k][0], DENOISED[k][1]), k
    out = {k: np.empty((n, H, W) + DENOISED[k][0], dtype=DENOISED[k][1]) for k in ("rgb8", "mean")}
    stride = 0 if seeded else 3
    got = g.render_views_denoised(vs, W, H, 1, 5, 6, seed=4, seed_stride=stride, seeds=seeds, sample_index_base=7, feature_samples=8,
                                  feature_sample_index_base=9, levels=2, sigma_color=1.0, sigma_normal=0.5, sigma_depth=0.25,
                                  sigma_albedo=0.125, exposure_value=2.0, flags=_abi.RPT_FLAG_WAVEFRONT, want=("rgb8", "mean"), out=out)
    cnt, arr, q, pseeds, d, o = the_call(g, "rptgpu_render_views_denoised", 7)
    assert fields(q) == dict(VIEW_QUERY, max_bounces=1, iterations=5, exposure_value=2.0, seed=4, seed_stride=stride,
                             sample_index_base=7, flags=_abi.RPT_FLAG_WAVEFRONT)
    assert fields(d) == dict(struct_size=64, batches=6, feature_iterations=8, _pad=0, feature_sample_index_base=9,
                             filter=dict(struct_size=40, levels=2, sigma_color=1.0, sigma_normal=0.5, sigma_depth=0.25, sigma_albedo=0.125))
    assert sorted(got) == ["mean", "rgb8"] and all(got[k] is out[k] for k in out)
    held(o, out, ["rgb8", "mean"])
    with pytest.raises(ValueError, match="exactly the keys"):
        g.render_views_denoised(vs, W, H, 1, 1, 1, out=out, seeds=seeds)
    with pytest.raises(ValueError, match="C-contiguous"):
        g.render_views_denoised(vs, W, H, 1, 1, 1, want=("rgb8", "mean"), out=dict(out, mean=np.zeros((n, H, W, 3), dtype=np.float32)), seeds=seeds)
    assert not g.lib.calls


@pytest.mark.parametrize("channels, names", [(_abi.RPT_AOV_ALL, list(AOV)), (_abi.RPT_AOV_ALBEDO | _abi.RPT_AOV_OBJECT, ["hits", "albedo", "object"]),
                                             (0, ["hits"])])
def test_render_aov(channels, names):
    g = wrapper()
    cam, p = Camera((1.0, 2.0, 3.0)), make_params(W, H, 2, 3)
    got = g.render_aov(cam, p, channels)
    pcam, pp, b = the_call(g, "rptgpu_render_aov", 4)
    assert bytes(pcam._obj) == bytes(cam.lower()) and pp._obj is p
    assert fields(b) == dict(struct_size=56, channels=channels)
    held(b, got, names)
    for k in names:
        assert is_array(got[k], (H, W) + AOV[k][0], AOV[k][1]) and not got[k].any(), k  # zero-initialised
    low = cam.lower()
    g.render_aov(low, p)  # a lowered camera goes as it is
    assert the_call(g, "rptgpu_render_aov", 4)[0]._obj is low


# ---- the live updates
@NS
def test_set_mesh(n):
    g = wrapper()
    tris = np.random.RandomState(1).uniform(-1.0, 1.0, (n, 18))
    assert g.set_mesh(2, tris) is None
    index, cnt, p = the_call(g, "rptgpu_scene_set_mesh", 4)
    assert (index, cnt) == (2, n) and isinstance(p, C.POINTER(_abi.RptTriangle)) and address(p) == tris.ctypes.data
    g.set_mesh(0, np.concatenate([tris, tris], axis=1)[:, :18])  # a view: a contiguous copy goes
    index, cnt, p = the_call(g, "rptgpu_scene_set_mesh", 4)
    assert (index, cnt) == (0, n) and (np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), (max(n, 1), 18))[:n] == tris).all()
    for bad, error in ((tris.astype(np.float32), TypeError), (tris.ravel(), ValueError), (np.zeros((n, 9)), ValueError)):
        with pytest.raises(error):
            g.set_mesh(2, bad)
    with pytest.raises(ValueError, match="negative"):
        g.set_mesh(-1, tris)
    assert not g.lib.calls


def test_set_group():
    g = wrapper()
    later = [k.translate((0.0, 0.0, 0.5)) for k in _children()]
    rec = transform_records(later)
    for children in (rec, later):
        assert g.set_group(1, children) is None
        index, cnt, arr = the_call(g, "rptgpu_scene_set_group", 4)
        assert (index, cnt) == (1, 4) and isinstance(arr, C.Array) and arr._type_ is _abi.RptShape and len(arr) == 4
        for i in range(4):
            assert (arr[i].kind, arr[i].transformed) == ((2, 1) if i % 2 else (0, 1))
            assert bytes(arr[i].xf) == rec[i].tobytes()
    g.set_group(3, [])  # no children: a sequence goes as it is
    index, cnt, arr = the_call(g, "rptgpu_scene_set_group", 4)
    assert (index, cnt) == (3, 0)
    for bad, error in ((rec.astype(np.float32), TypeError), (rec[:, :50], ValueError), (rec[:3], ValueError), (rec[:0], ValueError)):
        with pytest.raises(error):
            g.set_group(1, bad)
    with pytest.raises(ValueError, match="negative"):
        g.set_group(-1, rec)
    assert not g.lib.calls


# ---- tensors that are not on the handle's device: refused before the library and before any torch.cuda call
@pytest.fixture
def no_device(monkeypatch):
    torch = pytest.importorskip("torch")

    def fail(*args, **kw):
        raise AssertionError("torch.cuda.current_stream was asked for before the refusal")
    monkeypatch.setattr(torch.cuda, "current_stream", fail)
    return torch


def refused(g, error, call):
    with pytest.raises(error):
        call()
    assert not g.lib.calls


def test_ray_and_point_calls_refuse_host_tensors(no_device):
    torch = no_device
    g = wrapper()
    a = np.zeros((3, 3))
    t = torch.zeros((3, 3), dtype=torch.float64)
    ids, mt = torch.arange(3, dtype=torch.int32), torch.ones(3, dtype=torch.float64)
    for x, y in ((t, t), (t, a), (a, t)):
        refused(g, ValueError, lambda: g.trace_rays(x, y, 2))
        refused(g, ValueError, lambda: g.trace_rays(x, y, 2, streams=ids, out=torch.zeros((3, 3), dtype=torch.float64)))
        refused(g, ValueError, lambda: g.bake_probes(x, y, kind=_abi.RPT_PROBE_IRRADIANCE, samples=1, max_bounces=1, seed=1))
        refused(g, ValueError, lambda: g.occluded(x, y))
        refused(g, ValueError, lambda: g.occluded(x, y, max_t=mt))
        refused(g, ValueError, lambda: g.bake_ao(x, y, samples=1, seed=1))
        refused(g, ValueError, lambda: g.bake_ao(x, y, samples=1, seed=1, streams=ids, bent_normals=True))
        refused(g, ValueError, lambda: g.first_hits(x, y))
        refused(g, ValueError, lambda: g.hit_surface(x, y))
        refused(g, ValueError, lambda: g.trace_vertices(x, y, 2))
        refused(g, ValueError, lambda: g.trace_vertices(x, y, 2, streams=ids))
    refused(g, ValueError, lambda: g.bake_probes(t, kind=_abi.RPT_PROBE_SH9, samples=1, max_bounces=1, seed=1))
    refused(g, ValueError, lambda: g.bake_probes(t, kind=_abi.RPT_PROBE_SH9, samples=1, max_bounces=1, seed=1, streams=ids))


def test_view_calls_refuse_host_tensors(no_device):
    torch = no_device
    g = wrapper()
    cams, vs = views(2)
    n = 2
    refused(g, ValueError, lambda: g.render_views(vs, W, H, 1, out=torch.zeros((n, H, W, 3), dtype=torch.float64)))
    refused(g, ValueError, lambda: g.render_views(vs, W, H, 1, out=torch.zeros((n, H, W, 3), dtype=torch.float32), seeds=[1, 2]))
    hits, depth = torch.zeros((n, H, W), dtype=torch.int32), torch.zeros((n, H, W), dtype=torch.float64)
    for out in (dict(hits=hits, depth=depth), dict(hits=np.zeros((n, H, W), dtype=np.uint32), depth=depth),
                dict(hits=hits, depth=np.zeros((n, H, W)))):
        refused(g, ValueError, lambda: g.render_views_aov(vs, W, H, channels=_abi.RPT_AOV_DEPTH, out=out))
        refused(g, ValueError, lambda: g.render_views_aov(vs, W, H, channels=_abi.RPT_AOV_DEPTH, out=out, seeds=[1, 2]))
    den, rgb = torch.zeros((n, H, W, 3), dtype=torch.float64), torch.zeros((n, H, W, 3), dtype=torch.uint8)
    for out in (dict(denoised=den, rgb8=rgb), dict(denoised=np.zeros((n, H, W, 3)), rgb8=rgb),
                dict(denoised=den, rgb8=np.zeros((n, H, W, 3), dtype=np.uint8))):
        refused(g, ValueError, lambda: g.render_views_denoised(vs, W, H, 1, 1, 1, want=("denoised", "rgb8"), out=out))
        refused(g, ValueError, lambda: g.render_views_denoised(vs, W, H, 1, 1, 1, want=("denoised", "rgb8"), out=out, seeds=[1, 2]))
    refused(g, ValueError, lambda: g.render_views_aov(vs, W, H, out="numpy"))
    refused(g, ValueError, lambda: g.render_views_denoised(vs, W, H, 1, 1, 1, out="numpy"))


def test_live_updates_refuse_host_tensors(no_device):
    torch = no_device
    g = wrapper()
    refused(g, ValueError, lambda: g.set_mesh(2, torch.zeros((4, 18), dtype=torch.float64)))
    refused(g, TypeError, lambda: g.set_mesh(2, torch.zeros((4, 18), dtype=torch.float32)))
    refused(g, ValueError, lambda: g.set_mesh(2, torch.zeros((4, 9), dtype=torch.float64)))
    refused(g, ValueError, lambda: g.set_group(1, torch.zeros((4, 51), dtype=torch.float64)))
    refused(g, TypeError, lambda: g.set_group(1, torch.zeros((4, 51), dtype=torch.float32)))
    refused(g, ValueError, lambda: g.set_group(1, torch.zeros((4, 18), dtype=torch.float64)))
