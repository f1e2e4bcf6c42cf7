"""rptgpu_hit_surface without a GPU: the two symbols, detected the way a binding detects them, and both structs' layouts against
the header; every refusal that comes before the device — through the host and the device entry point, with its code, its
detail and the arrays untouched —; no CPU fallback; what GpuScene.hit_surface lowers its arguments to; rpt_amd.surface.interpolate
against a closed form; the sizing header (rpt_amd/csrc/surface_plan.h) in a stand-alone program (tests/cpp/surface_plan_check.cpp),
plain and under AddressSanitizer + UBSan.

And the YARDSTICK of tests/test_gpu_hit_surface.py, checked by itself: surface_model.tri_records — Triangle::intersect restated in
numpy — must give the oracle's t and shading normal, bit for bit, for SOME triangle of the mesh a ray of the untransformed mesh
scenes hits (cornell's walls, wine_glass's glass and table: the neighbours' box rays); and through the host mirror's matrices
(rpt_amd/glm.py) in nalgebra's operation order for a transformed mesh (coverage) and for meshes inside a group (fractal_teapots,
nested_groups) too, which is what lets the GPU test hold those to the bit as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi, surface

import routes_cases
import small_scenes
import surface_model as M
import test_gpu_occlusion as occ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
NAMES = ("rptgpu_hit_surface", "rptgpu_hit_surface_device")
QUERY_FIELDS = ("struct_size", "channels", "precision_mode", "flags")
ARRAY_FIELDS = ("struct_size", "reserved", "t", "object", "child", "primitive", "barycentric")
BITS = (("t", _abi.RPT_SURFACE_T), ("object", _abi.RPT_SURFACE_OBJECT), ("child", _abi.RPT_SURFACE_CHILD),
        ("primitive", _abi.RPT_SURFACE_PRIMITIVE), ("barycentric", _abi.RPT_SURFACE_BARYCENTRIC))


def test_symbols_and_struct_layouts_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert all(hasattr(lib, n) for n in NAMES) and _abi.hit_surface_supported(lib)
    assert tuple(s[0] for s in _abi.HIT_SURFACE_SYMBOLS) == NAMES and not set(NAMES) & {s[0] for s in _abi.SYMBOLS}
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7

    class Older:  # a library without the two: still ABI 7, and the detection says so
        rptgpu_first_hits = None
    assert not _abi.hit_surface_supported(Older())
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptSurfaceQuery));' + \
          "".join('printf(" %%zu", offsetof(RptSurfaceQuery, %s));' % f for f in QUERY_FIELDS) + \
          'printf(" %zu", sizeof(RptSurfaceArrays));' + \
          "".join('printf(" %%zu", offsetof(RptSurfaceArrays, %s));' % f for f in ARRAY_FIELDS) + \
          'printf(" %u %u %u %u %u", RPT_SURFACE_T, RPT_SURFACE_OBJECT, RPT_SURFACE_CHILD, RPT_SURFACE_PRIMITIVE, RPT_SURFACE_BARYCENTRIC);' + \
          'printf("\\n");return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    q, a, bits = nums[:5], nums[5:13], nums[13:]
    assert C.sizeof(_abi.RptSurfaceQuery) == q[0] == 16
    assert [getattr(_abi.RptSurfaceQuery, f).offset for f in QUERY_FIELDS] == q[1:] == [0, 4, 8, 12]
    assert [f for f, _ in _abi.RptSurfaceQuery._fields_] == list(QUERY_FIELDS)
    assert C.sizeof(_abi.RptSurfaceArrays) == a[0] == 48
    assert [getattr(_abi.RptSurfaceArrays, f).offset for f in ARRAY_FIELDS] == a[1:] == [0, 4, 8, 16, 24, 32, 40]
    assert [f for f, _ in _abi.RptSurfaceArrays._fields_] == list(ARRAY_FIELDS)
    assert bits == [b for _, b in BITS] == [1, 2, 4, 8, 16] and _abi.RPT_SURFACE_ALL == 31
    assert rpt_amd.RPT_SURFACE_PRIMITIVE == 8 and rpt_amd.surface is surface


def query(**kw):
    q = _abi.RptSurfaceQuery()
    q.struct_size, q.channels = C.sizeof(_abi.RptSurfaceQuery), _abi.RPT_SURFACE_ALL
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; hit surfaces run the closest-hit query "
              "and a resolve walk only").encode()
MODE = b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"
Q_SIZE = b"RptSurfaceQuery: struct_size is not sizeof(RptSurfaceQuery)"
A_SIZE = b"RptSurfaceArrays: struct_size is not sizeof(RptSurfaceArrays)"
# (what is passed: q, the arrays struct's fields, which arrays are NULL, n) -> the detail
REFUSALS = [
    ("no query", dict(q=None), b"null RptSurfaceQuery"),
    ("no arrays struct", dict(arrays=None), b"null RptSurfaceArrays"),
    ("query size 0", dict(q=query(struct_size=0)), Q_SIZE),
    ("query size 12", dict(q=query(struct_size=12)), Q_SIZE),
    ("query size 24", dict(q=query(struct_size=24)), Q_SIZE),
    ("arrays size 0", dict(a_size=0), A_SIZE),
    ("arrays size 40", dict(a_size=40), A_SIZE),
    ("arrays size 56", dict(a_size=56), A_SIZE),
    ("no channel", dict(q=query(channels=0)), b"RptSurfaceQuery: channels == 0 (name at least one RPT_SURFACE_* channel)"),
    ("unknown bit", dict(q=query(channels=32 | _abi.RPT_SURFACE_T)), b"RptSurfaceQuery: channels names an unknown RPT_SURFACE_* bit"),
    ("high bit", dict(q=query(channels=1 << 31)), b"RptSurfaceQuery: channels names an unknown RPT_SURFACE_* bit"),
    ("reserved", dict(reserved=1), b"RptSurfaceArrays: reserved != 0"),
    ("t", dict(t=False), b"RptSurfaceArrays: RPT_SURFACE_T is named but t is NULL"),
    ("object", dict(object=False), b"RptSurfaceArrays: RPT_SURFACE_OBJECT is named but object is NULL"),
    ("child", dict(child=False), b"RptSurfaceArrays: RPT_SURFACE_CHILD is named but child is NULL"),
    ("primitive", dict(primitive=False), b"RptSurfaceArrays: RPT_SURFACE_PRIMITIVE is named but primitive is NULL"),
    ("barycentric", dict(barycentric=False), b"RptSurfaceArrays: RPT_SURFACE_BARYCENTRIC is named but barycentric is NULL"),
    ("mode", dict(q=query(precision_mode=1)), MODE),
    ("persistent", dict(q=query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("origins", dict(origins=False), b"null argument"),
    ("dirs", dict(dirs=False), b"null argument"),
    ("handle", dict(), b"null handle"),
    ("handle, one channel and only its array", dict(q=query(channels=_abi.RPT_SURFACE_PRIMITIVE), t=False, object=False, child=False,
                                                     barycentric=False), b"null handle"),
    ("handle, no rays", dict(n=0, origins=False, dirs=False), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_hit_surface_refuses_before_the_device(row, device):
    """... so every refusal is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    o, d = np.full(12, 7.0), np.full(12, 7.0)
    outs = {"t": np.full(4, 7.0), "object": np.full(4, 7, dtype=np.int32), "child": np.full(4, 7, dtype=np.int32),
            "primitive": np.full(4, 7, dtype=np.int32), "barycentric": np.full(12, 7.0)}
    q = kw.get("q", query())
    a = _abi.RptSurfaceArrays()
    a.struct_size, a.reserved = kw.get("a_size", C.sizeof(_abi.RptSurfaceArrays)), kw.get("reserved", 0)
    types = dict(_abi.RptSurfaceArrays._fields_)
    for name, arr in outs.items():  # (device: pointers that are never followed — every row is refused before the device)
        if kw.get(name, True):
            setattr(a, name, arr.ctypes.data_as(types[name]))
    ap = C.byref(a) if kw.get("arrays", True) is not None else None
    qp = C.byref(q) if q is not None else None
    use = lambda name, arr: arr if kw.get(name, True) else None
    # a call with another detail first: the text checked afterwards is the call's own
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    if device:
        p = lambda arr: C.c_void_p(arr.ctypes.data) if arr is not None else None
        rc = lib.rptgpu_hit_surface_device(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), qp, ap, None)
    else:
        p = lambda arr: arr.ctypes.data_as(PD) if arr is not None else None
        rc = lib.rptgpu_hit_surface(None, kw.get("n", 4), p(use("origins", o)), p(use("dirs", d)), qp, ap)
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (o == 7).all() and (d == 7).all() and all((arr == 7).all() for arr in outs.values())


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never an answer from the host."""
    scene = rpt_amd.scenes.sphere_scene()[0]
    o = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    d = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1))
    if gpu_available:
        got = rpt_amd.GpuScene(scene).hit_surface(o, d)
        assert (got["object"] >= 0).all() and (got["primitive"] == -1).all() and (got["child"] == -1).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).hit_surface(o, d)
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


def test_what_the_python_call_lowers_to():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)
    g.lib, g.handle, g.device = Recorder(), C.c_void_p(0x1234), 0
    o = np.arange(12.0).reshape(4, 3)
    d = o[::-1] * 0.5            # not contiguous: the call sees a contiguous copy
    out = g.hit_surface(o, d, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
    name, (h, n, po, pd, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert name == "rptgpu_hit_surface" and h is g.handle and n == 4
    assert (q.struct_size, q.channels, q.precision_mode, q.flags) == (16, 31, _abi.RPT_PRECISION_F64_STRICT, _abi.RPT_FLAG_GENERAL_TRAVERSAL)
    assert (a.struct_size, a.reserved) == (48, 0)
    floats = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
    address = lambda p: C.cast(p, C.c_void_p).value
    assert (floats(po, 12) == o.ravel()).all() and (floats(pd, 12) == d.ravel()).all()
    assert sorted(out) == ["barycentric", "child", "object", "primitive", "t"]
    assert out["t"].shape == (4,) and out["t"].dtype == np.float64 and out["barycentric"].shape == (4, 3)
    for k in ("object", "child", "primitive"):
        assert out[k].shape == (4,) and out[k].dtype == np.int32
    for k, v in out.items():
        assert address(getattr(a, k)) == v.ctypes.data
    # two channels: the other pointers stay NULL
    out = g.hit_surface(o, d, channels=_abi.RPT_SURFACE_PRIMITIVE | _abi.RPT_SURFACE_BARYCENTRIC)
    name, (h, n, po, pd, q, a) = g.lib.calls.pop()
    q, a = q._obj, a._obj
    assert sorted(out) == ["barycentric", "primitive"] and (q.channels, q.flags) == (24, 0)
    assert not a.t and not a.object and not a.child and address(a.primitive) == out["primitive"].ctypes.data
    assert not g.lib.calls
    g.handle = None


def test_the_python_call_checks_its_shapes_and_dtypes():
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    z = np.zeros((3, 3))
    with pytest.raises(ValueError, match=r"hit_surface: origins must be an \(n, 3\) float64 array"):
        g.hit_surface(np.zeros((3, 2)), z)
    with pytest.raises(ValueError, match=r"hit_surface: dirs must be an \(n, 3\) float64 array"):
        g.hit_surface(z, z.astype(np.float32))
    with pytest.raises(ValueError, match="hit_surface: 3 origins for 2 directions"):
        g.hit_surface(z, np.zeros((2, 3)))
    for call, word in ((lambda: g.hit_surface(z, z), "null handle"),  # well-formed arrays: the library speaks
                       (lambda: g.hit_surface(z, z, channels=0), "channels == 0"),
                       (lambda: g.hit_surface(z, z, channels=64), "unknown RPT_SURFACE_")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            call()
        assert e.value.code == E and word in str(e.value)
    g.handle = None


def test_interpolate_against_a_closed_form():
    """an attribute that is AFFINE in position, a(p) = A p + b, given at the vertices, interpolates to a(hit point): the
    weights sum to 1 and u v1 + v v2 + w v3 is the point"""
    rs = np.random.RandomState(4)
    n_tris, n = 9, 50
    verts = rs.uniform(-2.0, 2.0, (n_tris, 3, 3))
    A, b = rs.uniform(-1.0, 1.0, (4, 3)), rs.uniform(-1.0, 1.0, 4)
    values = verts @ A.T + b                               # (n_tris, 3, 4)
    prim = rs.randint(-1, n_tris, n).astype(np.int32)
    bary = rs.dirichlet((1.0, 1.0, 1.0), n)
    bary[prim < 0] = 0.0
    got = surface.interpolate(values, prim, bary)
    assert got.shape == (n, 4) and got.dtype == np.float64
    hit = prim >= 0
    assert hit.any() and (~hit).any() and (got[~hit] == 0.0).all()
    point = np.einsum("ik,ikc->ic", bary[hit], verts[prim[hit]])
    assert np.abs(got[hit] - (point @ A.T + b)).max() <= 1e-14 * 16
    # the stated order of operations, to the bit; one corner's weight picks that corner's value
    a = values[prim[hit]]
    u, v, w = (bary[hit][:, k, None] for k in range(3))
    assert M.same(got[hit], u * a[:, 0] + v * a[:, 1] + w * a[:, 2])
    corner = surface.interpolate(values, np.array([3, 3, 3]), np.eye(3))
    assert (corner == values[3]).all()
    # scalars per vertex: (n_tris, 3) in, (n,) out
    s = surface.interpolate(values[:, :, 0], prim, bary)
    assert s.shape == (n,) and M.same(s, got[:, 0])
    assert surface.interpolate(values, np.zeros(0, dtype=np.int32), np.zeros((0, 3))).shape == (0, 4)
    for bad, word in (((values[:, :2], prim, bary), "values must be"), ((values, prim.astype(np.float64), bary), "integer"),
                      ((values, prim, bary[:-1]), "one row per primitive"), ((values, np.array([n_tris]), bary[:1]), "of a mesh of 9")):
        with pytest.raises(ValueError, match=word):
            surface.interpolate(*bad)


# ---- the yardstick against the oracle
def rays_for(name, kind):
    if kind == "box":
        return M.box_rays(name) if name in occ.BOXES else routes_cases.rays(name)
    box = occ.BOXES[name] if name in occ.BOXES else routes_cases.BOXES[name]
    return M.aimed_rays(small_scenes.small(name)[0], box, sum(map(ord, name)) + 7)


def reproduced(name, kind):
    """-> (rays on an object that holds a mesh at the top or one level down, those for which SOME triangle of such a mesh
    gives the oracle's t — bits — with weights >= 0, those for which it gives the oracle's normal too, whether any of them
    reached its mesh through a Transformed)"""
    from oracle import oracle_ffi
    scene = small_scenes.small(name)[0]
    o, d = rays_for(name, kind)
    t, nrm, obj = oracle_ffi.OracleScene(scene).closest_hit(o, d)
    by_object = {}
    for ob, ch, chain, mesh in M.meshes_of(scene):
        by_object.setdefault(ob, []).append((chain, mesh))
    on, with_t, with_n, placed = 0, 0, 0, False
    for i in np.flatnonzero(obj >= 0):
        if obj[i] not in by_object:
            continue
        on += 1
        found_t = found_n = False
        for chain, mesh in by_object[obj[i]]:
            lo, ld = o[i:i + 1], d[i:i + 1]
            for xf in chain:
                if xf is not None:
                    lo, ld = M.local_rays(xf, lo, ld)
            k = len(mesh.triangles)
            time, uvw, n = M.tri_records(mesh.triangles, np.repeat(lo, k, 0), np.repeat(ld, k, 0))
            for xf in reversed(chain):
                if xf is not None:
                    n = M.world_normals(xf, n)
            m = (M.bits(time) == M.bits(t[i:i + 1])) & (uvw >= 0.0).all(axis=1)
            if m.any():
                found_t = True
                if (M.bits(n[m]) == M.bits(nrm[i])).all(axis=1).any():
                    found_n = True
                    placed = placed or any(xf is not None for xf in chain)
        with_t += found_t
        with_n += found_n
    return on, with_t, with_n, placed


@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_the_restatement_gives_the_oracles_record_on_untransformed_meshes(name):
    """every hit on these scenes' meshes is a triangle's: all of them are reproduced, t and normal, bit for bit"""
    on, with_t, with_n, placed = reproduced(name, "box")
    assert on >= 60 and with_t == on and with_n == on and not placed


@pytest.mark.parametrize("name", ["coverage", "fractal_teapots", "nested_groups"])
def test_the_mirrors_matrices_restate_transformed_meshes_to_the_bit(name):
    """the local ray and the normal transform from rpt_amd/glm.py's matrices in nalgebra's order: where a ray's record is a
    triangle's (a group also holds spheres, cubes and monomial surfaces: their hits match no triangle's t), the restatement
    gives t AND the normal to the bit — no tolerance is needed for placed meshes"""
    on, with_t, with_n, placed = reproduced(name, "aimed")
    assert with_t >= 60 and with_n == with_t and placed
    if name == "fractal_teapots":
        assert with_t == on  # (its groups hold meshes only)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("surface_plan_" + request.param) / "surface_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "surface_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover"])
def test_surface_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
