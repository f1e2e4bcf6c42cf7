"""rptgpu_bake_probes without a GPU: the two symbols and RptProbeQuery's layout against the header, every refusal that
comes before the device with its code and detail, no CPU fallback, the Python wrapper's own checks, and the numpy helpers
rpt_amd.sh9_basis / sh9_irradiance against exact quadrature and closed forms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT
PD = C.POINTER(C.c_double)
FIELDS = ("struct_size", "kind", "samples", "max_bounces", "seed", "sample_index_base", "precision_mode", "flags")


def test_symbols_and_struct_size_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert hasattr(lib, "rptgpu_bake_probes") and hasattr(lib, "rptgpu_bake_probes_device")
    names = {s[0] for s in _abi.SYMBOLS}
    assert {"rptgpu_bake_probes", "rptgpu_bake_probes_device"} <= names
    assert lib.rptgpu_abi_version() == 7  # additions within ABI 7
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptProbeQuery));' + \
          "".join('printf(" %%zu", offsetof(RptProbeQuery, %s));' % f for f in FIELDS) + \
          'printf(" %d %d\\n", RPT_PROBE_SH9, RPT_PROBE_IRRADIANCE);return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(_abi.RptProbeQuery) == nums[0] == 40
    assert [getattr(_abi.RptProbeQuery, f).offset for f in FIELDS] == nums[1:-2]
    assert [f for f, _ in _abi.RptProbeQuery._fields_] == list(FIELDS)
    assert [_abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE] == nums[-2:] == [0, 1]
    assert (rpt_amd.RPT_PROBE_SH9, rpt_amd.RPT_PROBE_IRRADIANCE) == (0, 1)


def _query(**kw):
    q = _abi.RptProbeQuery()
    q.struct_size, q.kind, q.samples, q.max_bounces = C.sizeof(_abi.RptProbeQuery), _abi.RPT_PROBE_SH9, 4, 2
    for k, v in kw.items():
        setattr(q, k, v)
    return q


PERSISTENT = ("RptProbeQuery: RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; light probes run the "
              "wavefront pipeline only").encode()
IRR = _abi.RPT_PROBE_IRRADIANCE
REFUSALS = [
    ("no query", dict(q=None), b"null RptProbeQuery"),
    ("size 0", dict(q=_query(struct_size=0)), b"RptProbeQuery: struct_size is not sizeof(RptProbeQuery)"),
    ("size 32", dict(q=_query(struct_size=32)), b"RptProbeQuery: struct_size is not sizeof(RptProbeQuery)"),
    ("size 48", dict(q=_query(struct_size=48)), b"RptProbeQuery: struct_size is not sizeof(RptProbeQuery)"),
    ("kind 2", dict(q=_query(kind=2)), b"RptProbeQuery: unknown kind (RPT_PROBE_SH9 = 0, RPT_PROBE_IRRADIANCE = 1)"),
    ("kind 2^32 - 1", dict(q=_query(kind=0xffffffff)), b"RptProbeQuery: unknown kind (RPT_PROBE_SH9 = 0, RPT_PROBE_IRRADIANCE = 1)"),
    ("samples", dict(q=_query(samples=0)), b"RptProbeQuery: samples == 0"),
    ("bounces", dict(q=_query(max_bounces=255)), b"RptProbeQuery: max_bounces > 254"),
    ("mode", dict(q=_query(precision_mode=1)),
     b"unknown precision_mode (RPT_PRECISION_F64_STRICT = 0 is the only mode; F64_FAST was removed in ABI v4)"),
    ("persistent", dict(q=_query(flags=_abi.RPT_FLAG_PERSISTENT)), PERSISTENT),
    ("persistent | wavefront", dict(q=_query(flags=_abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_WAVEFRONT)), PERSISTENT),
    ("positions", dict(positions=False), b"null argument"),
    ("out", dict(out=False), b"null argument"),
    ("irradiance, positions", dict(q=_query(kind=IRR), positions=False), b"null argument"),
    ("irradiance, no normals", dict(q=_query(kind=IRR), normals=False),
     b"null normals: RPT_PROBE_IRRADIANCE gathers about each probe's normal"),
    ("2^32 + 1 probes without ids", dict(n=(1 << 32) + 1, streams=False),
     b"more than 2^32 probes without stream ids (a stream id has 32 bits)"),
    ("handle", dict(), b"null handle"),
    ("handle, sh9 without normals", dict(normals=False), b"null handle"),
    ("handle, irradiance", dict(q=_query(kind=IRR)), b"null handle"),
    ("handle, no ids", dict(streams=False), b"null handle"),
    ("handle, no probes", dict(n=0, positions=False, normals=False, out=False, streams=False), b"null handle"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_every_refusal_comes_before_the_device(row, device):
    """... so each of them is there without a handle: code, detail, and nothing written"""
    _, kw, detail = REFUSALS[row]
    lib = _abi.load_library()
    pos, nrm, out = np.full(12, 7.0), np.full(12, 7.0), np.full(4 * 27, 7.0)
    ids = np.full(4, 7, dtype=np.uint32)
    q = kw.get("q", _query())
    use = lambda name, a: a if kw.get(name, True) else None
    # a call with another detail first: the text below is this call's
    assert lib.rptgpu_render_batch(None, None, None, None) == E and lib.rptgpu_last_error_detail(None) == b"null out_rgb"
    if device:  # (pointers that are never followed: every row is refused before the device is looked at)
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib.rptgpu_bake_probes_device(None, kw.get("n", 4), p(use("positions", pos)), p(use("normals", nrm)),
                                           p(use("streams", ids)), C.byref(q) if q is not None else None, p(use("out", out)), None)
    else:
        p = lambda a: a.ctypes.data_as(PD) if a is not None else None
        s = use("streams", ids)
        rc = lib.rptgpu_bake_probes(None, kw.get("n", 4), p(use("positions", pos)), p(use("normals", nrm)),
                                    s.ctypes.data_as(C.POINTER(C.c_uint32)) if s is not None else None,
                                    C.byref(q) if q is not None else None, p(use("out", out)))
    assert rc == E
    assert lib.rptgpu_last_error_detail(None) == detail
    assert (pos == 7).all() and (nrm == 7).all() and (out == 7).all() and (ids == 7).all()


@pytest.mark.parametrize("kind", [_abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE], ids=["sh9", "irradiance"])
def test_no_cpu_fallback(gpu_available, kind):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never probes from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    pos = np.tile(np.array([0.0, 0.0, 5.0]), (4, 1))
    nrm = np.tile(np.array([0.0, 0.0, -1.0]), (4, 1)) if kind == _abi.RPT_PROBE_IRRADIANCE else None
    kw = dict(kind=kind, samples=3, max_bounces=2, seed=1)
    if gpu_available:
        out = rpt_amd.GpuScene(scene).bake_probes(pos, nrm, **kw)
        assert out.shape == ((4, 9, 3) if nrm is None else (4, 3)) and np.isfinite(out).all()
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).bake_probes(pos, nrm, **kw)
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


def test_python_wrapper_checks_its_shapes_and_dtypes():
    """GpuScene.bake_probes refuses malformed arrays itself (the C call takes one n for all of them)"""
    g = rpt_amd.GpuScene.__new__(rpt_amd.GpuScene)  # no handle: none of these reaches the library
    g.lib, g.handle, g.device = _abi.load_library(), None, 0
    SH9, IRRAD = _abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE
    kw = dict(samples=4, max_bounces=1, seed=1)
    z = np.zeros((3, 3))
    with pytest.raises(ValueError, match=r"positions must be an \(n, 3\) float64 array"):
        g.bake_probes(np.zeros((3, 2)), kind=SH9, **kw)
    with pytest.raises(ValueError, match=r"positions must be an \(n, 3\) float64 array"):
        g.bake_probes(np.zeros(9), kind=SH9, **kw)
    with pytest.raises(ValueError, match=r"positions must be an \(n, 3\) float64 array"):
        g.bake_probes(z.astype(np.float32), kind=SH9, **kw)
    with pytest.raises(ValueError, match=r"normals must be an \(n, 3\) float64 array"):
        g.bake_probes(z, z.astype(np.float32), kind=IRRAD, **kw)
    with pytest.raises(ValueError, match="2 normals for 3 positions"):
        g.bake_probes(z, np.zeros((2, 3)), kind=IRRAD, **kw)
    with pytest.raises(ValueError, match="needs normals"):
        g.bake_probes(z, kind=IRRAD, **kw)
    with pytest.raises(ValueError, match="takes no normals"):
        g.bake_probes(z, z, kind=SH9, **kw)
    with pytest.raises(ValueError, match="kind must be"):
        g.bake_probes(z, kind=2, **kw)
    with pytest.raises(ValueError, match="5 stream ids for 3 probes"):
        g.bake_probes(z, kind=SH9, streams=np.arange(5), **kw)
    with pytest.raises(ValueError, match="streams must be"):
        g.bake_probes(z, kind=SH9, streams=np.arange(3.0), **kw)
    with pytest.raises(ValueError, match="out must be"):
        g.bake_probes(z, kind=SH9, out=np.zeros((3, 27)), **kw)
    with pytest.raises(ValueError, match="out must be"):
        g.bake_probes(z, z, kind=IRRAD, out=np.zeros((3, 3), dtype=np.float32), **kw)
    with pytest.raises(TypeError):
        g.bake_probes(z, None, SH9, 4, 1, 1)  # kind, samples, max_bounces, seed are keyword-only
    for nrm, kind in ((None, SH9), (z, IRRAD)):  # well-formed arrays: the library speaks (no handle)
        with pytest.raises(rpt_amd.RptGpuError) as e:
            g.bake_probes(z, nrm, kind=kind, **kw)
        assert e.value.code == E and "null handle" in str(e.value)
    g.handle = None


# ---- the numpy helpers
def sphere_rule(n_theta, n_phi):
    """Gauss-Legendre in z = cos(theta) x uniform in phi: exact for every polynomial in (x, y, z) of degree
    <= min(2 n_theta - 1, n_phi - 1) — the z part is a polynomial of that degree, and the uniform rule integrates
    cos(m phi), sin(m phi) exactly (to zero) for 0 < m < n_phi."""
    z, w = np.polynomial.legendre.leggauss(n_theta)
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    Z, P = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - Z * Z)
    dirs = np.stack([r * np.cos(P), r * np.sin(P), Z], axis=-1).reshape(-1, 3)
    weights = np.repeat(w, n_phi) * (2.0 * np.pi / n_phi)
    return dirs, weights


def test_sh9_basis_is_orthonormal():
    """products of two basis functions are polynomials of degree <= 4: 6 x 12 nodes are exact (degree 11)"""
    dirs, w = sphere_rule(6, 12)
    assert abs(w.sum() - 4.0 * np.pi) < 1e-13
    Y = rpt_amd.sh9_basis(dirs)
    assert Y.shape == (len(dirs), 9) and Y.dtype == np.float64
    gram = np.einsum("kj,kl,k->jl", Y, Y, w)
    assert np.abs(gram - np.eye(9)).max() <= 1e-13, np.abs(gram - np.eye(9)).max()
    assert rpt_amd.sh9_basis(np.zeros((2, 5, 3))).shape == (2, 5, 9)  # leading axes are kept
    with pytest.raises(ValueError):
        rpt_amd.sh9_basis(np.zeros((4, 2)))


def test_sh9_basis_has_the_headers_expressions():
    """operation for operation (bits), on directions with every sign pattern"""
    rs = np.random.RandomState(9)
    d = rs.standard_normal((64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = rpt_amd.sh9_basis(d)
    for i, (x, y, z) in enumerate(d.tolist()):
        want = [0.28209479177387814, 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
                1.0925484305920792 * (x * y), 1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0),
                1.0925484305920792 * (x * z), 0.5462742152960396 * (x * x - y * y)]
        assert Y[i].tolist() == want


def test_sh9_irradiance_of_constant_radiance():
    """L = c everywhere: only the (0,0) coefficient, c * sqrt(4 pi); E = pi c for every normal"""
    c = np.array([0.25, 1.0, 3.5])
    coeffs = np.zeros((9, 3))
    coeffs[0] = c * 3.5449077018110318
    rs = np.random.RandomState(3)
    n = rs.standard_normal((17, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    got = rpt_amd.sh9_irradiance(coeffs, n)  # coeffs broadcast over the normals
    assert got.shape == (17, 3)
    assert np.abs(got / (np.pi * c) - 1.0).max() <= 1e-14
    # projected by quadrature instead of written down: the same
    dirs, w = sphere_rule(6, 12)
    proj = np.einsum("kj,k,c->jc", rpt_amd.sh9_basis(dirs), w, c)
    assert np.abs(rpt_amd.sh9_irradiance(proj, n) / (np.pi * c) - 1.0).max() <= 1e-13
    with pytest.raises(ValueError):
        rpt_amd.sh9_irradiance(np.zeros((27,)), n[0])


def test_sh9_irradiance_of_a_clamped_cosine_lobe():
    """L(d) = max(0, d.a).  About its axis a the lobe is zonal: with N_l = sqrt((2l + 1) / (4 pi)) and t = d.a,
         L(d) = sum_l L_l N_l P_l(t),   L_l = 2 pi N_l * integral_0^1 t P_l(t) dt,
       and integral t P_0 = 1/2, t P_1 = 1/3, t P_2 = t (3 t^2 - 1) / 2 = 1/8 give
         L_0 = sqrt(pi) / 2,   L_1 = sqrt(pi / 3),   L_2 = sqrt(5 pi) / 8.
       The cosine convolution multiplies band l by A_l = pi, 2 pi / 3, pi / 4, and at n = a (t = 1, P_l = 1):
         E(a) = sum_l A_l L_l N_l = pi * (1/2)(1/2) + (2 pi / 3)(1/2) + (pi / 4)(5/16) = pi * (1/4 + 1/3 + 5/64).
       (The exact irradiance, the integral of max(0, d.a)^2, is 2 pi / 3 = pi * 0.6667; the truncation gives pi * 0.6615.)
       In the fixed basis the coefficients follow from the addition theorem, sum_m Y_lm(a) Y_lm(d) = N_l^2 P_l(a.d):
       c_j = (L_l / N_l) * Y_j(a).  They are written down, not integrated: the lobe's kink makes a product rule inexact."""
    want = np.pi * (1.0 / 4.0 + 1.0 / 3.0 + 5.0 / 64.0)
    N = np.sqrt((2.0 * np.array([0, 1, 1, 1, 2, 2, 2, 2, 2]) + 1.0) / (4.0 * np.pi))
    Ll = np.array([np.sqrt(np.pi) / 2.0] + [np.sqrt(np.pi / 3.0)] * 3 + [np.sqrt(5.0 * np.pi) / 8.0] * 5)
    rs = np.random.RandomState(5)
    axes = np.vstack([np.eye(3), -np.eye(3), rs.standard_normal((10, 3))])
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    for a in axes:
        cj = Ll / N * rpt_amd.sh9_basis(a)
        coeffs = np.repeat(cj[:, None], 3, axis=1) * np.array([1.0, 2.0, 0.5])
        got = rpt_amd.sh9_irradiance(coeffs, a)
        assert np.abs(got / (want * np.array([1.0, 2.0, 0.5])) - 1.0).max() <= 1e-13, (a, got)
    # and the coefficients themselves against a fine numerical projection about +z (no kink in phi there)
    z, w = np.polynomial.legendre.leggauss(64)
    t, wt = 0.5 * (z + 1.0), 0.5 * w  # [0, 1]: the lobe's support in cos(theta), where it is the polynomial t
    c0 = 2.0 * np.pi * np.sum(wt * t) * N[0]
    c2 = 2.0 * np.pi * np.sum(wt * t * 0.4886025119029199 * t)
    c6 = 2.0 * np.pi * np.sum(wt * t * 0.31539156525252005 * (3.0 * t * t - 1.0))
    assert np.allclose([c0, c2, c6], [Ll[0], Ll[1], Ll[4]], rtol=1e-13, atol=0)
