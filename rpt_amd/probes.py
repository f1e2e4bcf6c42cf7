"""Spherical harmonics of bands 0-2 on the host: the basis rptgpu_bake_probes projects radiance into (include/rpt_gpu.h
fixes the expressions; kernels/wavefront.inc sh9_basis evaluates the same ones) and the cosine convolution that turns a
probe's nine radiance coefficients into the irradiance of a surface.  Pure numpy: what a caller does with baked probes."""
import numpy as np


def sh9_basis(dirs):
    """The nine real spherical harmonics Y_0..Y_8 — (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2) .. (2,2) — at the unit
    vectors dirs (..., 3) -> (..., 9) float64, each with the header's expression, operation for operation."""
    d = np.asarray(dirs, dtype=np.float64)
    if d.shape[-1:] != (3,):
        raise ValueError("sh9_basis: dirs must be (..., 3)")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = np.empty(d.shape[:-1] + (9,), dtype=np.float64)
    out[..., 0] = 0.28209479177387814
    out[..., 1] = 0.4886025119029199 * y
    out[..., 2] = 0.4886025119029199 * z
    out[..., 3] = 0.4886025119029199 * x
    out[..., 4] = 1.0925484305920792 * (x * y)
    out[..., 5] = 1.0925484305920792 * (y * z)
    out[..., 6] = 0.31539156525252005 * (3.0 * (z * z) - 1.0)
    out[..., 7] = 1.0925484305920792 * (x * z)
    out[..., 8] = 0.5462742152960396 * (x * x - y * y)
    return out


# the clamped cosine lobe's zonal coefficients times sqrt(4 pi / (2 l + 1)), per band: pi, 2 pi / 3, pi / 4
_BAND = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def sh9_irradiance(coeffs, normals):
    """Irradiance E(n) = integral of L(d) max(0, d.n) of the radiance whose SH9 coefficients are coeffs (..., 9, 3) (what
    GpuScene.bake_probes(kind=RPT_PROBE_SH9) returns), at the unit normals (..., 3) -> (..., 3): the convolution with the
    clamped cosine, sum_j A_l(j) * coeffs[j] * Y_j(n) with A = pi, 2 pi / 3, pi / 4 for bands 0, 1, 2."""
    c = np.asarray(coeffs, dtype=np.float64)
    if c.shape[-2:] != (9, 3):
        raise ValueError("sh9_irradiance: coeffs must be (..., 9, 3)")
    y = sh9_basis(normals) * _BAND
    return np.einsum("...j,...jc->...c", y, c)
