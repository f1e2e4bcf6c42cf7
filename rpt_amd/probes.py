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


class ProbeVolume:
    """A regular grid of SH9 probes, for GpuScene.sample_probe_volume, lookup_probe_volume and render_views_probe_lit
    (include/rpt_gpu_probe_volume.h).  counts = (nx, ny, nz); probe (i, j, k) stands at origin + (i, j, k) *
    spacing and has index (k * ny + j) * nx + i; coeffs is (nz, ny, nx, 9, 3) float64 — or (n, 9, 3) in index order, what
    bake_probes(kind=RPT_PROBE_SH9) returns for positions() —; valid (nz, ny, nx) or (n,) uint8 or bool, non-zero where the
    probe holds a value, or None: every probe does.  numpy arrays or torch tensors on the handle's device, both of one
    kind; the calls check them."""

    def __init__(self, origin, spacing, counts, coeffs, valid=None):
        self.origin = tuple(float(x) for x in origin)
        self.spacing = tuple(float(x) for x in spacing)
        self.counts = tuple(int(x) for x in counts)
        if len(self.origin) != 3 or len(self.spacing) != 3 or len(self.counts) != 3:
            raise ValueError("ProbeVolume: origin, spacing and counts have three entries each")
        self.coeffs, self.valid = coeffs, valid

    @staticmethod
    def positions(origin, spacing, counts):
        """The probes' positions -> (nx * ny * nz, 3) float64 in index order: x runs fastest, then y, then z; each
        coordinate is origin + index * spacing, one multiply and one add."""
        nx, ny, nz = (int(c) for c in counts)
        o, h = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        idx = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], axis=1).astype(np.float64)
        return o + idx * h

    @classmethod
    def bake(cls, gpu_scene, origin, spacing, counts, *, samples, max_bounces, seed, flags=0, device=False):
        """bake_probes(kind=RPT_PROBE_SH9) over positions(origin, spacing, counts), wrapped: probe p's stream id is p.
        device=True: the positions go to the handle's device as a torch tensor and the coefficients stay there."""
        from ._abi import RPT_PROBE_SH9
        pos = cls.positions(origin, spacing, counts)
        if device:
            import torch
            pos = torch.from_numpy(pos).to(torch.device("cuda", int(gpu_scene.device)))
        coeffs = gpu_scene.bake_probes(pos, kind=RPT_PROBE_SH9, samples=samples, max_bounces=max_bounces, seed=seed, flags=flags)
        return cls(origin, spacing, counts, coeffs)
