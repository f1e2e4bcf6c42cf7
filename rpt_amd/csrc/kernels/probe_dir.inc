// kernels/probe_dir.inc — what the two routes of rptgpu_bake_probes share: a light probe's direction from its stream and the SH9
// basis (kernels/sh9_basis.inc).  Included by wavefront.inc (rpt_raygen_probes, rpt_resolve_probes) and by paths_rays.inc (rpt_paths_rays,
// rpt_project_probes): ONE text, so the two routes cannot drift apart.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// A light probe's direction (rptgpu_bake_probes, include/rpt_gpu.h), drawn from the stream's draw 0 on.  SH9: uniform on the
// sphere without transcendentals — a point of the unit disc lifted to the sphere; IRRADIANCE: cosine-weighted about
// normalize(normal), Sphere::sample (sphere.rs:52-64) as it stands.  rng.draw is then where the probe's path continues.
RPT_DEV D3 probe_direction(uint32_t kind, D3 normal, Rng& rng) {
  if (kind == RPT_PROBE_IRRADIANCE) return sample_sphere(normal, rng).v;
  double x1, x2;
  unit_disc(rng, x1, x2);
  const double s = x1 * x1 + x2 * x2;
  const double r = 2.0 * sqrt(1.0 - s);
  return mk(x1 * r, x2 * r, 1.0 - 2.0 * s);
}

// sh9_basis, in a file of its own: the probe volume's kernels (kernels/probe_volume.inc) take it without this file's sampler
#include "sh9_basis.inc"
