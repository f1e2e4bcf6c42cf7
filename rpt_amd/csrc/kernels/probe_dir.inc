// kernels/probe_dir.inc — what the two routes of rptgpu_bake_probes share: a light probe's direction from its stream and the SH9
// basis.  Included by wavefront.inc (rpt_raygen_probes, rpt_resolve_probes) and by paths_rays.inc (rpt_paths_rays,
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

// The real spherical harmonics of bands 0-2 at the unit vector d, in the order (0,0), (1,-1), (1,0), (1,1), (2,-2) .. (2,2)
// and with the expressions include/rpt_gpu.h fixes (rpt_amd.sh9_basis restates them).
RPT_DEV void sh9_basis(D3 d, double (&Y)[9]) {
  const double x = d.x, y = d.y, z = d.z;
  Y[0] = 0.28209479177387814;
  Y[1] = 0.4886025119029199 * y;
  Y[2] = 0.4886025119029199 * z;
  Y[3] = 0.4886025119029199 * x;
  Y[4] = 1.0925484305920792 * (x * y);
  Y[5] = 1.0925484305920792 * (y * z);
  Y[6] = 0.31539156525252005 * (3.0 * (z * z) - 1.0);
  Y[7] = 1.0925484305920792 * (x * z);
  Y[8] = 0.5462742152960396 * (x * x - y * y);
}
