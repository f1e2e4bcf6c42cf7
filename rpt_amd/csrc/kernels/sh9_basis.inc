// kernels/sh9_basis.inc — the SH9 basis: ONE text for the bake (kernels/probe_dir.inc includes it, for rpt_resolve_probes and
// rpt_project_probes) and for the readers of a bake (kernels/probe_volume.inc).  Needs D3 (kernels/vec.inc) and RPT_DEV.

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
