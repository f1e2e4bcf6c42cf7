// shape_records.h — the records a placed sphere or cube gives rise to as a child of a KdTree<Box<dyn Bounded>>, ONE copy
// of each expression: compiled by the host flattener (host_scene.cpp, scene creation) and by the kernels of the live group
// update (group_update.hip), so that an updated handle cannot drift from a fresh one.  mesh_records.h's sibling, under the
// same rule: every translation unit that includes this is built with -ffp-contract=off and IEEE division / square root.
// tests/cpp/group_records_check.cpp holds these against the expressions as host_scene.cpp held them before.
#pragma once
#include "../../include/rpt_gpu.h"
#include "mesh_records.h"

namespace rptrec {

// column-major 4x4 * (v,1), accumulated column by column (nalgebra gemv order)
RPT_REC_FN void xf_point(const double* m, const double* v, double* r) {
  for (int k = 0; k < 3; k++) r[k] = ((m[k] * v[0] + m[4 + k] * v[1]) + m[8 + k] * v[2]) + m[12 + k] * 1.0;
}

// Bounded::bounding_box of the kinds whose box does not depend on a parameter: Sphere sphere.rs:66-73, Cube cube.rs:10-17;
// false for every other kind (lo / hi untouched)
RPT_REC_FN bool local_box(int32_t kind, double* lo, double* hi) {
  if (kind != RPT_SHAPE_SPHERE && kind != RPT_SHAPE_CUBE) return false;
  const double h = kind == RPT_SHAPE_SPHERE ? 1.0 : 0.5;
  for (int k = 0; k < 3; k++) { lo[k] = -h; hi[k] = h; }
  return true;
}

// Transformed::bounding_box shape.rs:153-176: the eight corners through m, merged in this order into the empty box
// (BoundingBox::default kdtree.rs:35-42)
RPT_REC_FN void transformed_box(const double* blo, const double* bhi, const double* m, double* rlo, double* rhi) {
  for (int k = 0; k < 3; k++) { rlo[k] = INFINITY; rhi[k] = -INFINITY; }
  for (int ix = 0; ix < 2; ix++)
    for (int iy = 0; iy < 2; iy++)
      for (int iz = 0; iz < 2; iz++) {
        double v[3] = {ix ? bhi[0] : blo[0], iy ? bhi[1] : blo[1], iz ? bhi[2] : blo[2]};
        double c[3];
        xf_point(m, v, c);
        for (int k = 0; k < 3; k++) {
          rlo[k] = min2(rlo[k], c[k]);
          rhi[k] = max2(rhi[k], c[k]);
        }
      }
}

// Spheres (and monomial surfaces) are tested by solving a polynomial whose coefficients grow with the square of the
// origin's distance in OBJECT units: from far away Sphere::intersect accepts lines that miss the sphere (kernels/
// shapes.inc boxray_make).  The device bounds the origin's distance to 1e7 grid steps when quadrics are filtered; a
// sphere whose smallest semi-axis is below 64 steps (1e-3 of the grid) is not filtered at all, nor is a monomial surface.
RPT_REC_FN bool quadric_too_small(const rptdev::Inst& in, const double* qscale) {
  if (in.kind == RPT_SHAPE_MONOMIAL) return true;
  if (in.kind != RPT_SHAPE_SPHERE) return false;
  double r_min = 1.0; // smallest singular value of the placement >= 1 / ||M^-1||_F
  if (in.has_xf) {
    double b = 0.0;
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) b += in.inv[4 * c + r] * in.inv[4 * c + r];
    r_min = 1.0 / sqrt(b);
  }
  const double step = max2(max2(qscale[0], qscale[1]), qscale[2]);
  return !(r_min >= 64.0 * step);
}

} // namespace rptrec
