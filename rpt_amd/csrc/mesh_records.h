// mesh_records.h — the records a mesh's triangles give rise to, ONE copy of each expression: compiled by the host
// flattener (host_scene.cpp, scene creation) and by the kernels of the live mesh update (mesh_update.hip), so that an
// updated handle cannot drift from a fresh one.  Every translation unit that includes this is built with
// -ffp-contract=off and IEEE division / square root: the values are the reference's doubles (mesh.rs:40-73,
// kdtree.rs:46-51).
#pragma once
#include <math.h>
#include <stdint.h>

#include "device_types.h"

#if defined(__HIPCC__)
#define RPT_REC_FN __host__ __device__ inline
#else
#define RPT_REC_FN inline
#endif

namespace rptrec {

// fmin / fmax as the host flattener has always evaluated them (what its compiler makes of std::fmin(x, y) on x86-64:
// the other operand when x is a NaN, else `y < x ? y : x`), written as comparisons so that the device agrees: of two
// equal zeros of opposite sign the FIRST argument is returned, a NaN in y never wins.  The kd builders are sensitive
// to the sign of a zero; tests/cpp/mesh_records_check.cpp holds these against std::fmin / std::fmax for
// every combination of +-0, NaN, infinities and ordinary values.
RPT_REC_FN double min2(double x, double y) { return x != x ? y : (y < x ? y : x); }
RPT_REC_FN double max2(double x, double y) { return x != x ? y : (y > x ? y : x); }

// a box as six doubles: lo xyz, hi xyz (rpthost::Box has the same layout)
struct Box6 {
  double lo[3], hi[3];
};

// Triangle::bounding_box: glm::min3 / max3 over the vertices, mesh.rs:40-45.  v: v1 v2 v3 (9 doubles, then the normals)
RPT_REC_FN void tri_box(const double* v, double* lo, double* hi) {
  for (int k = 0; k < 3; k++) {
    lo[k] = min2(min2(v[k], v[3 + k]), v[6 + k]);
    hi[k] = max2(max2(v[k], v[3 + k]), v[6 + k]);
  }
}

// BoundingBox::merge kdtree.rs:46-51: r = merge(a, b), the accumulated box first
RPT_REC_FN void merge_box(const double* alo, const double* ahi, const double* blo, const double* bhi, double* rlo, double* rhi) {
  for (int k = 0; k < 3; k++) {
    rlo[k] = min2(alo[k], blo[k]);
    rhi[k] = max2(ahi[k], bhi[k]);
  }
}

// mesh.rs:50-51 and :64-69, same expression order as the reference (nalgebra dot = (a+b)+c, normalize = component /
// norm).  v: the triangle's v1 v2 v3
RPT_REC_FN void fill_trix(const double* v, rptdev::TriX& x) {
  const double* v1 = v;
  const double* v2 = v + 3;
  const double* v3 = v + 6;
  double d0[3], d1[3], c[3];
  for (int k = 0; k < 3; k++) { d0[k] = v2[k] - v1[k]; d1[k] = v3[k] - v1[k]; }
  c[0] = d0[1] * d1[2] - d0[2] * d1[1];
  c[1] = d0[2] * d1[0] - d0[0] * d1[2];
  c[2] = d0[0] * d1[1] - d0[1] * d1[0];
  double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  for (int k = 0; k < 3; k++) { x.pn[k] = c[k] / len; x.v1[k] = v1[k]; x.d0[k] = d0[k]; x.d1[k] = d1[k]; }
  x.d00 = (d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2];
  x.d01 = (d0[0] * d1[0] + d0[1] * d1[1]) + d0[2] * d1[2];
  x.d11 = (d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2];
  x.denom = x.d00 * x.d11 - x.d01 * x.d01;
}

RPT_REC_FN bool finite1(double v) { return fabs(v) <= 1.7976931348623157e308; } // (false for NaN and the infinities)

// ill-conditioned barycentric system, degenerate or NaN: never filtered
RPT_REC_FN bool sliver(const rptdev::TriX& x) { return !(x.denom > 1e-10 * (x.d00 * x.d11)) || !finite1(x.denom); }

// Conservative 16-bit boxes of a mesh's leaf entries (device_types.h LeafBox).  Grid: 65529 steps across the
// tree's bounds per axis plus two steps of padding on either side; a minimum is rounded down and a maximum up, then
// both move one more step outwards, so the decoded box contains the triangle's true box with a margin of at least
// (1 - 1e-12) steps on every side —
// orders of magnitude more than the rounding of the decode and of the slab arithmetic on the device.  A triangle
// whose barycentric system is ill-conditioned (sliver: rounding in mesh.rs:64-73 could accept a point that is not
// near the triangle) or that has a non-finite vertex gets the whole grid, i.e. it is never filtered.  GROUP trees get
// the boxes of their children the same way (a child's hit point lies on the child, hence in its bounding box).
RPT_REC_FN rptdev::LeafBox quantise_box(const double* blo, const double* bhi, const double* qlo, const double* qscale, bool full) {
  uint32_t q[6];
  for (int k = 0; k < 3 && !full; k++) {
    double a = floor((blo[k] - qlo[k]) / qscale[k]) - 1.0;
    double c = ceil((bhi[k] - qlo[k]) / qscale[k]) + 1.0;
    if (!(a == a) || !(c == c)) { full = true; break; }
    q[k] = (uint32_t)min2(max2(a, 0.0), 65535.0);
    q[3 + k] = (uint32_t)min2(max2(c, 0.0), 65535.0);
  }
  if (full) { q[0] = q[1] = q[2] = 0; q[3] = q[4] = q[5] = 65535; }
  // stored per axis as centre and half-extent (device_types.h): c = floor of the middle, h = hi - c >= c - lo, so
  // [c - h, c + h] contains [lo, hi] and is at most one step wider on the low side (c - h may be -1: the decode is
  // arithmetic, nothing clamps it)
  rptdev::LeafBox lb;
  for (int k = 0; k < 3; k++) {
    const uint32_t c = (q[k] + q[3 + k]) >> 1, h = q[3 + k] - c;
    lb.w[k] = c | (h << 16);
  }
  lb.w[3] = full ? 1u : 0u;
  return lb;
}

// the grid is two steps larger than the bounds on every side: a coordinate of a primitive maps to [2, 65531], so the
// outward rounding above (floor - 1, ceil + 1) never reaches the clamp, i.e. a box on a face of the tree's bounds
// keeps its margin too (tests/test_leaf_boxes.py found the case: a vertex on the bounds, a hit exactly there)
RPT_REC_FN void grid_over(const double* bounds, double* qlo, double* qscale) {
  for (int k = 0; k < 3; k++) {
    double ext = bounds[3 + k] - bounds[k];
    qscale[k] = (ext > 0.0 && finite1(ext)) ? ext / 65529.0 : 1.0;
    qlo[k] = bounds[k] - 2.0 * qscale[k];
  }
}

} // namespace rptrec
