// Stand-alone check of rpt_amd/csrc/shape_records.h — the one copy of the expressions that scene creation
// (host_scene.cpp) and the live group update's kernels (group_update.hip) share — against the expressions as
// host_scene.cpp held them before the header existed, restated here.  Built by tests/test_group_update_host.py with the
// compiler and flags of host_scene.o (what std::fmax returns, and how the sums are associated, is the compiler's).
// Everything is compared bit for bit, with the exception tests/cpp/mesh_records_check.cpp documents: a NaN that ARITHMETIC
// produces from two NaN operands takes the sign and payload of whichever operand the compiler put first, so a coordinate
// of xf_point passes when both copies hold a NaN.  The boxes are selections (a NaN coordinate never enters one: min2 /
// max2 keep the accumulated side), the local boxes are constants and quadric_too_small is a flag: bit for bit.
// Prints one line per group and exits non-zero when a group differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../rpt_amd/csrc/shape_records.h"

namespace was { // host_scene.cpp before shape_records.h

struct Box { double lo[3], hi[3]; };

// column-major 4x4 * (v,1), accumulated column by column (nalgebra gemv order)
__attribute__((noinline)) void xf_point(const double* m, const double* v, double* r) {
  for (int k = 0; k < 3; k++) r[k] = ((m[k] * v[0] + m[4 + k] * v[1]) + m[8 + k] * v[2]) + m[12 + k] * 1.0;
}
Box merge(const Box& a, const Box& b) { // BoundingBox::merge kdtree.rs:46-51 (mesh_records.h, as the flattener had it)
  Box r;
  rptrec::merge_box(a.lo, a.hi, b.lo, b.hi, r.lo, r.hi);
  return r;
}
Box empty_box() { // BoundingBox::default kdtree.rs:35-42
  Box b;
  for (int k = 0; k < 3; k++) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; }
  return b;
}
__attribute__((noinline)) Box transformed_box(const Box& b, const double* m) { // shape.rs:153-176
  Box r = empty_box();
  for (int ix = 0; ix < 2; ix++)
    for (int iy = 0; iy < 2; iy++)
      for (int iz = 0; iz < 2; iz++) {
        double v[3] = {ix ? b.hi[0] : b.lo[0], iy ? b.hi[1] : b.lo[1], iz ? b.hi[2] : b.lo[2]};
        double c[3];
        xf_point(m, v, c);
        Box p;
        for (int k = 0; k < 3; k++) p.lo[k] = p.hi[k] = c[k];
        r = merge(r, p);
      }
  return r;
}
// fill_inst's local boxes: sphere.rs:66-73, cube.rs:10-17
__attribute__((noinline)) bool local_box(int32_t kind, Box& local) {
  switch (kind) {
    case RPT_SHAPE_SPHERE:
      for (int k = 0; k < 3; k++) { local.lo[k] = -1.0; local.hi[k] = 1.0; }
      return true;
    case RPT_SHAPE_CUBE:
      for (int k = 0; k < 3; k++) { local.lo[k] = -0.5; local.hi[k] = 0.5; }
      return true;
    default: return false;
  }
}
__attribute__((noinline)) bool quadric_too_small(const rptdev::Inst& in, const double* qscale) {
  if (in.kind == RPT_SHAPE_MONOMIAL) return true;
  if (in.kind != RPT_SHAPE_SPHERE) return false;
  double r_min = 1.0; // smallest singular value of the placement >= 1 / ||M^-1||_F
  if (in.has_xf) {
    double b = 0.0;
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) b += in.inv[4 * c + r] * in.inv[4 * c + r];
    r_min = 1.0 / std::sqrt(b);
  }
  const double step = std::fmax(std::fmax(qscale[0], qscale[1]), qscale[2]);
  return !(r_min >= 64.0 * step);
}

} // namespace was

namespace {

bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

uint64_t failures = 0;

// one matrix through both copies: a point, the placed sphere's and cube's boxes, a placed box of its own, and the
// quadric rule with the matrix as the record's inverse on the grid steps `qscale`
void check_matrix(const double* m, const double* v, const was::Box& own, const double* qscale) {
  double pa[3], pb[3];
  was::xf_point(m, v, pa);
  rptrec::xf_point(m, v, pb);
  for (int k = 0; k < 3; k++)
    if (!same(pa + k, pb + k, 8) && !(pa[k] != pa[k] && pb[k] != pb[k])) failures++;
  for (int32_t kind : {RPT_SHAPE_SPHERE, RPT_SHAPE_CUBE, RPT_SHAPE_PLANE, RPT_SHAPE_MESH, RPT_SHAPE_GROUP, RPT_SHAPE_MONOMIAL}) {
    was::Box la = own;
    rptrec::Box6 lb;
    std::memcpy(&lb, &own, sizeof lb);
    const bool ka = was::local_box(kind, la), kb = rptrec::local_box(kind, lb.lo, lb.hi);
    if (ka != kb || !same(&la, &lb, sizeof la)) failures++;
    const was::Box ba = was::transformed_box(la, m);
    rptrec::Box6 bb;
    rptrec::transformed_box(lb.lo, lb.hi, m, bb.lo, bb.hi);
    if (!same(&ba, &bb, sizeof ba)) failures++;
    for (int has_xf = 0; has_xf < 2; has_xf++) {
      rptdev::Inst in;
      std::memset(&in, 0, sizeof in);
      in.kind = kind; in.has_xf = has_xf;
      std::memcpy(in.inv, m, sizeof in.inv);
      if (was::quadric_too_small(in, qscale) != rptrec::quadric_too_small(in, qscale)) failures++;
    }
  }
}

bool group(const char* name) {
  std::printf("%-44s %s\n", name, failures ? "DIFFERS" : "equal");
  const bool ok = failures == 0;
  failures = 0;
  return ok;
}

} // namespace

int main() {
  const double inf = INFINITY, nan = NAN;
  const std::vector<double> special = {0.0, -0.0, nan, -nan, inf, -inf, 1.0, -1.0, 5e-324, -5e-324, 1.5, 1e308, -1e308, 2.5e-7};
  const double identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const was::Box unit = {{-1.0, -0.5, 0.0}, {1.0, 0.5, -0.0}};
  bool ok = true;

  // the identity, its signed-zero variants, translations, zero scales on every subset of axes, the zero matrix: on grid
  // steps around the quadric rule's threshold (1 / 64) and on special ones
  {
    std::mt19937_64 rng(20261019);
    std::uniform_real_distribution<double> u(-3.0, 3.0);
    for (int i = 0; i < 100000; i++) {
      double m[16];
      std::memcpy(m, identity, sizeof m);
      const int flat = i & 7; // axes whose scale is zero
      for (int k = 0; k < 3; k++) {
        if (flat & (1 << k)) m[5 * k] = (i & 8) ? -0.0 : 0.0;
        else if (i & 16) m[5 * k] = u(rng);
        if (i & 32) m[12 + k] = u(rng);
      }
      if (i & 64) for (int k = 0; k < 16; k++) if (m[k] == 0.0 && (rng() & 1)) m[k] = -0.0;
      if ((i & 0x780) == 0x780) std::memset(m, 0, sizeof m);
      const double v[3] = {u(rng), u(rng), u(rng)};
      double qscale[3];
      for (int k = 0; k < 3; k++) qscale[k] = (i & 128) ? special[rng() % special.size()] : (1.0 / 64.0) * (1.0 + 1e-15 * (double)((int)(rng() % 5) - 2));
      check_matrix(m, v, unit, qscale);
    }
  }
  ok = group("identity and singular matrices") && ok;

  // matrices, points, boxes and grid steps drawn from the special values (NaN, infinities, both zeros, extremes)
  {
    std::mt19937_64 rng(5);
    for (int i = 0; i < 300000; i++) {
      double m[16], v[3], qscale[3];
      was::Box own;
      for (int k = 0; k < 16; k++) m[k] = (i % 3 == 0 || (rng() & 3) == 0) ? special[rng() % special.size()] : identity[k];
      for (int k = 0; k < 3; k++) {
        v[k] = special[rng() % special.size()];
        own.lo[k] = special[rng() % special.size()];
        own.hi[k] = special[rng() % special.size()];
        qscale[k] = special[rng() % special.size()];
      }
      check_matrix(m, v, own, qscale);
    }
  }
  ok = group("non-finite and special matrices") && ok;

  // 10^6 random placements: a scale times a rotation-like mix plus a translation, at sizes from 1e-6 to 1e6, on grid steps
  // near 1 / (64 ||M^-1||) so that the quadric rule falls on both sides
  {
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(-1.0, 1.0), e(-6.0, 6.0);
    for (int i = 0; i < 1000000; i++) {
      double m[16], v[3], qscale[3];
      const double size = std::pow(10.0, e(rng));
      for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) m[4 * c + r] = r == 3 ? (c == 3 ? 1.0 : 0.0) : (c == 3 ? 10.0 * u(rng) : size * u(rng));
      was::Box own;
      double b = 0.0;
      for (int k = 0; k < 3; k++) {
        v[k] = u(rng);
        const double x = u(rng), y = u(rng);
        own.lo[k] = x < y ? x : y; own.hi[k] = x < y ? y : x;
      }
      for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) b += m[4 * c + r] * m[4 * c + r];
      const double edge = 1.0 / std::sqrt(b) / 64.0;
      for (int k = 0; k < 3; k++) qscale[k] = edge * (1.0 + ((i & 1) ? 1e-15 : 0.3) * u(rng));
      check_matrix(m, v, own, qscale);
    }
  }
  ok = group("1 000 000 random matrices") && ok;
  return ok ? 0 : 1;
}
