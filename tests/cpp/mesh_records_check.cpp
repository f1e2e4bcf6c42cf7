// Stand-alone check of rpt_amd/csrc/mesh_records.h — the one copy of the expressions that scene creation
// (host_scene.cpp) and the live mesh update's kernels (mesh_update.hip) share — against the expressions as host_scene.cpp
// held them before the header existed, restated here from the reference lines they cite.  Built by
// tests/test_mesh_update_host.py with the compiler and flags of host_scene.o (what std::fmin / std::fmax return for
// equal zeros of opposite sign depends on the compiler and the library, and existing handles must not change a bit).
// Everything is compared bit for bit, with one exception that no source can close: a NaN that ARITHMETIC produces from two
// NaN operands (a vertex's NaN meeting the default NaN of inf - inf, say) takes the sign and payload of whichever operand
// the compiler put first, and a compiler is free to commute a product or a sum — two copies of the same text inlined
// into different callers already differ there.  So a word of TriX that arithmetic produced passes when both copies hold
// a NaN; nothing reads such a NaN but comparisons, which are false for every NaN.  Selections and copies (min / max, the
// boxes, TriX::v1, the leaf boxes, the grid, the sliver flag) keep NaN signs and are compared bit for bit like the rest.
// Prints one line per group and exits non-zero when a group differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../rpt_amd/csrc/mesh_records.h"

namespace was { // host_scene.cpp before mesh_records.h

struct Box { double lo[3], hi[3]; };

// BoundingBox::merge kdtree.rs:46-51
__attribute__((noinline)) Box merge(const Box& a, const Box& b) {
  Box r;
  for (int k = 0; k < 3; k++) {
    r.lo[k] = std::fmin(a.lo[k], b.lo[k]);
    r.hi[k] = std::fmax(a.hi[k], b.hi[k]);
  }
  return r;
}
// glm::min3 / max3, mesh.rs:40-45
__attribute__((noinline)) void tri_box(const double* v1, const double* v2, const double* v3, Box& b) {
  for (int k = 0; k < 3; k++) {
    b.lo[k] = std::fmin(std::fmin(v1[k], v2[k]), v3[k]);
    b.hi[k] = std::fmax(std::fmax(v1[k], v2[k]), v3[k]);
  }
}
__attribute__((noinline)) double fmin2(double x, double y) { return std::fmin(x, y); }
__attribute__((noinline)) double fmax2(double x, double y) { return std::fmax(x, y); }
// mesh.rs:50-51 and :64-69 (nalgebra dot = (a+b)+c, normalize = component / norm)
__attribute__((noinline)) void fill_trix(const double* v1, const double* v2, const double* v3, rptdev::TriX& x) {
  double d0[3], d1[3], c[3];
  for (int k = 0; k < 3; k++) { d0[k] = v2[k] - v1[k]; d1[k] = v3[k] - v1[k]; }
  c[0] = d0[1] * d1[2] - d0[2] * d1[1];
  c[1] = d0[2] * d1[0] - d0[0] * d1[2];
  c[2] = d0[0] * d1[1] - d0[1] * d1[0];
  double len = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  for (int k = 0; k < 3; k++) { x.pn[k] = c[k] / len; x.v1[k] = v1[k]; x.d0[k] = d0[k]; x.d1[k] = d1[k]; }
  x.d00 = (d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2];
  x.d01 = (d0[0] * d1[0] + d0[1] * d1[1]) + d0[2] * d1[2];
  x.d11 = (d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2];
  x.denom = x.d00 * x.d11 - x.d01 * x.d01;
}
__attribute__((noinline)) rptdev::LeafBox quantise_box(const Box& b, const double* qlo, const double* qscale, bool full) {
  uint32_t q[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 3 && !full; k++) {
    double a = std::floor((b.lo[k] - qlo[k]) / qscale[k]) - 1.0;
    double c = std::ceil((b.hi[k] - qlo[k]) / qscale[k]) + 1.0;
    if (!(a == a) || !(c == c)) { full = true; break; }
    q[k] = (uint32_t)std::fmin(std::fmax(a, 0.0), 65535.0);
    q[3 + k] = (uint32_t)std::fmin(std::fmax(c, 0.0), 65535.0);
  }
  if (full) { q[0] = q[1] = q[2] = 0; q[3] = q[4] = q[5] = 65535; }
  rptdev::LeafBox lb;
  for (int k = 0; k < 3; k++) {
    const uint32_t c = (q[k] + q[3 + k]) >> 1, h = q[3 + k] - c;
    lb.w[k] = c | (h << 16);
  }
  lb.w[3] = full ? 1u : 0u;
  return lb;
}
__attribute__((noinline)) void grid_over(const double* bounds, double* qlo, double* qscale) {
  for (int k = 0; k < 3; k++) {
    double ext = bounds[3 + k] - bounds[k];
    qscale[k] = (ext > 0.0 && std::isfinite(ext)) ? ext / 65529.0 : 1.0;
    qlo[k] = bounds[k] - 2.0 * qscale[k];
  }
}
__attribute__((noinline)) bool sliver(const rptdev::TriX& x) {
  return !(x.denom > 1e-10 * (x.d00 * x.d11)) || !std::isfinite(x.denom);
}

} // namespace was

namespace {

bool same(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }
// TriX: v1 (a copy) bit for bit; the words arithmetic produced bit for bit, or a NaN in both (see the top of the file)
bool same_trix(const rptdev::TriX& a, const rptdev::TriX& b) {
  if (!same(a.v1, b.v1, sizeof a.v1)) return false;
  const double* pa = (const double*)&a;
  const double* pb = (const double*)&b;
  for (size_t k = 0; k < sizeof(rptdev::TriX) / sizeof(double); k++)
    if (!same(pa + k, pb + k, 8) && !(pa[k] != pa[k] && pb[k] != pb[k])) return false;
  return true;
}

struct Tri { double v[18]; };

uint64_t failures = 0;

// one triangle through both copies: records, box, sliver flag; then its leaf box on `bounds`
void check_triangle(const Tri& t, const double* bounds) {
  rptdev::TriX xa, xb;
  std::memset(&xa, 0, sizeof xa); std::memset(&xb, 0, sizeof xb);
  was::fill_trix(t.v, t.v + 3, t.v + 6, xa);
  rptrec::fill_trix(t.v, xb);
  if (!same_trix(xa, xb)) failures++;
  was::Box ba;
  rptrec::Box6 bb;
  was::tri_box(t.v, t.v + 3, t.v + 6, ba);
  rptrec::tri_box(t.v, bb.lo, bb.hi);
  if (!same(&ba, &bb, sizeof ba)) failures++;
  if (was::sliver(xa) != rptrec::sliver(xb)) failures++;
  double qa[6], qb[6];
  was::grid_over(bounds, qa, qa + 3);
  rptrec::grid_over(bounds, qb, qb + 3);
  if (!same(qa, qb, sizeof qa)) failures++;
  for (int full = 0; full < 2; full++) {
    rptdev::LeafBox la = was::quantise_box(ba, qa, qa + 3, full != 0 || was::sliver(xa));
    rptdev::LeafBox lb = rptrec::quantise_box(bb.lo, bb.hi, qb, qb + 3, full != 0 || rptrec::sliver(xb));
    if (!same(&la, &lb, sizeof la)) failures++;
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
  bool ok = true;

  // min / max: every pair and triple, both argument orders, and the sequential fold the bounds use
  for (double x : special)
    for (double y : special) {
      const double a = was::fmin2(x, y), b = rptrec::min2(x, y), c = was::fmax2(x, y), d = rptrec::max2(x, y);
      if (!same(&a, &b, 8) || !same(&c, &d, 8)) failures++;
      for (double z : special) {
        Tri t{};
        for (int k = 0; k < 3; k++) { t.v[k] = x; t.v[3 + k] = y; t.v[6 + k] = z; }
        was::Box ba;
        rptrec::Box6 bb;
        was::tri_box(t.v, t.v + 3, t.v + 6, ba);
        rptrec::tri_box(t.v, bb.lo, bb.hi);
        if (!same(&ba, &bb, sizeof ba)) failures++;
        // KdTree::new's fold (kdtree.rs:110-113) over three boxes, from the empty box
        was::Box fa;
        rptrec::Box6 fb;
        for (int k = 0; k < 3; k++) { fa.lo[k] = fb.lo[k] = inf; fa.hi[k] = fb.hi[k] = -inf; }
        for (double w : {x, y, z}) {
          was::Box p;
          for (int k = 0; k < 3; k++) p.lo[k] = p.hi[k] = w;
          fa = was::merge(fa, p);
          rptrec::Box6 r;
          rptrec::merge_box(fb.lo, fb.hi, p.lo, p.hi, r.lo, r.hi);
          fb = r;
        }
        if (!same(&fa, &fb, sizeof fa)) failures++;
      }
    }
  ok = group("min / max / fold over +-0, NaN, inf") && ok;

  // triangles whose coordinates are drawn from the special values (degenerate, non-finite, zero-extent axes), on
  // bounds drawn the same way (a vertex on the bounds, a zero-extent axis, NaN and infinite bounds)
  {
    std::mt19937_64 rng(20261019);
    const double unit[6] = {0.0, -0.0, -1.0, 1.5, 0.0, 1.0}; // (a zero-extent y axis: -0.0 .. 0.0)
    for (int i = 0; i < 200000; i++) {
      Tri t{};
      for (int k = 0; k < 9; k++) t.v[k] = special[rng() % special.size()];
      double bounds[6];
      for (int k = 0; k < 6; k++) bounds[k] = (i & 1) ? special[rng() % special.size()] : unit[k];
      check_triangle(t, bounds);
    }
    // degenerate: two or three equal vertices, collinear vertices, a vertex exactly on the bounds
    std::uniform_real_distribution<double> u(-3.0, 3.0);
    for (int i = 0; i < 100000; i++) {
      Tri t{};
      for (int k = 0; k < 9; k++) t.v[k] = u(rng);
      const int kind = i % 4;
      if (kind == 0) for (int k = 0; k < 3; k++) t.v[3 + k] = t.v[k];
      if (kind == 1) for (int k = 0; k < 3; k++) t.v[3 + k] = t.v[6 + k] = t.v[k];
      if (kind == 2) for (int k = 0; k < 3; k++) t.v[6 + k] = t.v[k] + 2.0 * (t.v[3 + k] - t.v[k]);
      double bounds[6];
      was::Box b;
      was::tri_box(t.v, t.v + 3, t.v + 6, b);
      for (int k = 0; k < 3; k++) { bounds[k] = b.lo[k]; bounds[3 + k] = kind == 3 ? b.hi[k] + 1.0 : b.hi[k]; }
      check_triangle(t, bounds);
    }
  }
  ok = group("special and degenerate triangles") && ok;

  // 10^6 random triangles on the bounds of all of them
  {
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(-10.0, 10.0), small(-1e-3, 1e-3);
    const double bounds[6] = {-10.0, -10.0, -10.0, 10.0, 10.0, 10.0};
    for (int i = 0; i < 1000000; i++) {
      Tri t{};
      for (int k = 0; k < 3; k++) t.v[k] = u(rng);
      for (int k = 3; k < 9; k++) t.v[k] = (i % 3) ? t.v[k % 3] + small(rng) : u(rng);
      check_triangle(t, bounds);
    }
  }
  ok = group("1 000 000 random triangles") && ok;
  return ok ? 0 : 1;
}
