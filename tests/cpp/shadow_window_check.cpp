// Host-side check of the shadow ray's window in the two-ray query (RPT_SHADOW_WINDOW: rpt_amd/csrc/scene_plan.h
// axis_flat_mesh, kernels/paths_flat.inc run_beyond).  Stand-alone, no GPU; built with -ffp-contract=off like the kernels
// and with -fsanitize=address,undefined (tests/test_shadow_window_host.py).  Two parts:
//  numbers: the two expressions the rule compares, restated here operation for operation — the plane table's quotient
//           q = (c - o_k) / d_k with mm = fmax(q, EPSILON) (run_slabs), and Triangle::intersect's
//           time = dot(pn, v1 - o) / dot(pn, d) of a record with pn zero off the axis and v1[k] = c (shapes.inc tri_plane) —
//           over seeded draws of (c, o_k, d_k, pn_k, t_stop): whenever tri_accept's guards pass,
//           time >= mm * (1 - 2^-50), and the rule never drops a case with time <= t_stop;
//  flags:   the PRODUCT's derivation (axis_flat_mesh, and plan_flat's bit 24 of plane_idx) over records made by the product's
//           fill_trix: C2's five walls and its light are marked; a quad tilted by one ulp, a mesh with one vertex off the
//           plane, a transformed mesh and an object that is no table user are not.
// Usage: shadow_window_check [draws]; prints "ok <checks> checks, <draws> draws" or one "FAIL" line per failed check (exit status 1).
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rpt_amd/csrc/mesh_records.h"
#include "../../rpt_amd/csrc/scene_plan.h"

static long checks = 0, failures = 0;
#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    checks++;                                                                                             \
    if (!(cond) && failures++ < 20) std::printf("FAIL shadow_window_check.cpp:%d: %s\n", __LINE__, #cond); \
  } while (0)

static const double EPSILON = 1e-12; // renderer.rs:14, kernels.inc

// ---- the device's expressions
static double dev_fmax(double a, double b) { return std::fmax(a, b); } // (a NaN loses, as on the device)
struct Case {
  double c, o, d, pn, t_stop;
};
struct Eval {
  double q, mm, cosine, time;
  bool guards, dropped;
};
static Eval eval(const Case& s, int axis) {
  Eval e;
  // run_slabs: both faces of the flat box are the plane c, so b_min == b_max == q for a candidate
  const double a = s.c - s.o;
  e.q = a / s.d;
  e.mm = dev_fmax(e.q, EPSILON);
  // tri_plane: dot(pn, v1 - o) / dot(pn, d), dot = (x + y) + z, with the two other axes' finite operands against pn = +-0
  double pn[3] = {0.0, -0.0, 0.0}, w[3] = {3.25, -17.5, 1e-3}, dd[3] = {0.5, -0.25, 0.125};
  pn[axis] = s.pn; w[axis] = a; dd[axis] = s.d;
  e.cosine = (pn[0] * dd[0] + pn[1] * dd[1]) + pn[2] * dd[2];
  e.time = ((pn[0] * w[0] + pn[1] * w[1]) + pn[2] * w[2]) / e.cosine;
  // tri_accept's guards that do not read the record; a NaN time passes them and then fails the barycentric test
  // (d2 = o + time * d is NaN, and u >= 0 is false), so it counts as a rejection here
  e.guards = !((std::fabs(e.cosine) < 1e-8) | (e.time < EPSILON)) && e.time == e.time;
  e.dropped = rpt_shadow_window_beyond(e.mm, s.t_stop); // run_beyond's comparison, the product's copy
  return e;
}

// ---- seeded draws
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() { // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static double unit() { return (double)(next_u64() >> 11) * 0x1p-53; }
static double ulps(double v, int n) {
  for (; n > 0; n--) v = std::nextafter(v, INFINITY);
  for (; n < 0; n++) v = std::nextafter(v, -INFINITY);
  return v;
}
static Case draw() {
  Case s;
  s.t_stop = 0.0;
  static const double PLANES[] = {0.0, -0.0, 556.0, 548.9, 548.8, 559.2, -1.0, 1e-3, 1e6, -3e-7};
  const uint64_t r = next_u64();
  s.c = (r & 1) ? PLANES[(r >> 1) % 10] : (unit() - 0.5) * 2000.0;
  switch ((r >> 8) % 6) {
    case 0: s.o = ulps(s.c, (int)((r >> 12) % 9) - 4); break;          // within a few ulp of the plane
    case 1: s.o = s.c + (unit() - 0.5) * 1e-9; break;
    case 2: s.o = (unit() - 0.5) * std::ldexp(1.0, (int)((r >> 12) % 2040) - 1020); break; // any magnitude
    default: s.o = s.c + (unit() - 0.5) * 1200.0; break;               // inside a room
  }
  switch ((r >> 24) % 8) {
    case 0: s.d = (r >> 28) & 1 ? 0.0 : -0.0; break;
    case 1: s.d = ((r >> 28) & 1 ? 1.0 : -1.0) * std::ldexp(unit(), -(int)((r >> 29) % 1074)); break; // tiny, down to subnormals
    case 2: s.d = -unit(); break;
    case 3: s.d = ((r >> 28) & 1 ? 1.0 : -1.0) * 1e-8 * (0.5 + unit()); break; // around the cosine guard
    default: s.d = unit() * 2.0 - 1.0; break;
  }
  const double sign = (r >> 40) & 1 ? 1.0 : -1.0;
  switch ((r >> 41) % 4) {
    case 0: s.pn = sign; break;
    case 1: s.pn = sign * ulps(1.0, (int)((r >> 44) % 5) - 2); break;
    default: s.pn = sign * std::ldexp(0.5 + unit() * 0.5, (int)((r >> 44) % 201) - 100); break; // 2^-101 .. 2^100
  }
  if (std::fabs(s.pn) < 0x1p-100) s.pn = sign * 0x1p-100; // (the host's precondition)
  const Eval e = eval(s, 1);
  switch ((r >> 54) % 8) { // t_stop: around the hit, around the rule's limit, and the special values
    case 0: s.t_stop = ulps(e.time, (int)((r >> 58) % 9) - 4); break;
    case 1: s.t_stop = e.mm * (1.0 - 0x1p-40 * (0.5 + unit())); break; // mm 2^12 to 3 * 2^12 doubles or so above it
    case 2: s.t_stop = e.time * (1.0 + (unit() - 0.5) * 0x1p-38); break;
    case 3: {
      static const double SPECIAL[] = {DBL_MAX, INFINITY, NAN, 0.0, 1e-12, 5e-324, -1.0, 1e300};
      s.t_stop = SPECIAL[(r >> 58) % 8];
    } break;
    default: s.t_stop = unit() * 1500.0; break;
  }
  return s;
}

static void numbers(long n) {
  long guarded = 0, dropped = 0, near = 0;
  const double low = 1.0 - 0x1p-50;
  for (long i = 0; i < n; i++) {
    const Case s = draw();
    const Eval e = eval(s, (int)(i % 3));
    if (e.dropped) dropped++;
    if (!e.guards) continue;
    guarded++;
    // q overflows where the three-rounding quotient does not (the proof's last case): the time is then at DBL_MAX's edge
    const bool edge = e.mm == INFINITY && e.time > DBL_MAX * low;
    CHECK(e.time >= e.mm * low || edge);
    CHECK(!(e.dropped && e.time <= s.t_stop));
    // the comparison on the patterns implies the inequality of the proof (a NaN t_stop aside: the query's result is false then)
    CHECK(!(e.dropped && s.t_stop == s.t_stop && !(e.mm > s.t_stop * (1.0 + 0x1p-40))));
    if (e.mm > s.t_stop * (1.0 + 0x1p-38) && s.t_stop > 0.0 && s.t_stop < 1e300) CHECK(e.dropped); // ... and is no more than 4x as cautious
    if (std::fabs(e.time - s.t_stop) <= 0x1p-40 * std::fabs(s.t_stop)) near++;
  }
  // the draws reach what they are for: accepted plane hits, drops, and hits within the margin of t_stop
  CHECK(guarded > n / 10);
  CHECK(dropped > n / 10);
  CHECK(near > n / 100);
}

// ---- the flag's derivation
struct Mesh {
  std::vector<rptdev::TriX> recs;
  double bounds[6];
};
static Mesh mesh_of(const std::vector<std::vector<double>>& tris) { // rows of v1 v2 v3; the bounds as the flattener folds them
  Mesh m;
  for (size_t j = 0; j < tris.size(); j++) {
    rptdev::TriX x;
    rptrec::fill_trix(tris[j].data(), x);
    m.recs.push_back(x);
    double lo[3], hi[3];
    rptrec::tri_box(tris[j].data(), lo, hi);
    if (j == 0) { std::memcpy(m.bounds, lo, sizeof lo); std::memcpy(m.bounds + 3, hi, sizeof hi); }
    else rptrec::merge_box(m.bounds, m.bounds + 3, lo, hi, m.bounds, m.bounds + 3);
  }
  return m;
}
static Mesh quad(const double p[4][3]) { // polygon(): the fan (p0, p1, p2), (p0, p2, p3)
  std::vector<std::vector<double>> t(2);
  const int fan[2][3] = {{0, 1, 2}, {0, 2, 3}};
  for (int j = 0; j < 2; j++)
    for (int v = 0; v < 3; v++)
      for (int k = 0; k < 3; k++) t[j].push_back(p[fan[j][v]][k]);
  return mesh_of(t);
}
static bool flat(const Mesh& m, int has_xf = 0, bool single_leaf = true, int kind = RPT_SHAPE_MESH) {
  return rptscene::axis_flat_mesh(kind, has_xf, single_leaf, m.bounds, m.recs.data(), m.recs.size());
}

static void flags() {
  // examples/cornell.rs: floor, ceiling, back wall, left wall, right wall, and the light
  const double C2[6][4][3] = {
      {{0.0, 0.0, 0.0}, {0.0, 0.0, 559.2}, {556.0, 0.0, 559.2}, {556.0, 0.0, 0.0}},
      {{0.0, 548.9, 0.0}, {556.0, 548.9, 0.0}, {556.0, 548.9, 559.2}, {0.0, 548.9, 559.2}},
      {{0.0, 0.0, 559.2}, {0.0, 548.9, 559.2}, {556.0, 548.9, 559.2}, {556.0, 0.0, 559.2}},
      {{556.0, 0.0, 0.0}, {556.0, 0.0, 559.2}, {556.0, 548.9, 559.2}, {556.0, 548.9, 0.0}},
      {{0.0, 0.0, 0.0}, {0.0, 548.9, 0.0}, {0.0, 548.9, 559.2}, {0.0, 0.0, 559.2}},
      {{343.0, 548.8, 227.0}, {343.0, 548.8, 332.0}, {213.0, 548.8, 332.0}, {213.0, 548.8, 227.0}}};
  std::vector<Mesh> walls;
  for (int i = 0; i < 6; i++) {
    walls.push_back(quad(C2[i]));
    CHECK(flat(walls.back()));
  }
  // each precondition on its own
  CHECK(!flat(walls[0], 1));                           // a transformed mesh
  CHECK(!flat(walls[0], 0, false));                    // a tree that is not one leaf
  CHECK(!flat(walls[0], 0, true, RPT_SHAPE_CUBE));     // not a mesh
  CHECK(!rptscene::axis_flat_mesh(RPT_SHAPE_MESH, 0, true, walls[0].bounds, nullptr, 0)); // no records
  { // tilted by one ulp: one corner of the ceiling leaves the plane
    double p[4][3];
    std::memcpy(p, C2[1], sizeof p);
    p[2][1] = std::nextafter(p[2][1], INFINITY);
    CHECK(!flat(quad(p)));
    std::memcpy(p, C2[4], sizeof p); // the wall in x = 0: one ulp off is the smallest subnormal
    p[1][0] = 5e-324;
    CHECK(!flat(quad(p)));
    p[1][0] = -0.0; // a zero of the other sign leaves the bounds' bits behind (lo is the first operand's zero, hi too)
    const Mesh m = quad(p);
    CHECK(flat(m) == (std::signbit(m.bounds[0]) == std::signbit(m.bounds[3])));
  }
  { // one vertex well off the plane
    double p[4][3];
    std::memcpy(p, C2[0], sizeof p);
    p[3][1] = 0.25;
    CHECK(!flat(quad(p)));
  }
  { // the box says flat, a record does not: v1 off the plane's bits, a normal with a second component, a normal out of range
    Mesh m = walls[1];
    m.recs[1].v1[1] = std::nextafter(m.recs[1].v1[1], 0.0);
    CHECK(!flat(m));
    m = walls[1]; m.recs[0].pn[0] = 5e-324; CHECK(!flat(m));
    m = walls[1]; m.recs[0].pn[2] = -1e-30; CHECK(!flat(m));
    m = walls[1]; m.recs[1].pn[1] = 0.0; CHECK(!flat(m));
    m = walls[1]; m.recs[1].pn[1] = NAN; CHECK(!flat(m));
    m = walls[1]; m.recs[1].pn[1] = INFINITY; CHECK(!flat(m));
    m = walls[1]; m.recs[1].pn[1] = 0x1p-101; CHECK(!flat(m));
    m = walls[1]; m.recs[1].pn[1] = -0x1p101; CHECK(!flat(m));
    m = walls[1]; m.recs[1].pn[1] = -0x1p100; CHECK(flat(m));
    m = walls[1]; m.recs[0].v1[0] = INFINITY; CHECK(!flat(m));
    m = walls[1]; m.bounds[1] = m.bounds[4] = INFINITY; CHECK(!flat(m));
    m = walls[1]; m.recs[0].pn[0] = -0.0; m.recs[0].pn[2] = -0.0; CHECK(flat(m)); // zeros of either sign
  }
  // through plan_flat: bit 24 of plane_idx beside the six slots, for table users only
  rptscene::FlatInput in;
  in.n_refs = 12; in.n_tris = 12;
  auto add = [&](int kind, int has_xf, const Mesh* m, bool with_recs) {
    rptscene::FlatObject o{kind, has_xf, {}};
    if (m) {
      std::memcpy(o.bounds, m->bounds, sizeof o.bounds);
      o.single_leaf = true;
      if (with_recs) { o.recs = m->recs.data(); o.n_recs = m->recs.size(); }
    }
    in.objects.push_back(o);
  };
  double tilted[4][3];
  std::memcpy(tilted, C2[2], sizeof tilted);
  tilted[1][2] = 332.0; tilted[2][2] = 332.0; // the back wall leaning forwards, onto a plane the table has (the light's edge)
  const Mesh lean = quad(tilted);
  for (int i = 0; i < 5; i++) add(RPT_SHAPE_MESH, 0, &walls[i], true);
  add(RPT_SHAPE_CUBE, 1, nullptr, false);
  add(RPT_SHAPE_CUBE, 1, nullptr, false);
  add(RPT_SHAPE_MESH, 0, &walls[5], true); // (the light's quad as an object of its own)
  add(RPT_SHAPE_MESH, 0, &walls[0], false); // a user whose records the caller did not hand over
  add(RPT_SHAPE_MESH, 1, &walls[0], true);  // transformed: not a table user
  in.n_lights = 1; in.light0_kind = RPT_LIGHT_OBJECT;
  {
    const rptscene::FlatPlan pl = rptscene::plan_flat(in);
    CHECK(pl.lay.plane_cnt != 0);
    for (int i = 0; i < 10; i++) {
      const bool user = pl.plane_use[i] != 0, mark = (pl.plane_idx[i] & RPT_PLANE_AXIS_FLAT) != 0;
      CHECK(user == (i < 5 || i == 7 || i == 8));
      CHECK(mark == (i < 5 || i == 7));
      CHECK((pl.plane_idx[i] >> 25) == 0u);
    }
  }
  { // the leaning wall in the back wall's place: a table user like before, without the mark
    rptscene::FlatObject& o = in.objects[2];
    std::memcpy(o.bounds, lean.bounds, sizeof o.bounds);
    o.recs = lean.recs.data(); o.n_recs = lean.recs.size();
    const rptscene::FlatPlan pl = rptscene::plan_flat(in);
    CHECK(pl.plane_use[2] != 0 && (pl.plane_idx[2] & RPT_PLANE_AXIS_FLAT) == 0);
    CHECK((pl.plane_idx[1] & RPT_PLANE_AXIS_FLAT) != 0 && (pl.plane_idx[3] & RPT_PLANE_AXIS_FLAT) != 0);
  }
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? std::atol(argv[1]) : 12000000L;
  numbers(n);
  flags();
  if (failures) return 1;
  std::printf("ok %ld checks, %ld draws\n", checks, n);
  return 0;
}
