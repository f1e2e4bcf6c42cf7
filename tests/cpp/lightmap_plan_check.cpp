// Host-side check of rptgpu_bake_lightmap's sizing arithmetic (rpt_amd/csrc/lightmap_plan.h): the clamp of a triangle's
// texel-space extent — a superset of the texels whose centres lie inside it, inside the map, never inverted, never a cast out
// of range, for huge, negative, infinite and NaN coordinates —, the pieces, which tile the map exactly, and the layout of a
// piece's compacted arrays: aligned, disjoint, inside `words`, 52 B of input per texel; and `sliver`, which says when the
// clamp is NOT such a superset for the header's ROUNDED edge tests: every triangle of a search over near-collinear ones that
// covers a texel outside its clamp must be named a sliver, and ordinary triangles must not be.
// Usage: lightmap_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../rpt_amd/csrc/lightmap_plan.h"

using namespace rptlightmap;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    checks++;                                                                \
    if (!(cond)) {                                                           \
      failures++;                                                            \
      std::printf("FAIL lightmap_plan_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                        \
  } while (0)

static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();
static bool is(TexelRange r, uint32_t lo, uint32_t hi) { return r.lo == lo && r.hi == hi; }
static bool empty(TexelRange r) { return r.lo == 0 && r.hi == 0; }

// by hand
static void clamp() {
  CHECK(is(clamp_range(1.0, 15.0, 16), 0, 16));      // the quad of the tests: floor(1) - 1 = 0, ceil(15) + 1 = 16
  CHECK(is(clamp_range(3.5, 4.5, 16), 2, 6));        // centres 3.5 and 4.5 are texels 3 and 4; one more either side
  CHECK(is(clamp_range(3.2, 3.2, 16), 2, 5));        // a degenerate extent still gets a range
  CHECK(is(clamp_range(-5.0, 2.0, 16), 0, 3));       // hangs over the left edge
  CHECK(is(clamp_range(14.0, 40.0, 16), 13, 16));    // ... over the right one
  CHECK(is(clamp_range(-1e300, 1e300, 16), 0, 16));  // much larger than the map
  CHECK(is(clamp_range(-INF, INF, 16), 0, 16));
  CHECK(is(clamp_range(0.0, 0.0, 1), 0, 1) && is(clamp_range(1.0, 1.0, 1), 0, 1) && is(clamp_range(0.3, 0.6, 1), 0, 1));
  CHECK(is(clamp_range(-0.0, -0.0, 4), 0, 1));       // a_max = -0.0 is >= 0: texel 0's neighbourhood
  CHECK(is(clamp_range(16.0, 20.0, 16), 15, 16));    // touches the map's far edge: generous, not empty
  CHECK(empty(clamp_range(16.5, 20.0, 16)));         // wholly above
  CHECK(empty(clamp_range(-20.0, -0.5, 16)));        // wholly below
  CHECK(empty(clamp_range(1e300, 1e301, 16)) && empty(clamp_range(-1e301, -1e300, 16)));
  CHECK(empty(clamp_range(INF, INF, 16)) && empty(clamp_range(-INF, -INF, 16)));
  CHECK(empty(clamp_range(NaN, 3.0, 16)) && empty(clamp_range(3.0, NaN, 16)) && empty(clamp_range(NaN, NaN, 16)));
  CHECK(empty(clamp_range(5.0, 4.0, 16)));           // inverted input
  CHECK(empty(clamp_range(0.0, 1.0, 0)));            // no map
  const uint32_t big = 0xFFFFFFFFu;                  // the widest map a uint32 names
  CHECK(is(clamp_range(-1e9, 1e12, big), 0, big));
  CHECK(is(clamp_range(4294967290.25, 4294967293.5, big), 4294967289u, big));
  CHECK(is(clamp_range(4294967290.25, 4294967292.5, big), 4294967289u, 4294967294u));
  CHECK(is(clamp_range(4294967295.0, 1e30, big), 4294967294u, big));
  CHECK(empty(clamp_range(4294967295.5, 1e30, big)));
  CHECK(streams_fit(65536, 65536, 0) && !streams_fit(65536, 65536, 1) && streams_fit(1, 1, 0xFFFFFFFFu) && !streams_fit(2, 1, 0xFFFFFFFFu));
  CHECK(streams_fit(0xFFFFFFFFu, 1, 1) && !streams_fit(0xFFFFFFFFu, 1, 2) && !streams_fit(0xFFFFFFFFu, 0xFFFFFFFFu, 0));
  CHECK(texels(0xFFFFFFFFu, 0xFFFFFFFFu) == 0xFFFFFFFE00000001ull);
}

// the clamp against its definition: every texel whose centre lies in [a_min, a_max] is inside the range, the range is
// inside the map and never inverted
static void cover() {
  const uint32_t sizes[] = {1, 2, 7, 13, 16, 4096};
  const double at[] = {-1e300, -1e9, -17.0, -1.5, -1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.49, 3.5, 3.51, 6.0, 6.5,
                       7.0, 12.5, 13.0, 15.5, 16.0, 16.5, 17.0, 4095.5, 4096.0, 4097.0, 1e9, 1e300, INF, -INF, NaN};
  for (uint32_t size : sizes)
    for (double lo : at)
      for (double hi : at) {
        const TexelRange r = clamp_range(lo, hi, size);
        CHECK(r.lo <= r.hi && r.hi <= size);
        CHECK(r.lo < r.hi || empty(r)); // an empty range is {0, 0}
        bool inside = true;
        for (uint32_t i = 0; i < size; i++) {
          const double c = (double)i + 0.5;
          if (lo <= c && c <= hi) inside = inside && r.lo <= i && i < r.hi;
        }
        CHECK(inside);
      }
}

// the header's rule, as kernels/lightmap.inc and tests/lightmap_model.py state it (this file is built with -ffp-contract=off)
static double edge(double px, double py, double qx, double qy, double cx, double cy) {
  return (qx - px) * (cy - py) - (qy - py) * (cx - px);
}
struct Tri {
  double x[3], y[3], area;
};
static Tri tri(const double uv[6], uint32_t w, uint32_t h) {
  Tri t;
  for (int k = 0; k < 3; k++) { t.x[k] = uv[2 * k] * (double)w; t.y[k] = uv[2 * k + 1] * (double)h; }
  t.area = edge(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
  return t;
}
static bool covers(const Tri& t, double cx, double cy) {
  const double e1 = edge(t.x[1], t.y[1], t.x[2], t.y[2], cx, cy), e2 = edge(t.x[2], t.y[2], t.x[0], t.y[0], cx, cy),
               e3 = edge(t.x[0], t.y[0], t.x[1], t.y[1], cx, cy);
  return t.area > 0.0 ? (e1 >= 0.0 && e2 >= 0.0 && e3 >= 0.0) : (e1 <= 0.0 && e2 <= 0.0 && e3 <= 0.0);
}
static double min3(const double* v) { return std::fmin(std::fmin(v[0], v[1]), v[2]); }
static double max3(const double* v) { return std::fmax(std::fmax(v[0], v[1]), v[2]); }
// does the triangle cover a texel its clamp leaves out?
static bool escapes(const Tri& t, uint32_t w, uint32_t h) {
  if (!(t.area != 0.0) || !std::isfinite(t.area)) return false;
  const TexelRange rx = clamp_range(min3(t.x), max3(t.x), w), ry = clamp_range(min3(t.y), max3(t.y), h);
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++)
      if (!(rx.lo <= x && x < rx.hi && ry.lo <= y && y < ry.hi) && covers(t, (double)x + 0.5, (double)y + 0.5)) return true;
  return false;
}
static bool is_sliver(const Tri& t, uint32_t w, uint32_t h) { return sliver(t.area, min3(t.x), max3(t.x), min3(t.y), max3(t.y), w, h); }
static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform() { // in [0, 1)
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg_state >> 11) * 0x1p-53;
}

static void slivers() {
  // one found by hand: vertices on the diagonal up to an ulp, area 2.9e-15, covering texel (10, 10) of a 16 x 16 map,
  // 1.9 texels beyond its furthest vertex
  const double found[6] = {0x1.650a87471b06cp-2, 0x1.650a87471b06cp-2, 0x1.4c5d63b09e87dp-2, 0x1.4c5d63b09e87cp-2,
                           0x1.1314877c90929p-1, 0x1.1314877c90929p-1};
  const Tri f = tri(found, 16, 16);
  CHECK(f.area != 0.0 && std::fabs(f.area) < 1e-13 && covers(f, 10.5, 10.5) && escapes(f, 16, 16) && is_sliver(f, 16, 16));
  // the search: three points on a random line through the map, each coordinate moved by up to two ulps
  int escaped = 0, named = 0;
  const uint32_t maps[][2] = {{16, 16}, {13, 7}, {64, 48}};
  for (const auto& wh : maps)
    for (int i = 0; i < 20000; i++) {
      const double ox = uniform(), oy = uniform(), dx = uniform() - 0.5, dy = uniform() - 0.5;
      double uv[6];
      for (int k = 0; k < 3; k++) {
        const double s = 2.0 * uniform() - 1.0;
        uv[2 * k] = ox + s * dx; uv[2 * k + 1] = oy + s * dy;
        for (int c = 0; c < 2; c++) {
          const int ulps = (int)(uniform() * 5.0) - 2;
          for (int n = 0; n < (ulps < 0 ? -ulps : ulps); n++)
            uv[2 * k + c] = std::nextafter(uv[2 * k + c], ulps < 0 ? -1e300 : 1e300);
        }
      }
      if (i % 4 == 0) { uv[1] = uv[0]; uv[3] = uv[2]; uv[5] = uv[4]; uv[3] = std::nextafter(uv[3], 0.0); } // on the diagonal, as above
      const Tri t = tri(uv, wh[0], wh[1]);
      const bool e = escapes(t, wh[0], wh[1]), s = is_sliver(t, wh[0], wh[1]);
      escaped += e; named += s;
      CHECK(!e || s); // the clamp is a superset for everything that is not named a sliver
    }
  CHECK(escaped >= 50);   // the search does find triangles the clamp alone gets wrong
  CHECK(named >= escaped);
  // ordinary triangles are not slivers: a texel-sized one, thin but honest ones, huge ones
  const double fat[][6] = {{0.1, 0.1, 0.2, 0.1, 0.1, 0.2}, {0.0, 0.0, 1.0, 0.0, 0.0, 1.0}, {0.5, 0.5, 0.5001, 0.5, 0.5, 0.5001},
                           {0.0, 0.0, 1.0, 1.0, 1.0, 1.0 - 1e-7}, {-50.0, -40.0, 60.0, -45.0, 0.0, 70.0},
                           {0.05, 0.05, 0.05, 0.45, 0.45, 0.05}, {-1e6, -1e6, 1e6, -1e6, 0.0, 1e6}};
  for (const auto& uv : fat)
    for (const auto& wh : maps) {
      const Tri t = tri(uv, wh[0], wh[1]);
      CHECK(!is_sliver(t, wh[0], wh[1]) && !escapes(t, wh[0], wh[1]));
    }
  for (uint32_t size : {16u, 2048u, 4096u, 65536u}) { // an atlas cell's triangle at the far corner of large maps
    const double s = (double)size, uv[6] = {(s - 6.0 + 0.25) / s, (s - 6.0 + 0.25) / s, (s - 0.25) / s, (s - 5.5) / s, (s - 5.5) / s, (s - 0.25) / s};
    CHECK(!is_sliver(tri(uv, size, size), size, size));
  }
  // errs to true: overflowing terms, an area that underflows
  CHECK(sliver(1.0, -1e200, 1e200, -1e200, 1e200, 16, 16));
  CHECK(sliver(0x1p-1060, 0.0, 0x1p-500, 0.0, 0x1p-500, 16, 16));
  CHECK(sliver(0.0, 0.0, 1.0, 0.0, 1.0, 16, 16));
}

static void pieces() {
  CHECK(piece(256, 0, 1000) == 256 && piece(256, 7, 1000) == 7 && piece(256, 7, 3) == 3 && piece(256, 0, 0) == 1);
  CHECK(piece(1ull << 32, 0, 1ull << 40) == PIECE_MAX && piece(1ull << 32, 1ull << 30, 1ull << 40) == PIECE_MAX);
  CHECK(piece(1, 64, 1000) == 1);
  const uint64_t ns[] = {1, 2, 91, 256, 1000, (1ull << 32)}, asks[] = {0, 1, 7, 64, 1ull << 40}, fits[] = {0, 1, 5, 1000, 1ull << 40};
  for (uint64_t n : ns)
    for (uint64_t asked : asks)
      for (uint64_t fit : fits) {
        const uint64_t p = piece(n, asked, fit);
        CHECK(p >= 1 && p <= n && p <= PIECE_MAX && (fit == 0 || p <= fit) && (asked == 0 || p <= asked));
        if (piece_count(n, p) > 5000) continue; // (the tiling is checked where it is short)
        uint64_t covered = 0, count = 0;
        for (uint64_t base = 0; base < n; base += p) {
          const uint64_t len = piece_len(base, n, p);
          CHECK(len >= 1 && len <= p && base == covered);
          covered += len;
          count++;
        }
        CHECK(covered == n && count == piece_count(n, p));
      }
  for (uint64_t pc : {(uint64_t)1, (uint64_t)2, (uint64_t)7, (uint64_t)64, (uint64_t)1001, PIECE_MAX})
    for (int irr = 0; irr < 2; irr++)
      for (int ao = 0; ao < 2; ao++) {
        const Compact c = compact(pc, irr != 0, ao != 0);
        struct Span { uint64_t lo, hi; };
        std::vector<Span> spans = {{c.point * 8, c.point * 8 + 24 * pc}, {c.normal * 8, c.normal * 8 + 24 * pc}, {c.ids * 8, c.ids * 8 + 4 * pc}};
        if (irr) spans.push_back({c.irradiance * 8, c.irradiance * 8 + 24 * pc});
        if (ao) spans.push_back({c.ao * 8, c.ao * 8 + 8 * pc});
        bool ok = true;
        for (size_t i = 0; i < spans.size(); i++) {
          ok = ok && spans[i].lo % 16 == 0 && spans[i].hi <= c.words * 8;
          for (size_t j = 0; j < i; j++) ok = ok && (spans[i].lo >= spans[j].hi || spans[j].lo >= spans[i].hi);
        }
        CHECK(ok);
        CHECK(c.words * 8 <= (52 + (irr ? 24 : 0) + (ao ? 8 : 0)) * pc + 16 * 5); // 52 B per texel in, 32 B out, and the padding
      }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "clamp")) clamp();
  else if (!std::strcmp(s, "cover")) cover();
  else if (!std::strcmp(s, "pieces")) pieces();
  else if (!std::strcmp(s, "slivers")) slivers();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
