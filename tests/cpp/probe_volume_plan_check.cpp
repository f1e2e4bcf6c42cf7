// Host-side check of the probe volume's host arithmetic (rpt_amd/csrc/probe_volume_plan.h): the checks of a grid's numbers in
// the header's order, the probe count that fits no allocation, the points or rays per piece — the pieces cover [0, n) once and
// in order —, the layout of a piece's arrays inside one allocation — aligned, disjoint, inside `words`, the first-hit query's
// four present whenever rays run, a host caller's point channels all staged and a device caller's none —, a host caller's
// volume staged whole, and the launch's grid: one lane per point.
// Usage: probe_volume_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../rpt_amd/csrc/probe_volume_plan.h"

using namespace rptvolume;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    checks++;                                                                    \
    if (!(cond)) {                                                               \
      failures++;                                                                \
      std::printf("FAIL probe_volume_plan_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                            \
  } while (0)

static const uint64_t Mi = 1ull << 20;
static bool says(const char* why, const char* word) { return why && std::strstr(why, word); }

// by hand
static void sizes() {
  CHECK(launch_blocks(1) == 1 && launch_blocks(256) == 1 && launch_blocks(257) == 2 && launch_blocks(4 * Mi) == 16384);
  CHECK(CH_POINT == (CH_VALUE | CH_COVERED | CH_INSIDE) && CH_HIT == 15u && (CH_POINT | CH_HIT) == CH_ALL);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double o[3] = {0.0, -1.0, 2.0}, h[3] = {1.0, 0.5, 2.0};
  CHECK(!bad_grid(1, 1, 1, o, h) && !bad_grid(4, 1, 3, o, h));
  CHECK(says(bad_grid(0, 1, 1, o, h), "count of 0") && says(bad_grid(1, 0, 1, o, h), "count of 0") && says(bad_grid(1, 1, 0, o, h), "count of 0"));
  for (int a = 0; a < 3; a++)
    for (double bad : {0.0, -1.0, inf, nan}) {
      double hh[3] = {1.0, 0.5, 2.0};
      hh[a] = bad;
      CHECK(says(bad_grid(2, 2, 2, o, hh), "spacing is not finite and positive"));
      CHECK(says(bad_grid(0, 2, 2, o, hh), "count of 0")); // the counts first
    }
  for (int a = 0; a < 3; a++)
    for (double bad : {inf, -inf, nan}) {
      double oo[3] = {0.0, -1.0, 2.0};
      oo[a] = bad;
      CHECK(says(bad_grid(2, 2, 2, oo, h), "origin is not finite"));
    }
  bool fits = false;
  CHECK(probe_count(3, 2, 2, fits) == 12 && fits);
  CHECK(probe_count(1u << 20, 1u << 20, 1u << 15, fits) == PROBES_MAX && fits);
  CHECK(probe_count(1u << 20, 1u << 20, (1u << 15) + 1, fits) == 0 && !fits);
  CHECK(probe_count(0xffffffffu, 0xffffffffu, 0xffffffffu, fits) == 0 && !fits); // refused, not wrapped
  // the piece: the wish within the bound, never above n, never 0
  CHECK(piece(257, 0, POINTS_PIECE) == 257 && piece(257, 64, POINTS_PIECE) == 64 && piece(257, 3, POINTS_PIECE) == 3);
  CHECK(piece(10 * Mi, 0, POINTS_PIECE) == POINTS_PIECE && piece(10 * Mi, 8 * Mi, POINTS_PIECE) == POINTS_PIECE);
  CHECK(piece(1, 1000, 5) == 1 && piece(0, 0, 5) == 1 && piece(1ull << 40, 0, ~0ull) == 1ull << 30);
  // a device caller of the point form: nothing of the handle's; of the ray form: the first-hit query's four
  CHECK(layout(600, CH_POINT, false, true).words == 0 && layout(600, CH_POINT, false, true).has == 0);
  const Layout ray = layout(600, CH_ALL, true, true);
  CHECK(ray.has == CH_HIT && ray.t == 0 && ray.position == 600 && ray.normal == 2400 && ray.object == 4200 && ray.words == 4500);
  // a host caller, one ray: t 1 -> 2 words, three times 3 -> 4, one int32 array and the two byte arrays 2 each
  const Layout odd = layout(1, CH_ALL, true, false);
  CHECK(odd.has == CH_ALL && odd.t == 0 && odd.position == 2 && odd.normal == 6 && odd.value == 10 && odd.object == 14 &&
        odd.covered == 16 && odd.inside == 18 && odd.words == 20);
  // a host caller's points, VALUE alone
  const Layout val = layout(5, CH_VALUE, false, false);
  CHECK(val.has == CH_VALUE && val.value == 0 && val.words == 16);
  // a volume of 12 probes with valid bytes: 324 words of coefficients, 12 bytes -> 2 words
  const Staged s = stage_volume(12, true);
  CHECK(s.ok && s.coeffs == 0 && s.coeff_words == 324 && s.valid == 324 && s.valid_bytes == 12 && s.words == 326);
  const Staged t = stage_volume(1, false);
  CHECK(t.ok && t.coeff_words == 27 && t.valid == 28 && t.valid_bytes == 0 && t.words == 28);
  CHECK(stage_volume(PROBES_MAX, true).ok && !stage_volume(PROBES_MAX + 1, true).ok);
}

static void cover() {
  // the pieces of a call cover [0, n) once and in order
  for (uint64_t n : std::vector<uint64_t>{1, 2, 3, 64, 257, 1000, 5 * Mi + 7})
    for (uint64_t asked : std::vector<uint64_t>{0, 1, 3, 64, 256, 300, 1ull << 40})
      for (uint64_t bound : std::vector<uint64_t>{1, 7, 4096, POINTS_PIECE, ~0ull}) {
        const uint64_t p = piece(n, asked, bound);
        CHECK(p >= 1 && p <= n && p <= bound && (!asked || p <= asked) && p <= (1ull << 30));
        if (n > 100000 && p < 1000) continue; // (the walk below, not for 5 Mi pieces of 1)
        uint64_t next = 0, count = 0;
        for (uint64_t base = 0; base < n; base += p) {
          const uint64_t m = std::min(p, n - base);
          if (base != next || !m) break;
          next = base + m;
          count++;
        }
        CHECK(next == n && count == (n + p - 1) / p);
      }
  const uint64_t pieces[] = {1, 2, 3, 7, 8, 9, 255, 256, 257, 600, 65535, 4 * Mi};
  for (uint64_t pc : pieces) {
    CHECK((uint64_t)launch_blocks(pc) * BLOCK >= pc && ((uint64_t)launch_blocks(pc) - 1) * BLOCK < pc);
    for (uint32_t ch = 0; ch <= CH_ALL; ch++)
      for (int rays = 0; rays < 2; rays++)
        for (int on_device = 0; on_device < 2; on_device++) {
          if (!rays && (ch & CH_HIT)) continue; // (a point has no such channel: refused before any layout)
          const Layout l = layout(pc, ch, rays != 0, on_device != 0);
          if (!on_device) CHECK((l.has & (ch & CH_POINT)) == (ch & CH_POINT)); // a host caller's point channels are all staged
          else CHECK(!(l.has & CH_POINT));                                      // a device caller's are written in place
          CHECK(rays ? (l.has & CH_HIT) == CH_HIT : !(l.has & CH_HIT));
          struct Span { uint64_t lo, hi; };
          std::vector<Span> spans;
          if (l.has & CH_T) spans.push_back({l.t * 8, l.t * 8 + pc * 8});
          if (l.has & CH_POSITION) spans.push_back({l.position * 8, l.position * 8 + 3 * pc * 8});
          if (l.has & CH_NORMAL) spans.push_back({l.normal * 8, l.normal * 8 + 3 * pc * 8});
          if (l.has & CH_VALUE) spans.push_back({l.value * 8, l.value * 8 + 3 * pc * 8});
          if (l.has & CH_OBJECT) spans.push_back({l.object * 8, l.object * 8 + pc * 4});
          if (l.has & CH_COVERED) spans.push_back({l.covered * 8, l.covered * 8 + pc});
          if (l.has & CH_INSIDE) spans.push_back({l.inside * 8, l.inside * 8 + pc});
          bool ok = true;
          for (size_t i = 0; i < spans.size(); i++) {
            ok = ok && spans[i].lo % 16 == 0 && spans[i].hi <= l.words * 8;
            for (size_t j = 0; j < i; j++) ok = ok && (spans[i].lo >= spans[j].hi || spans[j].lo >= spans[i].hi);
          }
          CHECK(ok);
          CHECK(spans.empty() == (l.words == 0));
        }
  }
  // a staged volume: the coefficients, then the bytes, aligned and inside `words`
  for (uint64_t probes : std::vector<uint64_t>{1, 2, 12, 27, 32768, 1ull << 40})
    for (int has_valid = 0; has_valid < 2; has_valid++) {
      const Staged s = stage_volume(probes, has_valid != 0);
      CHECK(s.ok && s.coeffs == 0 && s.coeff_words == 27 * probes && s.valid % 2 == 0 && s.valid >= s.coeff_words);
      CHECK(s.valid_bytes == (has_valid ? probes : 0) && s.valid * 8 + s.valid_bytes <= s.words * 8 && s.words % 2 == 0);
    }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
