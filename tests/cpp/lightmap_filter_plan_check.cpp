// Host-side check of rptgpu_filter_lightmap's sizing arithmetic (rpt_amd/csrc/lightmap_filter_plan.h): the limits of a map,
// the workspace — arrays aligned, disjoint, inside `words`, the per-texel bytes the public header states (113 at 3 words with
// a variance), the dilation's second copy and flags inside the columns they alias —, a host caller's staging, the ping-pong's
// sets, and the launch geometry: every texel of every map covered, the grid inside the launch limits.
// Usage: lightmap_filter_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rpt_amd/csrc/lightmap_filter_plan.h"

using namespace rptlightmapfilter;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    checks++;                                                                       \
    if (!(cond)) {                                                                  \
      failures++;                                                                   \
      std::printf("FAIL lightmap_filter_plan_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                               \
  } while (0)

static void limits() {
  CHECK(map_fits(1, 1) && map_fits(65536, 65536) && map_fits(0xFFFFFFFFu, 1) && map_fits(1, 0xFFFFFFFFu));
  CHECK(!map_fits(0, 4) && !map_fits(4, 0) && !map_fits(65536, 65537) && !map_fits(0xFFFFFFFFu, 2) && !map_fits(0xFFFFFFFFu, 0xFFFFFFFFu));
  CHECK(words_ok(1) && words_ok(3) && !words_ok(0) && !words_ok(2) && !words_ok(4) && !words_ok(0xFFFFFFFFu));
  CHECK(LEVELS_MAX == 8 && step(0) == 1 && step(1) == 2 && step(7) == 128);
  CHECK(rounds(0, 5, 9) == 0 && rounds(3, 5, 9) == 3 && rounds(9, 5, 9) == 9 && rounds(10, 5, 9) == 9 && rounds(0xFFFFFFFFu, 9, 5) == 9);
  for (uint32_t l = 0; l < LEVELS_MAX; l++) CHECK(source_set(l) == l % 2 && result_set(l + 1) == 1 - source_set(l));
  CHECK(result_set(0) == 0 && result_set(1) == 1 && result_set(2) == 0 && result_set(8) == 0);
}

struct Span {
  uint64_t lo, hi; // f64 words
};
static bool disjoint(const std::vector<Span>& s) {
  for (size_t i = 0; i < s.size(); i++)
    for (size_t j = i + 1; j < s.size(); j++)
      if (s[i].lo < s[j].hi && s[j].lo < s[i].hi) return false;
  return true;
}

static void workspace_layout() {
  const uint64_t sizes[] = {1, 2, 7, 8, 9, 91, 256, 325, 1170, 2048ull * 2048, (1ull << 32) - 1, 1ull << 32};
  for (uint64_t n : sizes)
    for (uint32_t comps : {1u, 3u})
      for (bool var : {false, true}) {
        const Workspace w = workspace(n, comps, var);
        std::vector<Span> s = {{w.position, w.position + 3 * n}, {w.normal, w.normal + 3 * n}, {w.c[0], w.c[0] + comps * n},
                               {w.c[1], w.c[1] + comps * n}, {w.valid, w.valid + (n + 7) / 8}};
        if (var) {
          s.push_back({w.v[0], w.v[0] + n});
          s.push_back({w.v[1], w.v[1] + n});
        }
        CHECK(disjoint(s));
        for (const Span& a : s) CHECK(a.lo % 2 == 0 && a.hi <= w.words);
        CHECK(w.has_variance == var);
        // the bytes the public header states, up to the alignment of seven arrays
        const uint64_t per_texel = 8 * (6 + 2 * comps + (var ? 2 : 0)) + 1;
        CHECK(8 * w.words >= per_texel * n && 8 * w.words <= per_texel * n + 7 * 16);
        // the dilation's second flags inside the position columns, its second copy inside the two column sets, which are
        // adjacent — and neither touches the validity bytes, its first flags
        CHECK(w.flags2 == w.position && (n + 7) / 8 <= 3 * n);
        CHECK(w.pong == w.c[0] && w.pong + comps * n <= w.c[1] + comps * n && w.c[1] >= w.c[0]);
        CHECK(w.pong + comps * n <= w.valid && w.flags2 + (n + 7) / 8 <= w.valid);
      }
  CHECK(8 * workspace(2048ull * 2048, 3, true).words == 113ull * 2048 * 2048); // (a size without padding: exactly the header's)
  const uint64_t n = 1024;
  CHECK(8 * workspace(n, 3, true).words == 113 * n && 8 * workspace(n, 3, false).words == 97 * n);
  CHECK(8 * workspace(n, 1, true).words == 81 * n && 8 * workspace(n, 1, false).words == 65 * n);
}

static void staging() {
  const uint64_t sizes[] = {1, 2, 7, 91, 325, 2048ull * 2048, 1ull << 32};
  for (uint64_t n : sizes)
    for (uint32_t comps : {1u, 3u})
      for (int mode = 0; mode < 3; mode++) {
        const bool var = mode > 0, outv = mode > 1;
        const Stage t = stage(n, comps, var, outv);
        std::vector<Span> s = {{t.position, t.position + 3 * n}, {t.normal, t.normal + 3 * n}, {t.values, t.values + comps * n},
                               {t.out, t.out + comps * n}, {t.owner, t.owner + (n + 1) / 2}};
        if (var) s.push_back({t.variance, t.variance + n});
        if (outv) s.push_back({t.out_variance, t.out_variance + n});
        CHECK(disjoint(s));
        for (const Span& a : s) CHECK(a.lo % 2 == 0 && a.hi <= t.words);
        const uint64_t per_texel = 4 + 8 * (6 + 2 * comps) + (var ? 8 : 0) + (outv ? 8 : 0);
        CHECK(8 * t.words >= per_texel * n && 8 * t.words <= per_texel * n + 7 * 16);
        CHECK(t.has_variance == var && t.has_out_variance == outv);
      }
}

// every texel (x, y) of the map is some lane's: x from blockIdx.x * 64 + threadIdx.x, y from blockIdx.y * 4 + threadIdx.y on
// in strides of 4 * grid.y
static void launches() {
  const uint32_t shapes[][2] = {{1, 1}, {13, 7}, {64, 4}, {65, 5}, {130, 9}, {2048, 2048}, {1, 262140}, {1, 262141}, {3, 1000003},
                                {0xFFFFFFFFu, 1}, {1, 0xFFFFFFFFu}, {65536, 65536}};
  for (const auto& s : shapes) {
    const uint32_t w = s[0], h = s[1];
    const Grid g = grid(w, h);
    CHECK(g.x >= 1 && g.y >= 1 && g.y <= GRID_Y_MAX && g.x <= (1u << 26));
    CHECK((uint64_t)g.x * BLOCK_X >= w && (uint64_t)(g.x - 1) * BLOCK_X < w); // covers the width, with no empty block column
    CHECK((uint64_t)(g.x - 1) * BLOCK_X + (BLOCK_X - 1) <= 0xFFFFFFFFull);     // a lane's x is a uint32
    // rows: the first pass covers [0, 4 * g.y), the stride is 4 * g.y — together every row; no empty block row
    CHECK((uint64_t)(g.y - 1) * BLOCK_Y < h);
    CHECK((uint64_t)g.y * BLOCK_Y >= h || g.y == GRID_Y_MAX);
    const uint64_t n = texels(w, h);
    const uint32_t fb = finish_blocks(n);
    CHECK(fb >= 1 && fb <= FINISH_GRID_MAX && ((uint64_t)fb * FINISH_BLOCK >= n || fb == FINISH_GRID_MAX));
  }
  CHECK(grid(64, 4).x == 1 && grid(64, 4).y == 1 && grid(65, 5).x == 2 && grid(65, 5).y == 2 && grid(130, 9).x == 3 && grid(130, 9).y == 3);
  CHECK(grid(1, 262140).y == 65535 && grid(1, 262141).y == 65535 && grid(1, 0xFFFFFFFFu).y == 65535);
  CHECK(BLOCK_X * BLOCK_Y == 256 && FINISH_BLOCK == 256);
  // by enumeration on a small map with a small cut: the rows a block walks
  for (uint32_t h : {1u, 4u, 5u, 9u, 23u}) {
    const Grid g = grid(7, h);
    std::vector<int> seen(h, 0);
    for (uint32_t by = 0; by < g.y; by++)
      for (uint32_t ty = 0; ty < BLOCK_Y; ty++)
        for (uint64_t y = (uint64_t)by * BLOCK_Y + ty; y < h; y += (uint64_t)g.y * BLOCK_Y) seen[y]++;
    for (uint32_t y = 0; y < h; y++) CHECK(seen[y] == 1);
  }
}

int main(int argc, char** argv) {
  const char* section = argc > 1 ? argv[1] : "";
  if (!std::strcmp(section, "limits")) limits();
  else if (!std::strcmp(section, "workspace")) workspace_layout();
  else if (!std::strcmp(section, "staging")) staging();
  else if (!std::strcmp(section, "launches")) launches();
  else {
    std::printf("FAIL unknown section '%s'\n", section);
    return 2;
  }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
