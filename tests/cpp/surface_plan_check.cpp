// Host-side check of rptgpu_hit_surface's sizing arithmetic (rpt_amd/csrc/surface_plan.h): the walk's columns — a grid that is
// a multiple of the block, within the block and byte caps, never empty, whose launches stay inside it — and the layout of a
// piece's arrays inside one allocation: aligned, disjoint, inside `words`, T and OBJECT present whenever the walk reads them.
// Usage: surface_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rpt_amd/csrc/surface_plan.h"

using namespace rptsurface;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    checks++;                                                               \
    if (!(cond)) {                                                          \
      failures++;                                                           \
      std::printf("FAIL surface_plan_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                       \
  } while (0)

static const uint64_t Mi = 1ull << 20;

// by hand
static void sizes() {
  const Columns one = columns(1, 0, 0); // a flat scene: every tree one leaf, no nest — a level and a frame all the same
  CHECK(one.threads == 256 && one.levels == 1 && one.frames == 1 && one.defer_words == 8 * 256 && one.frame_words == 12 * 256);
  const Columns c600 = columns(600, 23, 1);
  CHECK(c600.threads == 768 && c600.levels == 23 && c600.defer_words == 23ull * 8 * 768 && c600.frame_words == 12 * 768);
  CHECK(launch_blocks(600, c600) == 3 && launch_blocks(1, c600) == 1 && launch_blocks(256, c600) == 1 && launch_blocks(257, c600) == 2);
  const Columns big = columns(4 * Mi, 20, 2); // 1 472 B per thread: the block cap binds, not the bytes
  CHECK(big.threads == COLUMN_BLOCKS_MAX * BLOCK);
  CHECK(launch_blocks(4 * Mi, big) == COLUMN_BLOCKS_MAX); // the grid strides over the piece
  CHECK(columns(4 * Mi, 30, 2).threads == 992 * BLOCK);   // 2 112 B per thread: 512 MiB hold 992 blocks' columns
  const Columns tall = columns(4 * Mi, 1000, 40); // 67 840 B per thread: the byte cap binds
  CHECK(tall.threads == 7680 && (tall.defer_words + tall.frame_words) * 8 <= COLUMN_BYTES_MAX);
  const Columns huge = columns(4 * Mi, 1u << 20, 1u << 16); // beyond any cap: one block, whatever it costs
  CHECK(huge.threads == BLOCK);
  CHECK(needs_walk(CH_CHILD) && needs_walk(CH_PRIMITIVE) && needs_walk(CH_BARYCENTRIC) && needs_walk(CH_ALL));
  CHECK(!needs_walk(CH_T) && !needs_walk(CH_OBJECT) && !needs_walk(CH_T | CH_OBJECT) && !needs_walk(0));
  // a device caller that names everything: nothing of the handle's is needed
  CHECK(layout(600, CH_ALL, true).words == 0 && layout(600, CH_ALL, true).has == 0);
  // ... that names the walk's channels only: the pair
  const Layout pair = layout(600, CH_PRIMITIVE | CH_BARYCENTRIC, true);
  CHECK(pair.has == (CH_T | CH_OBJECT) && pair.t == 0 && pair.object == 600 && pair.words == 600 + 300);
  // ... T only: no walk, nothing
  CHECK(layout(600, CH_T, true).words == 0);
  // a host caller, one odd piece: t 1 -> 2 words, barycentric 3 -> 4, three int32 arrays of 1 -> 2 each
  const Layout odd = layout(1, CH_ALL, false);
  CHECK(odd.has == CH_ALL && odd.t == 0 && odd.barycentric == 2 && odd.object == 6 && odd.child == 8 && odd.primitive == 10 && odd.words == 12);
  // a host caller that names CHILD alone still gets the pair
  CHECK(layout(5, CH_CHILD, false).has == (CH_T | CH_OBJECT | CH_CHILD));
  CHECK(layout(5, CH_OBJECT, false).has == CH_OBJECT);
}

static void cover() {
  const uint64_t pieces[] = {1, 2, 3, 255, 256, 257, 600, 65535, 4 * Mi};
  const uint32_t levels[] = {0, 1, 7, 33, 200, 5000}, frames[] = {0, 1, 3, 64};
  for (uint64_t piece : pieces)
    for (uint32_t lv : levels)
      for (uint32_t fr : frames) {
        const Columns c = columns(piece, lv, fr);
        CHECK(c.threads >= BLOCK && c.threads % BLOCK == 0 && c.threads <= COLUMN_BLOCKS_MAX * BLOCK);
        CHECK(c.levels >= 1 && c.levels >= lv && c.frames >= 1 && c.frames >= fr);
        CHECK(c.defer_words == (uint64_t)c.levels * 8 * c.threads && c.frame_words == (uint64_t)c.frames * 12 * c.threads);
        CHECK(c.threads == BLOCK || (c.defer_words + c.frame_words) * 8 <= COLUMN_BYTES_MAX);
        CHECK(c.threads <= (piece + BLOCK - 1) / BLOCK * BLOCK); // no column without a ray
        for (uint64_t m : {(uint64_t)1, piece / 2 + 1, piece}) {
          const uint32_t blocks = launch_blocks(m, c);
          CHECK(blocks >= 1 && (uint64_t)blocks * BLOCK <= c.threads); // every thread of the grid owns a column
          CHECK((uint64_t)blocks * BLOCK >= m || blocks == c.threads / BLOCK); // one lane per ray, or the whole grid in strides
        }
        // the deepest entry a walk may touch lies inside the arrays
        CHECK(((uint64_t)(c.levels - 1) * 8 + 7) * c.threads + (c.threads - 1) < c.defer_words);
        CHECK(((uint64_t)(c.frames - 1) * 12 + 11) * c.threads + (c.threads - 1) < c.frame_words);
      }
  for (uint64_t piece : pieces)
    for (uint32_t ch = 1; ch <= CH_ALL; ch++)
      for (int on_device = 0; on_device < 2; on_device++) {
        const Layout l = layout(piece, ch, on_device != 0);
        if (!on_device) CHECK((l.has & ch) == ch);             // a host caller's channels are all staged
        else CHECK(!(l.has & ~(CH_T | CH_OBJECT)));             // a device caller's arrays are written in place
        if (needs_walk(ch)) CHECK((l.has & CH_T) || (on_device && (ch & CH_T)));
        if (needs_walk(ch)) CHECK((l.has & CH_OBJECT) || (on_device && (ch & CH_OBJECT)));
        struct Span { uint64_t lo, hi; };
        std::vector<Span> spans;
        if (l.has & CH_T) spans.push_back({l.t * 8, l.t * 8 + piece * 8});
        if (l.has & CH_BARYCENTRIC) spans.push_back({l.barycentric * 8, l.barycentric * 8 + 3 * piece * 8});
        if (l.has & CH_OBJECT) spans.push_back({l.object * 8, l.object * 8 + piece * 4});
        if (l.has & CH_CHILD) spans.push_back({l.child * 8, l.child * 8 + piece * 4});
        if (l.has & CH_PRIMITIVE) spans.push_back({l.primitive * 8, l.primitive * 8 + piece * 4});
        bool ok = true;
        for (size_t i = 0; i < spans.size(); i++) {
          ok = ok && spans[i].lo % 16 == 0 && spans[i].hi <= l.words * 8;
          for (size_t j = 0; j < i; j++) ok = ok && (spans[i].lo >= spans[j].hi || spans[j].lo >= spans[i].hi);
        }
        CHECK(ok);
        CHECK(spans.empty() == (l.words == 0));
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
