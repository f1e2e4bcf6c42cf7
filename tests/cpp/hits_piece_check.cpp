// Host-side check of the piece arithmetic of rptgpu_first_hits (rpt_amd/csrc/render_plan.h hits_pass_max, hits_piece): the
// pieces cover [0, n) once and in order, none is empty, none exceeds the wish, the pass bound or 32 bits — for n = 0, n = 1, a
// bound of 1 and n above 2^32.
// Usage: hits_piece_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>

#include "../../rpt_amd/csrc/render_plan.h"

using namespace rptplan;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    checks++;                                                             \
    if (!(cond)) {                                                        \
      failures++;                                                         \
      std::printf("FAIL hits_piece_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                     \
  } while (0)

static const uint64_t Mi = 1ull << 20, GiB = 1ull << 30, NONE = ~0ull;

// by hand
static void sizes() {
  CHECK(HITS_PIECE_MAX == 4 * Mi && HITS_PIECE_MAX <= RPT_MAX_PATHS_PER_PASS && HITS_PIECE_MAX <= 0xffffffffull);
  CHECK(hits_pass_max(0) == 1 && hits_pass_max(1) == 1 && hits_pass_max(5) == 5);
  CHECK(hits_pass_max(128 * Mi) == HITS_PIECE_MAX && hits_pass_max(NONE) == HITS_PIECE_MAX);
  CHECK(hits_piece(0, 0, NONE) == 1);                 // (n == 0 returns before any piece; the loop below runs zero times)
  CHECK(hits_piece(1, 0, NONE) == 1 && hits_piece(1, 256, 1) == 1);
  CHECK(hits_piece(600, 0, NONE) == 600);             // a small call is one piece
  CHECK(hits_piece(600, 256, NONE) == 256);           // the tests' hook: 256, 256, 88
  CHECK(hits_piece(600, 256, 100) == 100);            // ... within the pass bound
  CHECK(hits_piece(600, 0, 1) == 1 && hits_piece(600, 256, 1) == 1); // a bound of 1: one ray per piece
  CHECK(hits_piece(33 * Mi, 0, NONE) == HITS_PIECE_MAX);
  CHECK(hits_piece(33 * Mi, 0, 3 * Mi) == 3 * Mi);    // what the device has room for
  CHECK(hits_piece(33 * Mi, 64 * Mi, NONE) == HITS_PIECE_MAX); // a wish beyond the cap
  CHECK(hits_piece((1ull << 32) + 5, 0, NONE) == HITS_PIECE_MAX);
  CHECK(hits_piece(1ull << 40, 1ull << 40, NONE) == HITS_PIECE_MAX);
  CHECK(hits_piece(NONE, NONE, NONE) == HITS_PIECE_MAX);
}

// rptgpu_first_hits' loop: consecutive, none empty, together [0, n), never more than the piece, the wish or the bound
static void cover() {
  const uint64_t ns[] = {0, 1, 2, 255, 256, 257, 600, 4 * Mi, 4 * Mi + 3, 33 * Mi, (1ull << 32) + 5, 1ull << 36};
  const uint64_t asks[] = {0, 1, 7, 256, 5 * Mi, 64 * Mi};
  const uint64_t bounds[] = {1, 1000, 1 * Mi, 3 * Mi + 17, 128 * Mi, NONE};
  for (uint64_t n : ns)
    for (uint64_t asked : asks)
      for (uint64_t bound : bounds) {
        const uint64_t piece = hits_piece(n, asked, bound);
        CHECK(piece >= 1 && piece <= hits_pass_max(bound) && piece <= bound && piece <= HITS_PIECE_MAX);
        CHECK(!asked || piece <= asked);
        CHECK(!n || piece <= n);
        const uint64_t count = (n + piece - 1) / piece;
        // the last piece, in closed form (also where a loop of billions would show nothing more)
        CHECK(!n || ((count - 1) * piece < n && n - (count - 1) * piece <= piece && n - (count - 1) * piece >= 1));
        if (count > 200000) continue;
        uint64_t next = 0, seen = 0;
        bool ok = true;
        for (uint64_t base = 0; base < n; base += piece) {
          const uint64_t m = std::min(piece, n - base);
          ok = ok && base == next && m >= 1 && m <= piece && m <= 0xffffffffull;
          next = base + m;
          seen++;
        }
        CHECK(ok && next == n);
        CHECK(seen == count);
      }
}

// with the planner's own target for a scene with deep trees: what the driver computes (api_hits.cpp first_hits)
static void planned() {
  for (uint64_t target_paths : {(uint64_t)0, 1 * Mi, 128 * Mi, (uint64_t)RPT_MAX_PATHS_PER_PASS})
    for (int64_t free_gib : {1, 16, 200}) {
      PassInput in{};
      in.npix = 1; in.iterations = 1; in.remaining = 1;
      in.ratio = 1.0;
      in.per_slot = wavefront_slot_bytes(2, true, true, false);
      in.target_paths = target_paths; in.budget_bytes = 240 * GiB; in.free_bytes = target_paths ? -1 : free_gib * (int64_t)GiB;
      in.free_percent = 85;
      const uint64_t target = plan_pass(in).target;
      CHECK(target >= 1);
      const uint64_t piece = hits_piece(33 * Mi, 0, target);
      CHECK(piece >= 1 && piece <= target && piece <= HITS_PIECE_MAX);
      CHECK(hits_piece(600, 256, target) == std::min<uint64_t>(256, target));
    }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else if (!std::strcmp(s, "planned")) planned();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
