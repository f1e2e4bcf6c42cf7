// Host-side check of the piece arithmetic of rptgpu_trace_rays (rpt_amd/csrc/render_plan.h rays_piece): the pieces cover
// the rays once, and every pass the planner then makes for a piece fits the workspace's target and the 32-bit slot index.
// Usage: rays_piece_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>

#include "../../rpt_amd/csrc/render_plan.h"

using namespace rptplan;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    checks++;                                                                  \
    if (!(cond)) {                                                             \
      failures++;                                                              \
      std::printf("FAIL rays_piece_check.cpp:%d: %s\n", __LINE__, #cond);      \
    }                                                                          \
  } while (0)

static const uint64_t Mi = 1ull << 20, GiB = 1ull << 30;

static void sizes() {
  CHECK(RAYS_PIECE_MAX == 4 * Mi);
  CHECK(rays_piece(1, 0, 128 * Mi) == 1);
  CHECK(rays_piece(1000, 0, 128 * Mi) == 1000);          // a small call is one piece
  CHECK(rays_piece(4 * Mi, 0, 128 * Mi) == 4 * Mi);
  CHECK(rays_piece(4 * Mi + 1, 0, 128 * Mi) == 4 * Mi);  // the default cap
  CHECK(rays_piece(1ull << 40, 0, 128 * Mi) == 4 * Mi);
  CHECK(rays_piece(1000, 100, 128 * Mi) == 100);         // the tests' hook
  CHECK(rays_piece(50, 100, 128 * Mi) == 50);
  CHECK(rays_piece(64 * Mi, 16 * Mi, 128 * Mi) == 16 * Mi); // ... may also ask for more than the default
  CHECK(rays_piece(64 * Mi, 16 * Mi, 2 * Mi) == 2 * Mi);    // ... but never for more than a pass holds
  CHECK(rays_piece(64 * Mi, 0, 1 * Mi) == 1 * Mi);
  CHECK(rays_piece(64 * Mi, 0, 0) == 1);                 // (a target of nothing: still progress)
  CHECK(rays_piece(1ull << 40, 1ull << 40, ~0ull) == RPT_MAX_PATHS_PER_PASS); // whatever the target says: 32-bit slots
  CHECK(rays_piece_count(1000, 100) == 10 && rays_piece_count(1001, 100) == 11 && rays_piece_count(99, 100) == 1);
  CHECK(rays_piece_count(1, 1) == 1 && rays_piece_count(4 * Mi + 1, 4 * Mi) == 2);
}

// the pieces are consecutive, none is empty, none is longer than `piece`, together they are the n rays
static void cover() {
  const uint64_t ns[] = {1, 2, 99, 100, 101, 200, 201, 257, 4 * Mi - 1, 4 * Mi, 4 * Mi + 1, 9 * Mi + 5};
  const uint64_t asks[] = {0, 1, 7, 100, 128, 5 * Mi};
  for (uint64_t n : ns)
    for (uint64_t asked : asks) {
      if (asked == 1 && n > 1000) continue; // (a loop of millions shows nothing more)
      const uint64_t piece = rays_piece(n, asked, 128 * Mi);
      uint64_t covered = 0, count = 0, last = 0;
      for (uint64_t base = 0; base < n; base += piece) {
        last = std::min(piece, n - base);
        covered += last;
        count++;
      }
      CHECK(piece >= 1 && piece <= n);
      CHECK(covered == n && count == rays_piece_count(n, piece));
      CHECK(last >= 1 && last <= piece && last == n - (count - 1) * piece);
    }
}

// what the planner does with a piece as its frame: every pass's paths fit the target and 32 bits, at every stage of the
// record-ratio learning, for every sample count — the driver computes npix * s_chunk in 32 bits
static void passes() {
  const uint64_t targets[] = {0, 1 * Mi, 3 * Mi + 17, 128 * Mi, RPT_MAX_PATHS_PER_PASS};
  const uint32_t spps[] = {1, 4, 16, 1000, 100000};
  const double ratios[] = {0.0, 1.3, 9.0};
  const uint64_t ns[] = {1, 257, 1 * Mi, 4 * Mi + 1, 700 * Mi};
  for (uint64_t target_paths : targets)
    for (uint64_t n : ns)
      for (uint64_t asked : {(uint64_t)0, (uint64_t)100, 600 * Mi}) {
        PassInput in{};
        in.npix = 1; in.iterations = 1; in.remaining = 1;
        in.ratio = 9.0; // max_bounces + 1: room for every level of every path
        in.per_slot = wavefront_slot_bytes(2, true, true, false);
        in.target_paths = target_paths; in.budget_bytes = 240 * GiB; in.free_bytes = target_paths ? -1 : (int64_t)(200 * GiB);
        in.free_percent = 85;
        const uint64_t pass_target = plan_pass(in).target;
        const uint64_t piece = rays_piece(n, asked, pass_target);
        CHECK(piece <= std::max<uint64_t>(1, pass_target) && piece <= RPT_MAX_PATHS_PER_PASS);
        for (uint32_t spp : spps)
          for (double rec_ratio : ratios) {
            PassInput pi = in;
            pi.npix = (uint32_t)piece; pi.iterations = spp; pi.remaining = spp;
            pi.rec_ratio = rec_ratio; pi.ratio = pass_ratio(rec_ratio, 8);
            const PassPlan pp = plan_pass(pi);
            const uint64_t paths = piece * (uint64_t)pp.s_chunk;
            CHECK(pp.s_chunk >= 1 && pp.s_chunk <= spp);
            CHECK(paths <= std::max<uint64_t>(piece, pp.target)); // one sample of every ray, or what the target holds
            CHECK(paths <= 0xffffffffull && pass_slots((uint32_t)piece, pp) <= 0xffffffffull);
          }
      }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else if (!std::strcmp(s, "passes")) passes();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
