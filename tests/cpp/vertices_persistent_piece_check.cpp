// Host-side check of the piece of rptgpu_trace_vertices under RPT_FLAG_VERTICES_PERSISTENT (rpt_amd/csrc/render_plan.h
// vertices_persistent_piece): the smaller of vertices_piece — rays_piece's bound and, for a host caller, the staging cap of the
// named channels — and what rpt_paths_vertices' 32-bit work counter holds (rays_persistent_piece).  The loop api_vertices.cpp
// runs with it covers [0, n) once and in order without an empty piece, and both caps hold for every channel subset.
// Usage: vertices_persistent_piece_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>

#include "../../rpt_amd/csrc/render_plan.h"

using namespace rptplan;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    checks++;                                                                            \
    if (!(cond)) {                                                                       \
      failures++;                                                                        \
      std::printf("FAIL vertices_persistent_piece_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                                    \
  } while (0)

static const uint64_t MAX32 = 0xffffffffull;
static const uint32_t BATCH = RPT_PATHS_BATCH_MAX;
static const uint32_t WAVES = RPT_PATHS_WAVES_PER_CU_MAX;
static const uint32_t ALL = (1u << VERTICES_CHANNEL_BITS) - 1u;

// by hand
static void sizes() {
  const uint32_t nb = 256 * WAVES;
  // the tests' shapes and the bench's, device arrays: nothing is cut, the piece is vertices_piece's
  CHECK(vertices_persistent_piece(777, 0, 1ull << 22, false, 3, 8, ALL, nb, BATCH) == 777);
  CHECK(vertices_persistent_piece(777, 100, 1ull << 22, false, 3, 8, ALL, nb, BATCH) == 100);
  CHECK(vertices_persistent_piece(1, 0, 1ull << 22, true, 1, 0, 1u, nb, BATCH) == 1);
  CHECK(vertices_persistent_piece(1920ull * 1080, 0, 1ull << 24, false, 4, 8, ALL, nb, BATCH) ==
        vertices_piece(1920ull * 1080, 0, 1ull << 24, false, 4, 8, ALL));
  // a host caller with every channel: 4 x (9 x 152 + 4) = 5 488 B per ray, so the staging cap cuts first
  CHECK(vertices_staging_bytes(1, 4, 8, ALL) == 5488);
  CHECK(vertices_persistent_piece(1920ull * 1080, 0, 1ull << 24, true, 4, 8, ALL, nb, BATCH) == VERTICES_STAGING_MAX / 5488);
  // a wished-for piece of 2^29 rays at 16 samples is 2^33 items: the counter cuts it (LENGTH alone stages 64 B per ray)
  const uint64_t room = views_dead_room(nb, BATCH);
  CHECK(vertices_persistent_piece(1ull << 30, 1ull << 29, 1ull << 30, false, 16, 0, 1u, nb, BATCH) == (MAX32 - room) / 16);
  CHECK(vertices_persistent_piece(1ull << 30, 1ull << 29, 1ull << 30, true, 16, 0, 1u, nb, BATCH) == VERTICES_STAGING_MAX / 64);
  // never empty
  CHECK(vertices_persistent_piece(10, 0, 1ull << 22, true, 0xffffffffu, 254, ALL, nb, BATCH) == 1);
  CHECK(vertices_persistent_piece(0, 0, 0, true, 4, 8, ALL, nb, BATCH) == 1);
}

// the call's loop over its pieces: [0, n) once, in order, no empty piece, both caps for every piece
static bool covered(uint64_t n, uint64_t piece, bool host, uint32_t it, uint32_t mb, uint32_t ch, uint32_t nb) {
  if (!piece) return false;
  uint64_t next = 0, steps = 0;
  for (uint64_t base = 0; base < n; base += piece) {
    if (++steps > 256) { // (a long call: the pieces in between are all alike — on to the last one)
      base = (n - 1) / piece * piece;
      next = base;
    }
    const uint64_t m = std::min(piece, n - base);
    if (base != next || !m) return false;
    if (m > MAX32 || work_items((uint32_t)m, it, 1) + views_dead_room(nb, BATCH) > MAX32) return false;
    if (host && m > 1 && vertices_staging_bytes(m, it, mb, ch) > VERTICES_STAGING_MAX) return false; // (one ray is still a piece)
    next = base + m;
  }
  return next == n;
}

// every channel subset, both kinds of caller
static void subsets() {
  const uint64_t ns[] = {1, 65, 1ull << 21, 1ull << 31};
  const uint64_t askeds[] = {0, 100, 1ull << 29};
  const uint32_t iters[] = {1, 5, 1u << 16};
  const uint32_t bounces[] = {0, 254};
  const uint64_t target = 1ull << 30;
  const uint32_t nb = 256 * WAVES;
  for (uint32_t ch = 1; ch <= ALL; ch++)
    for (uint64_t n : ns)
      for (uint64_t asked : askeds)
        for (uint32_t it : iters)
          for (uint32_t mb : bounces)
            for (int host = 0; host < 2; host++) {
              const uint64_t p = vertices_persistent_piece(n, asked, target, host != 0, it, mb, ch, nb, BATCH);
              const uint64_t pv = vertices_piece(n, asked, target, host != 0, it, mb, ch);
              bool ok = p >= 1 && p <= pv && p == rays_persistent_piece(pv, it, nb, BATCH);
              ok = ok && covered(n, p, host != 0, it, mb, ch, nb);
              // the counter's cap is tight where it is the one that cut
              if (ok && p < pv) ok = (p + 1) * it + views_dead_room(nb, BATCH) > MAX32 || p == 1;
              if (!ok) {
                std::printf("FAIL case: channels %u n %llu asked %llu iterations %u max_bounces %u host %d -> piece %llu\n", ch,
                            (unsigned long long)n, (unsigned long long)asked, it, mb, host, (unsigned long long)p);
                CHECK(ok);
                return;
              }
              checks++;
            }
}

// the launch plans the driver can make of such a piece fit the counter
static void plans() {
  const uint64_t wants[] = {1, 65, 777, 1ull << 20, 1ull << 29};
  const uint32_t iters[] = {1, 3, 5, 33, 1000};
  const int cus[] = {1, 64, 256};
  const uint32_t chunks[] = {0, 1, 2, 16};
  const uint64_t lbufs[] = {24, 48, 1ull << 20, 1ull << 34};
  for (uint64_t want : wants)
    for (uint32_t it : iters)
      for (int cu : cus) {
        const uint32_t blocks_max = (uint32_t)cu * WAVES;
        const uint64_t m = vertices_persistent_piece(want, want, 1ull << 30, false, it, 8, ALL, blocks_max, BATCH);
        CHECK(m >= 1 && m <= want);
        for (uint32_t chunk : chunks)
          for (uint64_t lbuf : lbufs)
            for (int flat = 0; flat < 2; flat++) {
              const PersistentPlan pl = plan_persistent((uint32_t)m, it, 8, cu, 8, lbuf, 0, -1, chunk, flat != 0, false, flat != 0);
              bool ok = pl.nblocks <= blocks_max && pl.spp_l >= 1 && pl.spp_l <= it && pl.chunk >= 1;
              ok = ok && !views_items(m, pl.spp_l, pl.chunk, pl.nblocks, BATCH).capped;
              ok = ok && (uint64_t)pl.n_launch * pl.spp_l >= it && (uint64_t)(pl.n_launch - 1) * pl.spp_l < it;
              if (!ok) { CHECK(ok); return; }
              checks++;
            }
      }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "subsets")) subsets();
  else if (!std::strcmp(s, "plans")) plans();
  else { std::printf("FAIL unknown section '%s'\n", s); return 1; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
