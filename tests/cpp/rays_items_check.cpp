// Host-side check of the piece cap of rptgpu_trace_rays / rptgpu_bake_probes under RPT_FLAG_RAYS_PERSISTENT
// (rpt_amd/csrc/render_plan.h rays_persistent_piece): a piece of the caller's rays or probes is the "frame" of rpt_paths_rays'
// launches, so it is cut to what the kernel's 32-bit work counter holds — views_items' arithmetic with npix = m, asked at one
// sample per item and the most blocks a device may hold.  Whatever launch plan plan_persistent then makes over the piece
// (fewer blocks, longer items, fewer samples per launch) fits the counter too, which is what render_persistent checks.
// Usage: rays_items_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>

#include "../../rpt_amd/csrc/render_plan.h"

using namespace rptplan;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    checks++;                                                                 \
    if (!(cond)) {                                                            \
      failures++;                                                             \
      std::printf("FAIL rays_items_check.cpp:%d: %s\n", __LINE__, #cond);     \
    }                                                                         \
  } while (0)

static const uint64_t MAX32 = 0xffffffffull;
static const uint32_t BATCH = RPT_PATHS_BATCH_MAX;
static const uint32_t WAVES = RPT_PATHS_WAVES_PER_CU_MAX;

// by hand
static void sizes() {
  // the tests' shapes and the bench's: nothing is cut
  CHECK(rays_persistent_piece(777, 4, 256 * WAVES, BATCH) == 777);
  CHECK(rays_persistent_piece(1, 1, 256 * WAVES, BATCH) == 1);
  CHECK(rays_persistent_piece(16, 33, 256 * WAVES, BATCH) == 16);
  CHECK(rays_persistent_piece(1920ull * 1080, 4, 256 * WAVES, BATCH) == 1920ull * 1080);
  CHECK(rays_persistent_piece(65536, 64, 256 * WAVES, BATCH) == 65536);
  // rays_piece's default, at any sample count a call of that size would run
  CHECK(rays_persistent_piece(RAYS_PIECE_MAX, 4, 256 * WAVES, BATCH) == RAYS_PIECE_MAX);
  CHECK(rays_persistent_piece(RAYS_PIECE_MAX, 1000, 256 * WAVES, BATCH) == RAYS_PIECE_MAX);
  // a wished-for piece of 2^29 rays (RPTGPU_RAYS_PIECE; rays_piece lets it through up to RPT_MAX_PATHS_PER_PASS) at 16 samples
  // is 2^33 items: cut to the counter less the dead claims' room, over the samples
  const uint64_t room = views_dead_room(256 * WAVES, BATCH);
  CHECK(room == 256ull * 32 * 1088);
  CHECK(rays_persistent_piece(1ull << 29, 16, 256 * WAVES, BATCH) == (MAX32 - room) / 16);
  CHECK(rays_persistent_piece(1ull << 29, 7, 256 * WAVES, BATCH) == std::min<uint64_t>(1ull << 29, (MAX32 - room) / 7));
  CHECK(rays_persistent_piece(1ull << 29, 8, 256 * WAVES, BATCH) < (1ull << 29));
  CHECK(rays_persistent_piece(1ull << 29, 4, 256 * WAVES, BATCH) == (1ull << 29));
  // never empty: one ray of more samples than the counter holds is still a piece (the driver then refuses its plan, or
  // plan_persistent packs the samples into longer items)
  CHECK(rays_persistent_piece(10, 0xffffffffu, 256 * WAVES, BATCH) == 1);
  CHECK(rays_persistent_piece(0, 4, 256 * WAVES, BATCH) == 1);
}

// the capped piece under every launch plan the driver can make of it
static void plans() {
  const uint64_t pieces[] = {1, 5, 65, 777, 1ull << 20, RAYS_PIECE_MAX, 1ull << 28, 1ull << 29, RPT_MAX_PATHS_PER_PASS};
  const uint32_t iters[] = {1, 3, 4, 33, 64, 1000, 1u << 16};
  const int cus[] = {1, 64, 256};
  const int per_cus[] = {1, 8, 32, 64};
  const uint32_t chunks[] = {0, 1, 2, 16, 1000};
  const uint64_t lbufs[] = {24, 1ull << 20, 1ull << 34, 1ull << 40};
  for (uint64_t want : pieces)
    for (uint32_t it : iters)
      for (int cu : cus) {
        const uint32_t blocks_max = (uint32_t)cu * WAVES;
        const uint64_t m = rays_persistent_piece(want, it, blocks_max, BATCH);
        CHECK(m >= 1 && m <= want && m <= MAX32);
        CHECK(work_items((uint32_t)m, it, 1) + views_dead_room(blocks_max, BATCH) <= MAX32);
        if (m < want) CHECK((m + 1) * it + views_dead_room(blocks_max, BATCH) > MAX32); // the cap is tight
        for (int per_cu : per_cus)
          for (uint32_t chunk : chunks)
            for (uint64_t lbuf : lbufs)
              for (int flat = 0; flat < 2; flat++) {
                const PersistentPlan pl = plan_persistent((uint32_t)m, it, 8, cu, per_cu, lbuf, 0, -1, chunk, flat != 0, false, flat != 0);
                bool ok = pl.nblocks <= blocks_max && pl.spp_l >= 1 && pl.spp_l <= it && pl.chunk >= 1;
                // what render_persistent checks of the plan it runs
                ok = ok && !views_items(m, pl.spp_l, pl.chunk, pl.nblocks, BATCH).capped;
                ok = ok && work_items((uint32_t)m, pl.spp_l, pl.chunk) + (uint64_t)pl.nblocks * (64 + BATCH) <= MAX32;
                // ... and the launches cover the call's samples
                ok = ok && (uint64_t)pl.n_launch * pl.spp_l >= it && (uint64_t)(pl.n_launch - 1) * pl.spp_l < it;
                if (!ok) { CHECK(ok); return; }
                checks++;
              }
      }
}

// at the counter's edge
static void edge() {
  const uint32_t blocks[] = {1, 256, 8192, 1u << 20};
  const uint32_t spps[] = {1, 3, 64, 1u << 20, 0xffffffffu};
  const uint64_t ms[] = {1, 1000, 4ull << 20, MAX32 - 1, MAX32, 1ull << 40};
  for (uint32_t nb : blocks)
    for (uint32_t spp : spps)
      for (uint64_t m : ms) {
        const uint64_t got = rays_persistent_piece(m, spp, nb, BATCH);
        const ViewsItems vi = views_items(m, spp, 1, nb, BATCH);
        CHECK(got == std::max<uint64_t>(1, vi.m)); // views_items' arithmetic with npix = m, and never empty
        if (vi.m) CHECK(got * spp + views_dead_room(nb, BATCH) <= MAX32);
      }
  const uint64_t room = views_dead_room(8192, BATCH);
  CHECK(rays_persistent_piece(MAX32 - room, 1, 8192, BATCH) == MAX32 - room);     // the counter's last value is used
  CHECK(rays_persistent_piece(MAX32 - room + 1, 1, 8192, BATCH) == MAX32 - room); // one more ray is not
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "plans")) plans();
  else if (!std::strcmp(s, "edge")) edge();
  else { std::printf("FAIL unknown section '%s'\n", s); return 1; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
