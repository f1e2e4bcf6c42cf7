// Host-side check of rpt_amd/csrc/render_plan.h: the launch and pass plans of the render drivers, pinned to literal values.
// Usage: render_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
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
      std::printf("FAIL render_plan_check.cpp:%d: %s\n", __LINE__, #cond);     \
    }                                                                          \
  } while (0)

static const uint64_t GiB = 1ull << 30;
static const uint32_t P1080 = 1920u * 1080u;

// a persistent plan with the defaults of a large scene on 256 CUs: 2 blocks per CU, nothing held, free memory unknown
static PersistentPlan persistent(uint32_t npix, uint32_t spp, uint64_t lbuf_cap = 32 * GiB, uint32_t paths_chunk = 0,
                                 uint32_t max_bounces = 8, int64_t free_bytes = -1) {
  return plan_persistent(npix, spp, max_bounces, 256, 2, lbuf_cap, 0, free_bytes, paths_chunk, false, false, false);
}

static void launches() {
  PersistentPlan pl = persistent(P1080, 512); // 25.5 GB of per-sample radiance under the 32 GiB cap: one launch
  CHECK(pl.n_launch == 1 && pl.spp_l == 512);
  pl = plan_persistent(P1080, 512, 8, 256, 2, 32 * GiB, 0, 256 * GiB, 0, false, false, false);
  CHECK(pl.n_launch == 1 && pl.spp_l == 512);
  pl = persistent(P1080, 512, 32 * GiB, 0, 8, 40000000000ll); // growing: half of the free memory
  CHECK(pl.n_launch == 2 && pl.spp_l == 256);
  pl = plan_persistent(P1080, 512, 8, 256, 2, 32 * GiB, 32 * GiB, 1000, 0, false, false, false); // held up to the cap: free not asked
  CHECK(pl.n_launch == 1 && pl.spp_l == 512);
  pl = plan_persistent(P1080, 512, 8, 256, 2, 32 * GiB, 20 * GiB, 1000, 0, false, false, false); // what is held stays available
  CHECK(pl.n_launch == 2 && pl.spp_l == 256);
  // tests/test_gpu_parity.py's (chunk, spp_cap) grid at 7 spp: RPTGPU_LBUF_BYTES = npix x 24 x spp_cap
  const uint32_t npix = 48 * 27;
  const uint32_t grid[5][4] = {{1, 7, 1, 1}, {3, 7, 1, 3}, {16, 2, 4, 2}, {2, 3, 3, 2}, {5, 1, 7, 1}}; // chunk, cap, launches, chunk used
  for (const auto& g : grid) {
    pl = persistent(npix, 7, (uint64_t)npix * 24 * g[1], g[0]);
    CHECK(pl.n_launch == (7 + g[1] - 1) / g[1] && pl.n_launch == g[2]);
    CHECK(pl.chunk == g[3] && pl.spp_l * pl.n_launch >= 7 && pl.spp_l <= g[1]);
  }
}

static void chunk() {
  CHECK(persistent(P1080, 64).chunk == 16);
  CHECK(persistent(P1080, 64, 32 * GiB, 0, 3).chunk == 16);
  // a flat scene with the object filter, tracing long paths: 2 — not under RPT_FLAG_GENERAL_TRAVERSAL, not without the filter
  CHECK(plan_persistent(P1080, 64, 4, 256, 2, 32 * GiB, 0, -1, 0, true, false, true).chunk == 2);
  CHECK(plan_persistent(P1080, 64, 3, 256, 2, 32 * GiB, 0, -1, 0, true, false, true).chunk == 16);
  CHECK(plan_persistent(P1080, 64, 4, 256, 2, 32 * GiB, 0, -1, 0, true, true, true).chunk == 16);
  CHECK(plan_persistent(P1080, 64, 4, 256, 2, 32 * GiB, 0, -1, 0, true, false, false).chunk == 16);
  CHECK(plan_persistent(P1080, 64, 4, 256, 2, 32 * GiB, 0, -1, 0, false, false, true).chunk == 16);
  // halved while a lane (of 256 CUs x 8 x 64) would get fewer than 24 items
  CHECK(persistent(P1080, 16).chunk == 8);
  CHECK(persistent(64 * 36, 64).chunk == 1);
  CHECK(plan_persistent(64 * 36, 64, 8, 1, 2, 32 * GiB, 0, -1, 0, false, false, false).chunk == 8);
  // an explicit chunk is neither chosen nor halved, only clamped to [1, spp_l]
  CHECK(persistent(64 * 36, 64, 32 * GiB, 16).chunk == 16);
  CHECK(persistent(64 * 36, 7, 32 * GiB, 100).chunk == 7);
  CHECK(persistent(64 * 36, 7, 64 * 36 * 24 * 2, 100).chunk == 2);
}

static void items() {
  CHECK(work_items(P1080, 16, 8) == 2ull * P1080 && work_items(10, 7, 3) == 30 && work_items(10, 6, 3) == 20);
  const uint64_t item_limit = 0xFFFFFFF0ull - 256ull * 32 * (64 + 1024);
  CHECK(item_limit == 4286054384ull);
  // a frame just under 2^31 pixels at 10^6 spp with room for 21 845 samples per launch: 46 launches of 21 740, and the
  // item count only fits the 32-bit counter with one item per pixel and launch
  PersistentPlan pl = persistent(0x7fffffffu, 1000000, 1ull << 50);
  CHECK(pl.n_launch == 46 && pl.spp_l == 21740);
  CHECK(pl.n_items <= item_limit && pl.n_items == 0x7fffffffull && pl.chunk == 21740);
  CHECK(work_items(0x7fffffffu, pl.spp_l, pl.chunk - 1) > item_limit);
  // 2^30 pixels: three items per pixel and launch fit, four do not
  pl = persistent(1u << 30, 1000000, 1ull << 50);
  CHECK(pl.n_launch == 23 && pl.spp_l == 43479 && pl.n_items == 3ull << 30 && pl.chunk == 14493);
  CHECK(work_items(1u << 30, pl.spp_l, pl.chunk - 1) > item_limit);
  // explicit chunks are raised to the limit as well
  pl = persistent(1u << 30, 1000000, 1ull << 50, 1);
  CHECK(pl.n_items == 3ull << 30 && pl.chunk == 14493);
  // nblocks = min(CUs x blocks per CU, ceil(items / 64)); blocks per CU clamped to RPT_PATHS_WAVES_PER_CU_MAX
  pl = persistent(P1080, 512);
  CHECK(pl.n_items == 32ull * P1080 && pl.per_cu == 2 && pl.nblocks == 512);
  pl = persistent(100, 1);
  CHECK(pl.n_items == 100 && pl.nblocks == 2);
  pl = persistent(64, 1);
  CHECK(pl.n_items == 64 && pl.nblocks == 1);
  pl = plan_persistent(P1080, 512, 8, 256, 40, 32 * GiB, 0, -1, 0, false, false, false);
  CHECK(pl.per_cu == 32 && pl.nblocks == 8192);
  pl = plan_persistent(100000, 1, 8, 256, 40, 32 * GiB, 0, -1, 0, false, false, false);
  CHECK(pl.per_cu == 32 && pl.nblocks == 1563);
}

// a wavefront pass of a scene with one light and deep trees, nothing held, no failures, free memory unknown
static PassInput pass_input(uint32_t npix, uint32_t iterations, uint32_t remaining, double rec_ratio, uint32_t max_bounces,
                            uint64_t target_paths) {
  PassInput in{};
  in.npix = npix; in.iterations = iterations; in.remaining = remaining;
  in.rec_ratio = rec_ratio; in.ratio = pass_ratio(rec_ratio, max_bounces);
  in.per_slot = wavefront_slot_bytes(1, true, true, false);
  in.target_paths = target_paths; in.budget_bytes = 240 * GiB; in.free_bytes = -1; in.free_percent = RPT_WS_FREE_PERCENT;
  return in;
}

static void ratio() {
  CHECK(pass_ratio(0.0, 16) == 17.0 && pass_ratio(0.0, 0) == 1.0);
  CHECK(pass_ratio(1.96, 16) == 2.25); // (1.96 x 1.1 + 0.05) = 2.206, up to a twentieth
  CHECK(pass_ratio(2.5, 8) == 2.8);
  CHECK(pass_ratio(0.01, 8) == 0.1);
  CHECK(pass_ratio(10.0, 8) == 9.0 && pass_ratio(8.2, 8) == 9.0); // at most max_bounces + 1
  // unmeasured, more than one sample left: the measuring pass of one sample per pixel, with room for every level
  PassPlan pp = plan_pass(pass_input(P1080, 64, 64, 0.0, 16, 0));
  CHECK(pp.s_chunk == 1 && pp.s_alloc == 1);
  pp = plan_pass(pass_input(P1080, 1, 1, 0.0, 16, 0));
  CHECK(pp.s_chunk == 1 && pp.s_alloc == 1);
  pp = plan_pass(pass_input(P1080, 64, 64, 2.0, 16, 0)); // measured: the budget decides
  CHECK(pp.s_chunk == 64 && pp.s_alloc == 64);
  CHECK(pp.target == (uint64_t)((double)(240 * GiB) / (332.0 + 2.25 * 68.0)) && pp.target == 531336160);
}

static void passes() {
  // 256 spp with room for 123 per pass: three passes of 86 / 85 / 85
  const uint32_t npix = 1000;
  uint32_t done = 0, sizes[4] = {0, 0, 0, 0}, n = 0;
  while (done < 256 && n < 4) {
    const PassPlan pp = plan_pass(pass_input(npix, 256, 256 - done, 2.0, 16, 123ull * npix));
    CHECK(pp.target == 123ull * npix && pp.s_alloc == 123);
    sizes[n++] = pp.s_chunk;
    done += pp.s_chunk;
  }
  CHECK(n == 3 && sizes[0] == 86 && sizes[1] == 85 && sizes[2] == 85 && done == 256);
  // the workspace is made for the pass a call of this size runs once measured: the call after the measuring pass
  PassPlan pp = plan_pass(pass_input(npix, 16, 15, 2.0, 16, 0));
  CHECK(pp.s_chunk == 15 && pp.s_alloc == 16);
  // a size that did not fit before: at most half of it
  PassInput in = pass_input(npix, 256, 256, 2.0, 16, 100000);
  in.fail_paths = 50000;
  pp = plan_pass(in);
  CHECK(pp.target == 25000 && pp.s_chunk == 24 && pp.s_alloc == 25);
  // from the budget: clamped to [2^20, RPT_MAX_PATHS_PER_PASS] paths
  in = pass_input(npix, 256, 256, 2.0, 16, 0);
  in.budget_bytes = 1000;
  CHECK(plan_pass(in).target == 1ull << 20);
  in.budget_bytes = 1ull << 60;
  CHECK(plan_pass(in).target == RPT_MAX_PATHS_PER_PASS && RPT_MAX_PATHS_PER_PASS == 512ull << 20);
  // ... and with the free memory known: 85 % of (free + what the handle holds)
  in.budget_bytes = 240 * GiB;
  in.free_bytes = 100 * GiB;
  in.held_slots = 1000000; in.held_cols = 2000000;
  const uint64_t budget = (100 * GiB + 1000000ull * 332 + 2000000ull * 68) / 100 * 85;
  CHECK(plan_pass(in).target == (uint64_t)((double)budget / (332.0 + 2.25 * 68.0)) && plan_pass(in).target == 189001762);
  in.free_percent = 50;
  CHECK(plan_pass(in).target == 111177507);
  // an explicit target bypasses the budget and its clamp (not the failures)
  in = pass_input(npix, 256, 256, 2.0, 16, 5);
  in.budget_bytes = 1ull << 60;
  pp = plan_pass(in);
  CHECK(pp.target == 5 && pp.s_chunk == 1 && pp.s_alloc == 1);
  in.target_paths = 1ull << 40;
  in.fail_paths = 4000;
  CHECK(plan_pass(in).target == 2000);
}

static void retries() {
  // out of memory: first the room ahead goes, then the pass halves, down to one sample per pixel
  PassPlan pp{0, 12, 40};
  const uint32_t seq[5][2] = {{12, 12}, {6, 6}, {3, 3}, {1, 1}, {1, 1}};
  for (const auto& s : seq) {
    pp = shrink_after_oom(pp);
    CHECK(pp.s_chunk == s[0] && pp.s_alloc == s[1]);
  }
  CHECK(pass_slots(1000, PassPlan{0, 12, 40}) == 40000 && pass_slots(1000, PassPlan{0, 12, 12}) == 12000);
  CHECK(fail_paths_after_oom(0, 40000) == 40000 && fail_paths_after_oom(30000, 40000) == 30000 &&
        fail_paths_after_oom(50000, 40000) == 40000);
  // record columns: np x ratio rounded up, at least np, at most 0xfffffff0
  CHECK(pass_rec_cols(1000, 2.25) == 2250);
  CHECK(pass_rec_cols(1000, 0.5) == 1000);
  CHECK(pass_rec_cols(3, 1.1) == 4);
  CHECK(pass_rec_cols(1ull << 31, 17.0) == 0xfffffff0ull);
  CHECK(pass_rec_cols(1ull << 33, 1.0) == 1ull << 33);
  // the measured ratio: the largest average seen; after a pool that ran out, 1.5 x what it saw, at most max_bounces + 1
  CHECK(ratio_after_pass(1.5, 196, 100) == 1.96 && ratio_after_pass(2.0, 196, 100) == 2.0);
  CHECK(ratio_after_restart(0.01, 300, 100, 8) == 4.5);
  CHECK(ratio_after_restart(4.0, 300, 100, 8) == 6.0);
  CHECK(ratio_after_restart(0.01, 2000, 100, 8) == 9.0);
}

static void bytes() {
  CHECK(WAVEFRONT_REC_BYTES == 68);
  // (lights, deep trees, ray sort, path re-order) -> bytes of a path slot
  CHECK(wavefront_slot_bytes(1, false, false, false) == 228 && wavefront_slot_bytes(0, false, false, false) == 228);
  CHECK(wavefront_slot_bytes(1, true, false, false) == 304 && wavefront_slot_bytes(1, true, true, false) == 332);
  CHECK(wavefront_slot_bytes(1, false, true, false) == 228 && wavefront_slot_bytes(1, false, false, true) == 264);
  CHECK(wavefront_slot_bytes(1, true, true, true) == 368);
  CHECK(wavefront_slot_bytes(3, false, false, false) == 364 && wavefront_slot_bytes(3, true, false, false) == 440);
  CHECK(wavefront_slot_bytes(3, true, true, false) == 468 && wavefront_slot_bytes(3, false, false, true) == 400);
}

int main(int argc, char** argv) {
  static const struct { const char* name; void (*run)(); } sections[] = {
      {"launches", launches}, {"chunk", chunk}, {"items", items}, {"ratio", ratio},
      {"passes", passes},     {"retries", retries}, {"bytes", bytes}};
  for (const auto& s : sections)
    if (argc < 2 || std::strcmp(argv[1], s.name) == 0) s.run();
  if (!checks) {
    std::printf("FAIL no such section\n");
    return 1;
  }
  if (!failures) std::printf("ok %d\n", checks);
  return failures ? 1 : 0;
}
