// Host-side check of the piece arithmetic of rptgpu_render_views (rpt_amd/csrc/render_plan.h views_piece, views_piece_len):
// the pieces cover the call's (view, pixel) indices once and in order, stay within a view when the views' seeds differ, and
// never hold more than a pass may.
// Usage: views_piece_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rpt_amd/csrc/render_plan.h"

using namespace rptplan;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    checks++;                                                                  \
    if (!(cond)) {                                                             \
      failures++;                                                              \
      std::printf("FAIL views_piece_check.cpp:%d: %s\n", __LINE__, #cond);     \
    }                                                                          \
  } while (0)

static const uint64_t Mi = 1ull << 20, GiB = 1ull << 30;

struct Piece { uint64_t base, len; };
static std::vector<Piece> pieces(uint64_t n_views, uint64_t npix, uint64_t asked, uint64_t pass_target, bool at_views) {
  const uint64_t n = n_views * npix, piece = views_piece(n, asked, pass_target);
  std::vector<Piece> out;
  for (uint64_t base = 0, m; base < n; base += m) {
    m = views_piece_len(base, n, npix, piece, at_views);
    out.push_back({base, m});
    if (!m) break; // (no progress: reported by the caller's checks)
  }
  return out;
}

// by hand
static void sizes() {
  CHECK(views_piece(3 * 777, 0, 128 * Mi) == 3 * 777);   // a small call is one piece
  CHECK(views_piece(3 * 777, 100, 128 * Mi) == 100);     // the tests' hook
  CHECK(views_piece(64ull * 129600, 0, 128 * Mi) == RAYS_PIECE_MAX);
  CHECK(views_piece(1ull << 40, 1ull << 40, ~0ull) == RPT_MAX_PATHS_PER_PASS);
  // three views of 777 pixels in pieces of 100: the piece that starts at 700 ...
  CHECK(views_piece_len(700, 2331, 777, 100, false) == 100); // ... spans views 0 and 1,
  CHECK(views_piece_len(700, 2331, 777, 100, true) == 77);   // ... or ends with view 0
  CHECK(views_piece_len(777, 2331, 777, 100, true) == 100);
  CHECK(views_piece_len(2300, 2331, 777, 100, false) == 31 && views_piece_len(2300, 2331, 777, 100, true) == 31);
  CHECK(views_piece_len(0, 2331, 777, 2331, false) == 2331 && views_piece_len(0, 2331, 777, 2331, true) == 777);
  CHECK(views_piece_len(0, 5, 1, 100, true) == 1); // views of one pixel
  const std::vector<Piece> a = pieces(3, 777, 100, 128 * Mi, false), b = pieces(3, 777, 100, 128 * Mi, true);
  CHECK(a.size() == 24 && b.size() == 24); // ceil(2331 / 100); 3 * ceil(777 / 100)
  CHECK(a[7].base == 700 && a[7].len == 100 && b[7].base == 700 && b[7].len == 77 && b[8].base == 777);
}

// consecutive, none empty, together the n indices; within a view when asked; never more than the piece or the pass
static void cover() {
  const uint64_t views[] = {1, 2, 3, 16, 64, 1000};
  const uint64_t npixs[] = {1, 2, 99, 100, 101, 777, 759, 129600, 2 * Mi + 3};
  const uint64_t asks[] = {0, 1, 7, 100, 128, 5 * Mi};
  const uint64_t targets[] = {1 * Mi, 3 * Mi + 17, 128 * Mi};
  for (uint64_t nv : views)
    for (uint64_t npix : npixs)
      for (uint64_t asked : asks)
        for (uint64_t target : targets)
          for (int at_views = 0; at_views < 2; at_views++) {
            const uint64_t n = nv * npix;
            if (asked && n / asked > 100000) continue; // (a loop of millions shows nothing more)
            const uint64_t piece = views_piece(n, asked, target);
            const std::vector<Piece> ps = pieces(nv, npix, asked, target, at_views != 0);
            uint64_t next = 0;
            bool ok = true, in_view = true, fits = true;
            for (const Piece& p : ps) {
              ok = ok && p.base == next && p.len >= 1;
              fits = fits && p.len <= piece && p.len <= target && p.len <= RPT_MAX_PATHS_PER_PASS;
              in_view = in_view && p.base / npix == (p.base + p.len - 1) / npix;
              next = p.base + p.len;
            }
            CHECK(ok && next == n);
            CHECK(fits);
            CHECK(!at_views || in_view);
            // a piece is cut short only by the end of the call or, when asked, of a view
            for (const Piece& p : ps)
              if (p.len < piece && p.base + p.len != n) CHECK(at_views && (p.base + p.len) % npix == 0);
          }
}

// what the planner does with a piece as its frame: every pass's paths fit the target and 32 bits (rays_piece_check's
// `passes`, over the pieces of views)
static void passes() {
  const uint64_t targets[] = {0, 1 * Mi, 128 * Mi, RPT_MAX_PATHS_PER_PASS};
  const uint32_t spps[] = {1, 4, 64, 100000};
  for (uint64_t target_paths : targets)
    for (uint64_t nv : {(uint64_t)1, (uint64_t)6, (uint64_t)64, (uint64_t)4096})
      for (uint64_t npix : {(uint64_t)777, (uint64_t)129600, 8 * Mi})
        for (int at_views = 0; at_views < 2; at_views++) {
          PassInput in{};
          in.npix = 1; in.iterations = 1; in.remaining = 1;
          in.ratio = 9.0; // max_bounces + 1: room for every level of every path
          in.per_slot = wavefront_slot_bytes(2, true, true, false);
          in.target_paths = target_paths; in.budget_bytes = 240 * GiB; in.free_bytes = target_paths ? -1 : (int64_t)(200 * GiB);
          in.free_percent = 85;
          const uint64_t pass_target = plan_pass(in).target;
          uint64_t longest = 0;
          for (const Piece& p : pieces(nv, npix, 0, pass_target, at_views != 0)) longest = std::max(longest, p.len);
          CHECK(longest >= 1 && longest <= pass_target && longest <= RPT_MAX_PATHS_PER_PASS);
          for (uint32_t spp : spps)
            for (double rec_ratio : {0.0, 1.3, 9.0}) {
              PassInput pi = in;
              pi.npix = (uint32_t)longest; pi.iterations = spp; pi.remaining = spp;
              pi.rec_ratio = rec_ratio; pi.ratio = pass_ratio(rec_ratio, 8);
              const PassPlan pp = plan_pass(pi);
              const uint64_t paths = longest * (uint64_t)pp.s_chunk;
              CHECK(pp.s_chunk >= 1 && pp.s_chunk <= spp);
              CHECK(paths <= std::max<uint64_t>(longest, pp.target));
              CHECK(paths <= 0xffffffffull && pass_slots((uint32_t)longest, pp) <= 0xffffffffull);
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
