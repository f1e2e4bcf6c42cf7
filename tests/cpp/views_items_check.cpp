// Host-side check of the work items of rpt_paths_views (rpt_amd/csrc/render_plan.h views_items, views_item, views_index): a
// launch over a piece of m indices covers every (index, sample) exactly once, every index maps to its (view, pixel), and
// the items plus the room for dead claims never exceed the kernel's 32-bit work counter — the piece is capped so.
// Usage: views_items_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
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
      std::printf("FAIL views_items_check.cpp:%d: %s\n", __LINE__, #cond);     \
    }                                                                          \
  } while (0)

static const uint64_t MAX32 = 0xffffffffull;
static const uint32_t BATCH = RPT_PATHS_BATCH_MAX;

// by hand
static void sizes() {
  CHECK(VIEWS_COUNTER_MAX == MAX32);
  CHECK(views_dead_room(2048, 1024) == 2048ull * 1088);
  { // 5 views of 35 pixels, 3 spp in items of 2: two items per index
    const ViewsItems vi = views_items(175, 3, 2, 512, BATCH);
    CHECK(vi.m == 175 && vi.n_items == 350 && !vi.capped);
    CHECK(vi.n_items == work_items(175, 3, 2));
    const ViewsItem a = views_item(0, 175, 3, 2), b = views_item(174, 175, 3, 2), c = views_item(175, 175, 3, 2), d = views_item(349, 175, 3, 2);
    CHECK(a.index == 0 && a.s_first == 0 && a.s_end == 2);
    CHECK(b.index == 174 && b.s_first == 0 && b.s_end == 2);
    CHECK(c.index == 0 && c.s_first == 2 && c.s_end == 3); // the last item of an index is short
    CHECK(d.index == 174 && d.s_first == 2 && d.s_end == 3);
  }
  { // a chunk larger than spp: one item per index with all its samples; chunk 0 counts as 1
    const ViewsItems vi = views_items(777, 3, 16, 8, BATCH);
    CHECK(vi.m == 777 && vi.n_items == 777);
    const ViewsItem a = views_item(776, 777, 3, 16);
    CHECK(a.index == 776 && a.s_first == 0 && a.s_end == 3);
    CHECK(views_items(777, 3, 0, 8, BATCH).n_items == 3 * 777);
  }
  { // the piece that starts at index 100 of views of 35 pixels: index 0 is pixel 30 of view 2, index 5 pixel 0 of view 3
    const ViewsIndex a = views_index(100, 0, 35), b = views_index(100, 4, 35), c = views_index(100, 5, 35);
    CHECK(a.view == 2 && a.pixel == 30 && a.view_local == 0);
    CHECK(b.view == 2 && b.pixel == 34 && b.view_local == 0);
    CHECK(c.view == 3 && c.pixel == 0 && c.view_local == 1);
    const ViewsIndex d = views_index(0, 7, 1); // views of one pixel
    CHECK(d.view == 7 && d.pixel == 0 && d.view_local == 7);
    const ViewsIndex e = views_index((1ull << 57) + 3, MAX32 - 1, 1ull << 32); // far out: the arithmetic is 64 bits wide
    CHECK(e.view == (1ull << 25) + 1 && e.pixel == 1 && e.view_local == 1);
  }
  // a piece too long for the counter is capped, and one index of more samples than the counter holds does not fit at all
  const ViewsItems big = views_items(1ull << 31, 4, 1, 8192, BATCH);
  CHECK(big.capped && big.m == (MAX32 - 8192ull * 1088) / 4 && big.n_items == 4 * big.m);
  CHECK(views_items(10, 0xffffffffu, 1, 8192, BATCH).m == 0);
  CHECK(views_items(10, 0xffffffffu, 1u << 12, 8192, BATCH).m == 10);
}

// every (index, sample) exactly once, every index at its (view, pixel)
static void cover() {
  const uint64_t npixs[] = {1, 35, 777};
  const uint64_t n_views[] = {1, 5, 64};
  const uint32_t chunks[] = {1, 2, 7, 100};
  const uint32_t spps[] = {1, 3, 4, 16};
  const uint64_t asks[] = {0, 1, 100, 128}; // 0: the whole call in one piece; the others end pieces inside views
  for (uint64_t npix : npixs)
    for (uint64_t nv : n_views)
      for (uint64_t ask : asks) {
        const uint64_t n = nv * npix, piece = ask ? ask : n;
        uint64_t seen_j = 0;
        for (uint64_t base = 0; base < n; base += piece) {
          const uint64_t m = views_piece_len(base, n, npix, piece, false);
          for (uint64_t i = 0; i < m; i++) { // the index -> (view, pixel) map
            const ViewsIndex ix = views_index(base, i, npix);
            bool ok = ix.view * npix + ix.pixel == base + i && ix.pixel < npix && ix.view < nv &&
                      ix.view_local == ix.view - base / npix;
            if (!ok) { CHECK(ok); return; }
            seen_j++;
          }
          for (uint32_t spp : spps)
            for (uint32_t chunk : chunks) {
              const ViewsItems vi = views_items(m, spp, chunk, 2048, BATCH);
              CHECK(vi.m == m && !vi.capped && vi.n_items == work_items((uint32_t)m, spp, chunk));
              CHECK(vi.n_items + views_dead_room(2048, BATCH) <= MAX32);
              std::vector<uint8_t> hit(m * spp, 0);
              bool ok = true;
              for (uint64_t it = 0; it < vi.n_items && ok; it++) {
                const ViewsItem w = views_item(it, m, spp, chunk);
                ok = w.index < m && w.s_first < w.s_end && w.s_end <= spp && w.s_end - w.s_first <= chunk;
                for (uint32_t s = w.s_first; ok && s < w.s_end; s++) ok = hit[w.index * spp + s]++ == 0;
              }
              for (uint64_t k = 0; k < m * spp && ok; k++) ok = hit[k] == 1;
              CHECK(ok);
            }
        }
        CHECK(seen_j == n);
      }
}

// at the counter's edge: whatever is asked, the items and the dead claims' room fit 32 bits, and one index more would not
static void edge() {
  const uint32_t blocks[] = {1, 256, 2048, 8192, 1u << 20};
  const uint32_t spps[] = {1, 3, 4, 1000, 1u << 20, 0xffffffffu};
  const uint32_t chunks[] = {1, 2, 16, 1u << 16};
  const uint64_t ms[] = {1, 1000, 4ull << 20, MAX32 - 1, MAX32, 1ull << 40};
  for (uint32_t nb : blocks)
    for (uint32_t spp : spps)
      for (uint32_t chunk : chunks)
        for (uint64_t m : ms) {
          const ViewsItems vi = views_items(m, spp, chunk, nb, BATCH);
          const uint64_t room = views_dead_room(nb, BATCH), per = ((uint64_t)spp + chunk - 1) / chunk;
          CHECK(vi.m <= m && vi.m <= MAX32 && vi.capped == (vi.m < m) && vi.n_items == vi.m * per);
          CHECK(vi.n_items + room <= MAX32);
          if (vi.capped && vi.m < MAX32) CHECK((vi.m + 1) * per + room > MAX32); // the cap is tight
          if (vi.m) { // the last item is the last sample run of the last index
            const ViewsItem w = views_item(vi.n_items - 1, vi.m, spp, chunk);
            CHECK(w.index == vi.m - 1 && w.s_end == spp && w.s_first == (per - 1) * chunk);
          }
        }
  // exactly at the edge: the counter's last value is used, one more item is refused
  const uint64_t room = views_dead_room(2048, BATCH);
  CHECK(views_items(MAX32 - room, 1, 1, 2048, BATCH).m == MAX32 - room && !views_items(MAX32 - room, 1, 1, 2048, BATCH).capped);
  CHECK(views_items(MAX32 - room + 1, 1, 1, 2048, BATCH).capped);
  // what the host asks with (api_internal.h persistent_piece): the call's samples in items of one, every block a device may hold
  const ViewsItems host = views_items(RAYS_PIECE_MAX, 4, 1, 256 * RPT_PATHS_WAVES_PER_CU_MAX, BATCH);
  CHECK(!host.capped && host.n_items == 4 * RAYS_PIECE_MAX);
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else if (!std::strcmp(s, "edge")) edge();
  else { std::printf("FAIL unknown section '%s'\n", s); return 1; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
