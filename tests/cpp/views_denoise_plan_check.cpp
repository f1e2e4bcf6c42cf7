// Host-side check of the working-set arithmetic of rptgpu_render_views_denoised (rpt_amd/csrc/render_plan.h
// views_denoise_plan, sample_range_fits): the batch's index count fits the 32-bit accumulation or the plan says so without
// overflowing on the way, the byte counts are the arrays the driver allocates, and a sample range is refused exactly when
// its last index needs a 65th bit.
// Usage: views_denoise_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>

#include "../../rpt_amd/csrc/render_plan.h"

using namespace rptplan;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    checks++;                                                                        \
    if (!(cond)) {                                                                   \
      failures++;                                                                    \
      std::printf("FAIL views_denoise_plan_check.cpp:%d: %s\n", __LINE__, #cond);    \
    }                                                                                \
  } while (0)

static const uint64_t MAX = 0xffffffffull;

// the 32-bit bound, at its edges and where the product itself would wrap
static void bound() {
  CHECK(VIEWS_DENOISE_MAX_N == MAX);
  CHECK(views_denoise_plan(0, 777, true, true, true, true, true).n == 0);
  CHECK(views_denoise_plan(3, 777, true, true, true, true, true).n == 2331);
  CHECK(views_denoise_plan(MAX, 1, false, true, false, false, false).n == MAX);
  CHECK(views_denoise_plan(MAX + 1, 1, false, true, false, false, false).n == 0);
  CHECK(views_denoise_plan(1, MAX, false, true, false, false, false).n == MAX);
  CHECK(views_denoise_plan(1, MAX + 1, false, true, false, false, false).n == 0); // (width * height may be 2^32)
  CHECK(views_denoise_plan(65535, 65537, false, true, false, false, false).n == MAX); // 2^32 - 1 = 65535 * 65537
  CHECK(views_denoise_plan(65536, 65536, false, true, false, false, false).n == 0);
  CHECK(views_denoise_plan(33140, 129600, false, true, false, false, false).n == 33140ull * 129600); // 480 x 270: 4 294 944 000
  CHECK(views_denoise_plan(33141, 129600, false, true, false, false, false).n == 0);
  // products that wrap 64 bits to something small are still refused
  CHECK(views_denoise_plan(1ull << 58, 1ull << 6, false, true, false, false, false).n == 0);   // 2^64 -> 0
  CHECK(views_denoise_plan((1ull << 58) + 1, 1ull << 6, false, true, false, false, false).n == 0); // -> 64
  CHECK(views_denoise_plan(~0ull, ~0ull, false, true, false, false, false).n == 0);            // -> 1
  CHECK(views_denoise_plan(~0ull, 2, false, true, false, false, false).n == 0);
  for (uint64_t npix : {(uint64_t)1, (uint64_t)2, (uint64_t)777, (uint64_t)129600, MAX, MAX + 1})
    for (uint64_t nv : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)64, (uint64_t)65535, (uint64_t)65536, MAX / npix, MAX / npix + 1,
                        (uint64_t)1 << 40, ~(uint64_t)0 / npix, ~(uint64_t)0 / npix + 1, ~(uint64_t)0}) {
      if (!nv) continue;
      const bool fits = nv <= MAX / npix; // (exact: floor division)
      const ViewsDenoisePlan p = views_denoise_plan(nv, npix, true, true, true, true, true);
      CHECK((p.n != 0) == fits);
      CHECK(!fits || (p.n == nv * npix && p.n <= MAX));
      CHECK(fits || p.bytes() == 0);
    }
}

// the bytes: what api_views_denoise.cpp allocates, and DESIGN.md §18's figure
static void bytes() {
  const uint64_t n = 16ull * 129600; // 16 views of 480 x 270
  const ViewsDenoisePlan d = views_denoise_plan(16, 129600, false, true, true, true, true);
  CHECK(d.state == n * 60 && d.staging == n * 24 && d.columns == n * 145 && d.outputs == 0);
  CHECK(d.features >= n * 84 && d.features <= n * 84 + 64); // hits 4, depth 8, normal, albedo, position 24 each; 16-byte rounding
  CHECK(d.bytes() >= n * 313 && d.bytes() <= n * 313 + 64);
  const ViewsDenoisePlan h = views_denoise_plan(16, 129600, true, true, true, true, true);
  CHECK(h.outputs == n * 59 && h.bytes() == d.bytes() + n * 59);
  CHECK(views_denoise_plan(16, 129600, true, true, false, false, false).outputs == n * 24);
  CHECK(views_denoise_plan(16, 129600, true, false, true, false, false).outputs == n * 3);
  CHECK(views_denoise_plan(16, 129600, true, false, true, true, false).outputs == n * 27);
  CHECK(views_denoise_plan(16, 129600, true, false, true, false, true).outputs == n * 11);
  // odd counts: the feature arrays keep aov_arrays' rounding (every array 16-byte aligned)
  for (uint64_t k = 1; k <= 9; k++) {
    const ViewsDenoisePlan p = views_denoise_plan(1, k, false, true, false, false, false);
    const uint64_t want = ((k + 1) / 2 * 2 + 3 * ((3 * k + 1) / 2 * 2) + (k + 3) / 4 * 2) * 8;
    CHECK(p.features == want && p.features % 16 == 0 && p.features >= k * 84);
  }
  // the largest batch: no byte count wraps
  const ViewsDenoisePlan m = views_denoise_plan(MAX, 1, true, true, true, true, true);
  CHECK(m.n == MAX && m.bytes() > MAX * 372 && m.bytes() < MAX * 373);
}

// a sample range base .. base + count - 1
static void ranges() {
  CHECK(sample_range_fits(0, 1) && sample_range_fits(5, 6) && sample_range_fits(0, ~0ull));
  CHECK(sample_range_fits(~0ull, 1));          // the last index itself
  CHECK(!sample_range_fits(~0ull, 2));
  CHECK(sample_range_fits(1, ~0ull) && !sample_range_fits(2, ~0ull));
  CHECK(sample_range_fits(~0ull - 11, 12) && !sample_range_fits(~0ull - 11, 13));
  const uint64_t most = 0xffffffffull * 0xffffffffull; // batches * iterations at their largest
  CHECK(sample_range_fits(0, most) && sample_range_fits(~0ull - most + 1, most) && !sample_range_fits(~0ull - most + 2, most));
  CHECK(sample_range_fits(1ull << 63, 1ull << 63) && !sample_range_fits((1ull << 63) + 1, 1ull << 63));
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "bound")) bound();
  else if (!std::strcmp(s, "bytes")) bytes();
  else if (!std::strcmp(s, "ranges")) ranges();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
