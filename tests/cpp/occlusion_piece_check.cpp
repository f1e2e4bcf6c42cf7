// Host-side check of the piece arithmetic of rptgpu_occluded and rptgpu_bake_ao (rpt_amd/csrc/render_plan.h
// occlusion_pass_max, occlusion_piece, ao_piece, ao_pass_samples): the pieces cover [0, n) once and in order, a piece of
// points is whole points, and no pass holds more rays than a pass may — also when one point's samples alone exceed it.
// Usage: occlusion_piece_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
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
      std::printf("FAIL occlusion_piece_check.cpp:%d: %s\n", __LINE__, #cond); \
    }                                                                          \
  } while (0)

static const uint64_t Mi = 1ull << 20, GiB = 1ull << 30;

// by hand
static void sizes() {
  CHECK(occlusion_pass_max(0) == 1 && occlusion_pass_max(5) == 5);
  CHECK(occlusion_pass_max(128 * Mi) == OCCLUSION_PIECE_MAX && occlusion_pass_max(~0ull) == OCCLUSION_PIECE_MAX);
  CHECK(OCCLUSION_PIECE_MAX <= RPT_MAX_PATHS_PER_PASS);
  CHECK(occlusion_piece(0, 0, 128 * Mi) == 1);            // (n == 0 returns before any piece; the loop below runs zero times)
  CHECK(occlusion_piece(1, 0, 128 * Mi) == 1);
  CHECK(occlusion_piece(600, 0, 128 * Mi) == 600);        // a small call is one piece
  CHECK(occlusion_piece(600, 100, 128 * Mi) == 100);      // the tests' hook
  CHECK(occlusion_piece(33ull * Mi, 0, 128 * Mi) == OCCLUSION_PIECE_MAX);
  CHECK(occlusion_piece(33ull * Mi, 0, 3 * Mi) == 3 * Mi); // what the device has room for
  CHECK(occlusion_piece(1ull << 40, 1ull << 40, ~0ull) == OCCLUSION_PIECE_MAX);
  CHECK(ao_piece(0, 0, 16, 128 * Mi) == 1 && ao_piece(1, 0, 16, 128 * Mi) == 1);
  CHECK(ao_piece(16, 0, 33, 128 * Mi) == 16 && ao_piece(16, 5, 33, 128 * Mi) == 5);
  CHECK(ao_piece(2 * Mi + 600, 0, 16, 128 * Mi) == Mi);   // 1080p at S = 16: pieces of 16 Mi rays
  CHECK(ao_piece(1000, 0, 64 * Mi, 128 * Mi) == 1);       // S larger than a pass: one point per piece ...
  CHECK(ao_pass_samples(1, 64 * Mi, 128 * Mi) == 16 * Mi); // ... in passes of what a pass holds
  CHECK(ao_pass_samples(16, 33, 128 * Mi) == 33 && ao_pass_samples(16, 33, 100) == 6 && ao_pass_samples(16, 33, 16) == 1);
  CHECK(ao_pass_samples(5, 3, 100) == 3);                 // never more than remain
}

// rptgpu_occluded's loop: consecutive, none empty, together [0, n), never more than the piece or the pass
static void cover() {
  const uint64_t ns[] = {0, 1, 2, 99, 100, 101, 600, 4 * Mi + 3, 33 * Mi};
  const uint64_t asks[] = {0, 1, 7, 100, 5 * Mi, 64 * Mi};
  const uint64_t targets[] = {1, 1000, 1 * Mi, 3 * Mi + 17, 128 * Mi};
  for (uint64_t n : ns)
    for (uint64_t asked : asks)
      for (uint64_t target : targets) {
        const uint64_t piece = occlusion_piece(n, asked, target);
        CHECK(piece >= 1 && piece <= occlusion_pass_max(target) && piece <= std::max<uint64_t>(1, target));
        CHECK(!asked || piece <= asked);
        if (n / piece > 200000) continue; // (a loop of millions shows nothing more)
        uint64_t next = 0, count = 0;
        bool ok = true;
        for (uint64_t base = 0; base < n; base += piece) {
          const uint64_t m = std::min(piece, n - base);
          ok = ok && base == next && m >= 1 && m <= piece && m <= 0xffffffffull;
          next = base + m;
          count++;
        }
        CHECK(ok && next == n);
        CHECK(count == (n + piece - 1) / piece);
      }
}

// rptgpu_bake_ao's loops: pieces of whole points that cover [0, n); per piece, passes that cover [0, S) in order; every pass
// points x samples within the bound, within the slots the driver asks the workspace for, and within 32 bits
static void ao() {
  const uint64_t ns[] = {0, 1, 2, 16, 17, 1000, 2 * Mi + 600};
  const uint32_t Ss[] = {1, 16, 33, 4096, 100000, 40u * (uint32_t)Mi, 0xffffffffu};
  const uint64_t asks[] = {0, 1, 5, 1000, 64 * Mi};
  const uint64_t targets[] = {1, 100, 1 * Mi, 3 * Mi + 17, 128 * Mi};
  for (uint64_t n : ns)
    for (uint32_t S : Ss)
      for (uint64_t asked : asks)
        for (uint64_t target : targets) {
          const uint64_t fit = occlusion_pass_max(target);
          const uint64_t piece = ao_piece(n, asked, S, target);
          CHECK(piece >= 1 && piece <= fit && (!asked || piece <= asked));
          const uint64_t slots = std::min<uint64_t>(piece * S, fit); // (api_occlusion.cpp bake_ao)
          if (n / piece > 20000) continue;
          uint64_t next = 0;
          bool ok = true, fits = true, samples_ok = true;
          for (uint64_t base = 0; base < n; base += piece) {
            const uint64_t m = std::min(piece, n - base); // whole points: a point is in exactly one piece
            ok = ok && base == next && m >= 1;
            next = base + m;
            if (base && base + piece < n) continue; // (the inner pieces are all alike: the first and the last two show it)
            uint32_t s0 = 0;
            uint64_t passes = 0;
            while (s0 < S) {
              const uint32_t s_pass = ao_pass_samples(m, S - s0, target);
              samples_ok = samples_ok && s_pass >= 1 && s_pass <= S - s0;
              fits = fits && m * s_pass <= fit && m * s_pass <= slots && m * s_pass <= 0xffffffffull;
              if (!s_pass) break;
              s0 += s_pass;
              if (++passes > 1000000) { s0 = S; } // (S = 2^32 - 1 in passes of one sample: the first million show it)
            }
            samples_ok = samples_ok && s0 == S;
          }
          CHECK(ok && next == n);
          CHECK(fits);
          CHECK(samples_ok);
        }
}

// with the planner's own target for a scene: what the driver computes (api_occlusion.cpp Occlusion)
static void planned() {
  for (uint64_t target_paths : {(uint64_t)0, 1 * Mi, 128 * Mi, (uint64_t)RPT_MAX_PATHS_PER_PASS})
    for (int64_t free_gib : {1, 16, 200}) {
      PassInput in{};
      in.npix = 1; in.iterations = 1; in.remaining = 1;
      in.ratio = 1.0;
      in.per_slot = wavefront_slot_bytes(0, true, true, false); // no lights: one column all the same
      in.target_paths = target_paths; in.budget_bytes = 240 * GiB; in.free_bytes = target_paths ? -1 : free_gib * (int64_t)GiB;
      in.free_percent = 85;
      const uint64_t target = plan_pass(in).target;
      CHECK(target >= 1);
      CHECK(occlusion_piece(33 * Mi, 0, target) <= target && occlusion_piece(33 * Mi, 0, target) <= OCCLUSION_PIECE_MAX);
      const uint64_t piece = ao_piece(2 * Mi, 0, 16, target);
      CHECK(piece * ao_pass_samples(piece, 16, target) <= std::min<uint64_t>(target, OCCLUSION_PIECE_MAX));
    }
  CHECK(wavefront_slot_bytes(0, false, false, false) == wavefront_slot_bytes(1, false, false, false));
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else if (!std::strcmp(s, "ao")) ao();
  else if (!std::strcmp(s, "planned")) planned();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
