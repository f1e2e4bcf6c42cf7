// Host-side check of the piece arithmetic of rptgpu_trace_vertices (rpt_amd/csrc/render_plan.h vertices_piece): the pieces cover
// the rays once and in order, none is empty, a host caller's staging stays under its cap for every channel subset, and the
// bytes counted per vertex are those of the arrays include/rpt_gpu_vertices.h declares.
// Usage: vertices_piece_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
#include <cstdio>
#include <cstring>

#include "../../include/rpt_gpu.h"
#include "../../rpt_amd/csrc/render_plan.h"

using namespace rptplan;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    checks++;                                                                  \
    if (!(cond)) {                                                             \
      failures++;                                                              \
      std::printf("FAIL vertices_piece_check.cpp:%d: %s\n", __LINE__, #cond);  \
    }                                                                          \
  } while (0)

static const uint64_t Mi = 1ull << 20, Gi = 1ull << 30;
static const uint32_t ALL = (1u << VERTICES_CHANNEL_BITS) - 1u;

// the header's element types, channel by channel
static uint64_t header_vertex_bytes(uint32_t ch) {
  RptVertexArrays a;
  uint64_t b = 0;
  if (ch & RPT_VERTEX_T) b += sizeof *a.t;
  if (ch & RPT_VERTEX_NORMAL) b += 3 * sizeof *a.normal;
  if (ch & RPT_VERTEX_OBJECT) b += sizeof *a.object;
  if (ch & RPT_VERTEX_POSITION) b += 3 * sizeof *a.position;
  if (ch & RPT_VERTEX_DIRECTION) b += 3 * sizeof *a.direction;
  if (ch & RPT_VERTEX_DRAW) b += sizeof *a.draw;
  if (ch & RPT_VERTEX_RADIANCE) b += 3 * sizeof *a.radiance;
  if (ch & RPT_VERTEX_BSDF) b += 3 * sizeof *a.bsdf;
  if (ch & RPT_VERTEX_INV_PDF) b += sizeof *a.inv_pdf;
  if (ch & RPT_VERTEX_ABS_COS) b += sizeof *a.abs_cos;
  return b;
}

static void sizes() {
  CHECK(ALL == 4095u && (RPT_VERTEX_RGB << 1) == (1u << VERTICES_CHANNEL_BITS));
  CHECK(VERTICES_STAGING_MAX == 1 * Gi);
  for (uint32_t ch = 0; ch <= ALL; ch++) {
    CHECK(vertices_vertex_bytes(ch) == header_vertex_bytes(ch));
    CHECK(vertices_path_bytes(ch) == ((ch & RPT_VERTEX_LENGTH) ? sizeof(uint32_t) : 0u));
  }
  CHECK(vertices_vertex_bytes(ALL) == 152 && vertices_vertex_bytes(RPT_VERTEX_LENGTH | RPT_VERTEX_RGB) == 0);
  // a device caller: rays_piece as it stands
  CHECK(vertices_piece(1000, 0, 128 * Mi, false, 4, 8, ALL) == 1000);
  CHECK(vertices_piece(64 * Mi, 0, 128 * Mi, false, 1000, 254, ALL) == RAYS_PIECE_MAX);
  CHECK(vertices_piece(1000, 100, 128 * Mi, false, 4, 8, ALL) == 100);
  CHECK(vertices_piece(64 * Mi, 0, 1 * Mi, false, 4, 8, ALL) == 1 * Mi);
  // a host caller: 4 samples x 9 vertices x 152 B + 4 x 4 B = 5488 B per ray
  CHECK(vertices_staging_bytes(1, 4, 8, ALL) == 5488);
  CHECK(vertices_piece(64 * Mi, 0, 128 * Mi, true, 4, 8, ALL) == Gi / 5488);
  CHECK(vertices_piece(1000, 0, 128 * Mi, true, 4, 8, ALL) == 1000);
  CHECK(vertices_piece(64 * Mi, 0, 128 * Mi, true, 4, 8, RPT_VERTEX_RGB) == RAYS_PIECE_MAX); // nothing per vertex to stage
  CHECK(vertices_piece(64 * Mi, 0, 128 * Mi, true, 4, 8, RPT_VERTEX_LENGTH) == RAYS_PIECE_MAX);
  CHECK(vertices_piece(64 * Mi, 0, 128 * Mi, true, 1u << 20, 254, ALL) == 1);              // one ray beyond the cap: still a piece
  CHECK(vertices_piece(64 * Mi, 0, 0, true, 4, 8, ALL) == 1);
  CHECK(vertices_staging_bytes(~0ull, 0xffffffffu, 254, ALL) == ~0ull);                     // saturates
  // the size refusal: n * iterations * (B + 1) < 2^56
  CHECK(vertices_fit(0, 0xffffffffu, 254) && vertices_fit(1, 0xffffffffu, 254));
  CHECK(vertices_fit((1ull << 56) - 1, 1, 0) && !vertices_fit(1ull << 56, 1, 0));
  CHECK(vertices_fit((1ull << 48) - 1, 16, 15) && !vertices_fit(1ull << 48, 16, 15));
  CHECK(!vertices_fit(~0ull, 0xffffffffu, 254));
}

// the driver's loop: consecutive pieces, none empty, none longer than `piece`, together the n rays in order
static void cover() {
  const uint64_t ns[] = {1, 2, 99, 100, 101, 257, 777, 4 * Mi - 1, 4 * Mi + 1, 9 * Mi + 5};
  const uint64_t asks[] = {0, 1, 7, 100, 5 * Mi};
  const uint32_t chans[] = {ALL, RPT_VERTEX_LENGTH | RPT_VERTEX_RGB, RPT_VERTEX_POSITION, RPT_VERTEX_OBJECT | RPT_VERTEX_DRAW};
  for (uint64_t n : ns)
    for (uint64_t asked : asks)
      for (uint32_t ch : chans)
        for (int host = 0; host < 2; host++) {
          if (asked == 1 && n > 1000) continue; // (a loop of millions shows nothing more)
          const uint64_t piece = vertices_piece(n, asked, 128 * Mi, host != 0, 3, 8, ch);
          CHECK(piece >= 1 && piece <= n);
          uint64_t next = 0, count = 0;
          bool ordered = true, none_empty = true;
          for (uint64_t base = 0; base < n; base += piece) {
            const uint64_t m = std::min(piece, n - base);
            ordered = ordered && base == next;
            none_empty = none_empty && m >= 1 && m <= piece;
            next = base + m;
            count++;
          }
          CHECK(ordered && none_empty && next == n && count == rays_piece_count(n, piece));
        }
}

// every channel subset, for several shapes of a call: a host caller's piece is staged within the cap (or is one ray), and is
// the largest such piece rays_piece allows; a device caller's is rays_piece's
static void staging() {
  const struct { uint32_t iterations, max_bounces; } shapes[] = {{1, 0}, {3, 8}, {4, 8}, {64, 16}, {1000, 254}, {1u << 20, 254}};
  const uint64_t n = 700 * Mi, target = 128 * Mi;
  for (const auto& s : shapes)
    for (uint32_t ch = 1; ch <= ALL; ch++) {
      const uint64_t base_piece = rays_piece(n, 0, target);
      CHECK(vertices_piece(n, 0, target, false, s.iterations, s.max_bounces, ch) == base_piece);
      const uint64_t piece = vertices_piece(n, 0, target, true, s.iterations, s.max_bounces, ch);
      const uint64_t bytes = vertices_staging_bytes(piece, s.iterations, s.max_bounces, ch);
      CHECK(piece >= 1 && piece <= base_piece);
      CHECK(bytes <= VERTICES_STAGING_MAX || piece == 1);
      if (piece < base_piece) CHECK(vertices_staging_bytes(piece + 1, s.iterations, s.max_bounces, ch) > VERTICES_STAGING_MAX);
      // a wish (the tests' hook) is held to the same cap
      const uint64_t wished = vertices_piece(n, 600 * Mi, target, true, s.iterations, s.max_bounces, ch);
      CHECK(vertices_staging_bytes(wished, s.iterations, s.max_bounces, ch) <= VERTICES_STAGING_MAX || wished == 1);
    }
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "sizes")) sizes();
  else if (!std::strcmp(s, "cover")) cover();
  else if (!std::strcmp(s, "staging")) staging();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
