// lightmap_plan.h — the host-only arithmetic of rptgpu_bake_lightmap (api_lightmap.cpp): the clamp of a
// triangle's texel-space extent to the range of texels rpt_lightmap_owners tests (kernels/lightmap.inc compiles the same
// function for the device), the pieces the map is cut into, the layout of a piece's compacted probe arrays inside one
// allocation, and RptLightmapArrays' channel table (channel_plan.h).  No HIP, no handle: tests/cpp/lightmap_plan_check.cpp builds it alone, with the host sanitizers too.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/rpt_gpu.h"
#include "channel_plan.h"

#ifndef RPT_LIGHTMAP_HD
#define RPT_LIGHTMAP_HD
#endif

namespace rptlightmap {

// ---- the texels [lo, hi) of one axis whose centres i + 0.5 may lie in [a_min, a_max], generously: one texel more on either
// side than floor / ceil give, cut to [0, size).  a_min / a_max: the smallest and largest texel-space coordinate of a
// triangle's vertices — finite for a triangle that covers anything, but ANY doubles are taken: huge, negative, infinite or NaN
// (then empty).  Never lo > hi, never a cast of a value outside [0, size]; empty is {0, 0}.
struct TexelRange {
  uint32_t lo, hi;
};
RPT_LIGHTMAP_HD inline TexelRange clamp_range(double a_min, double a_max, uint32_t size) {
  const double s = (double)size; // exact: size < 2^32
  // (the negated comparisons also catch NaN) wholly below the map, wholly above it, inverted, or no map
  if (!(a_max >= 0.0) || !(a_min <= s) || !(a_min <= a_max) || size == 0) return TexelRange{0u, 0u};
  // here a_min <= s and a_max >= 0.  floor(a_min) - 1 lies in [0, s - 1] when a_min > 1; ceil(a_max) + 1 in [1, s] when
  // a_max < s - 1: both casts are of integers inside uint32_t's range
  const uint32_t lo = a_min > 1.0 ? (uint32_t)(std::floor(a_min) - 1.0) : 0u;
  const uint32_t hi = a_max < s - 1.0 ? (uint32_t)(std::ceil(a_max) + 1.0) : size;
  // lo <= s - 1 < s, and lo <= floor(a_min) - 1 < a_min <= a_max < ceil(a_max) + 1: the range is never empty or inverted here
  return TexelRange{lo, hi};
}

// ---- is the box a superset of what the ROUNDED edge tests cover?  Not for a sliver: the edge functions measure the distance
// to the edges' LINES, and for a triangle whose vertices are collinear up to rounding all three come out with the right sign
// at centres on that line far beyond the vertices.  The bound: with every coordinate and every centre within [-M, M], D = 2M,
// Ex / Ey the extents of the vertices and u = 2^-53, a computed edge function is within eps = 8u D (Ex + Ey) of the exact
// one (three roundings per product term and the subtraction).  A centre that passes the rounded tests has exact e_i >=
// -eps (area > 0; mirrored likewise), so its negative barycentrics are at most eps / |area| each, two at the most; a centre
// the clamp leaves out lies at least half a texel outside the vertices' extent in some axis, which takes negative weights of
// 0.5 / E in sum, E = max(Ex, Ey).  So |area| > 4 eps E = 32u D (Ex + Ey) E rules such a centre out; the computed area is
// within 16u Ex Ey of the exact one.  `sliver` is that test with a factor of four to spare and a floor for products that
// underflow; it errs to `true` (overflow included), which only costs time: a sliver's box is the whole map.
// area: the computed e(A1, A2, A3); min / max: over the three texel-space vertices, finite
RPT_LIGHTMAP_HD inline bool sliver(double area, double min_x, double max_x, double min_y, double max_y, uint32_t width, uint32_t height) {
  const double ex = max_x - min_x, ey = max_y - min_y, e = ex > ey ? ex : ey;
  double m = (double)(width > height ? width : height);
  m = std::fmax(m, std::fmax(std::fmax(std::fabs(min_x), std::fabs(max_x)), std::fmax(std::fabs(min_y), std::fabs(max_y))));
  const double bound = 0x1p-46 * ((2.0 * m) * (ex + ey) * e + ex * ey) + 0x1p-1000 * std::fmax(1.0, e);
  return !(std::fabs(area) > bound);
}

// ---- the map.  width * height + stream_base <= 2^32: every texel's stream id stream_base + y * width + x has 32 bits
constexpr uint64_t STREAMS = 1ull << 32;
constexpr uint64_t TRIS_MAX = (1ull << 31) - 1; // OWNER is an int32, and 0xFFFFFFFF is "nobody"
inline uint64_t texels(uint32_t width, uint32_t height) { return (uint64_t)width * height; }
inline bool streams_fit(uint32_t width, uint32_t height, uint32_t stream_base) {
  return texels(width, height) + stream_base <= STREAMS;
}

// ---- pieces: whole texel ranges [base, base + len) in row-major order.  fit: what one pass of the probe call may hold
// (rptplan::rays_piece's bound), asked: RPTGPU_LIGHTMAP_PIECE (0: not set).  A piece's compacted arrays are indexed with 32
// bits, and the scan's counts are uint32: a piece has at most PIECE_MAX texels
constexpr uint64_t PIECE_MAX = 4ull << 20;
inline uint64_t piece(uint64_t n_texels, uint64_t asked, uint64_t fit) {
  const uint64_t want = asked ? std::min(asked, PIECE_MAX) : PIECE_MAX;
  return std::max<uint64_t>(1, std::min(std::min(n_texels, want), std::max<uint64_t>(1, fit)));
}
inline uint64_t piece_count(uint64_t n_texels, uint64_t piece) { return (n_texels + piece - 1) / piece; }
inline uint64_t piece_len(uint64_t base, uint64_t n_texels, uint64_t piece) { return std::min(piece, n_texels - base); }

// ---- a piece's compacted arrays inside ONE f64 allocation, offsets in f64 words, each array 16-byte aligned: the gather
// points and normals [piece][3] and the stream ids [piece] uint32 — 52 B per owned texel —, then what the gathers return,
// irradiance [piece][3] and ao [piece], where named
struct Compact {
  uint64_t point, normal, ids, irradiance, ao; // irradiance / ao: valid where the flag says so
  bool has_irradiance, has_ao;
  uint64_t words;
};
inline uint64_t even(uint64_t w) { return (w + 1) / 2 * 2; }
inline Compact compact(uint64_t piece, bool irradiance, bool ao) {
  Compact c{};
  uint64_t off = 0;
  c.point = off; off += even(3 * piece);
  c.normal = off; off += even(3 * piece);
  c.ids = off; off += even((piece + 1) / 2);
  c.has_irradiance = irradiance; c.has_ao = ao;
  if (irradiance) { c.irradiance = off; off += even(3 * piece); }
  if (ao) { c.ao = off; off += even(piece); }
  c.words = off;
  return c;
}

// ---- RptLightmapArrays' channels in staging order (channel_plan.h): a host caller's whole map, the owners last
enum { R_IRRADIANCE, R_AO, R_BARYCENTRIC, R_POSITION, R_NORMAL, R_OWNER };
constexpr rptchan::Row ROWS[] = {RPT_CHANNEL_ROW(RptLightmapArrays, RPT_LIGHTMAP_IRRADIANCE, irradiance, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptLightmapArrays, RPT_LIGHTMAP_AO, ao, 1, 8, 0),
                                 RPT_CHANNEL_ROW(RptLightmapArrays, RPT_LIGHTMAP_BARYCENTRIC, barycentric, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptLightmapArrays, RPT_LIGHTMAP_POSITION, position, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptLightmapArrays, RPT_LIGHTMAP_NORMAL, normal, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptLightmapArrays, RPT_LIGHTMAP_OWNER, owner, 1, 4, 0)};

} // namespace rptlightmap
