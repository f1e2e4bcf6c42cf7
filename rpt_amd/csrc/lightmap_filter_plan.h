// lightmap_filter_plan.h — the host-only arithmetic of rptgpu_filter_lightmap (api_lightmap_filter.cpp): the
// limits of a map, the layout of the filter's columns inside ONE f64 allocation, the dilation's second copy and flags inside
// that same allocation, a host caller's staging, and the launch geometry of the three kernels.  No HIP, no handle:
// tests/cpp/lightmap_filter_plan_check.cpp builds it alone, with the host sanitizers too.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rptlightmapfilter {

constexpr uint64_t TEXELS_MAX = 1ull << 32; // width * height at the most
constexpr uint32_t LEVELS_MAX = 8;          // tap spacings 1 .. 128
inline uint64_t texels(uint32_t width, uint32_t height) { return (uint64_t)width * height; }
inline bool map_fits(uint32_t width, uint32_t height) { return width && height && texels(width, height) <= TEXELS_MAX; }
inline bool words_ok(uint32_t words) { return words == 1 || words == 3; }
inline uint32_t step(uint32_t level) { return 1u << level; } // level < LEVELS_MAX
// the rounds of the dilation that are run: after max(W, H) of them nothing is left to fill
inline uint32_t rounds(uint32_t dilate, uint32_t width, uint32_t height) { return std::min(dilate, std::max(width, height)); }

// ---- the workspace: offsets in f64 words into one allocation of `words` f64, every array 16-byte aligned.  position and
// normal: three columns of n each (component k of texel p at [k * n + p]); c[2]: the two ping-pong sets of `comps` columns;
// v[2]: the two variance columns (has_variance); valid: n bytes, the last array.  Per texel 8 * (6 + 2 * comps + (variance ?
// 2 : 0)) + 1 bytes: 113 at 3 words with a variance.
// The dilation runs when the filter is done with everything but `valid`, which is its round-0 flags: its second set of
// flags (n bytes) lies over `position`, its second copy of the map ([n][comps] f64, interleaved) over c[0] .. c[1].
struct Workspace {
  uint64_t position, normal, c[2], v[2], valid; // v: valid where has_variance
  uint64_t flags2, pong;                        // the dilation's, aliases of position and c[0]
  bool has_variance;
  uint64_t words;                               // f64 words of the whole allocation
};
inline uint64_t even(uint64_t w) { return (w + 1) / 2 * 2; }
inline Workspace workspace(uint64_t n, uint32_t comps, bool variance) {
  Workspace w{};
  uint64_t off = 0;
  w.position = off; off += even(3 * n);
  w.normal = off; off += even(3 * n);
  w.c[0] = off; off += even((uint64_t)comps * n);
  w.c[1] = off; off += even((uint64_t)comps * n);
  w.has_variance = variance;
  if (variance) {
    w.v[0] = off; off += even(n);
    w.v[1] = off; off += even(n);
  }
  w.valid = off; off += even((n + 7) / 8);
  w.flags2 = w.position; // n bytes <= 24 n
  w.pong = w.c[0];       // comps * n words <= 2 * even(comps * n)
  w.words = off;
  return w;
}
// the set a level reads and the set it writes; after `levels` levels the result lies in set result_set(levels)
inline uint32_t source_set(uint32_t level) { return level % 2; }
inline uint32_t result_set(uint32_t levels) { return levels % 2; }

// ---- a host caller's arrays staged on the device, in one f64 allocation in the same way: the inputs, then the outputs
struct Stage {
  uint64_t position, normal, values, variance, out, out_variance, owner; // variance / out_variance: valid where the flags say so
  bool has_variance, has_out_variance;
  uint64_t words;
};
inline Stage stage(uint64_t n, uint32_t comps, bool variance, bool out_variance) {
  Stage s{};
  uint64_t off = 0;
  s.position = off; off += even(3 * n);
  s.normal = off; off += even(3 * n);
  s.values = off; off += even((uint64_t)comps * n);
  s.has_variance = variance; s.has_out_variance = out_variance;
  if (variance) { s.variance = off; off += even(n); }
  s.out = off; off += even((uint64_t)comps * n);
  if (out_variance) { s.out_variance = off; off += even(n); }
  s.owner = off; off += even((n + 1) / 2); // int32
  s.words = off;
  return s;
}

// ---- the launches.  prepare and level: blocks of 64 x 4 lanes, one lane per texel, a wave 64 consecutive x of one row.
// grid.x covers the width (at most 2^26 blocks); grid.y is cut to GRID_Y_MAX and a block walks down the map in strides of
// 4 * grid.y rows, so a map of any height the limits allow is one launch.  finish: 256 lanes, one per texel, a grid-stride
// loop over at most FINISH_GRID_MAX blocks.
constexpr uint32_t BLOCK_X = 64, BLOCK_Y = 4, FINISH_BLOCK = 256;
constexpr uint32_t GRID_Y_MAX = 65535, FINISH_GRID_MAX = 1u << 20;
struct Grid {
  uint32_t x, y;
};
inline Grid grid(uint32_t width, uint32_t height) {
  const uint64_t gx = ((uint64_t)width + BLOCK_X - 1) / BLOCK_X, gy = ((uint64_t)height + BLOCK_Y - 1) / BLOCK_Y;
  return Grid{(uint32_t)std::max<uint64_t>(1, gx), (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, gy), GRID_Y_MAX)};
}
inline uint32_t finish_blocks(uint64_t n) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (n + FINISH_BLOCK - 1) / FINISH_BLOCK), FINISH_GRID_MAX);
}

} // namespace rptlightmapfilter
