// surface_plan.h — the host-only arithmetic of rptgpu_hit_surface (api_surface.cpp): the columns of
// rpt_hit_surface's walk (kernels/hit_surface.inc), the handle's scratch pair for T and OBJECT, and a host caller's staging
// layout.  No HIP, no handle: tests/cpp/surface_plan_check.cpp builds it alone, with the host sanitizers too.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rptsurface {

// ---- the walk's columns.  rpt_hit_surface keeps generic_walk's two kinds of pending work in global memory, one column per
// thread of a bounded grid: deferred far children [levels][8][threads] and suspended group leaves [frames][12][threads], f64
// words.  levels and frames are the scene's (FlatScene::generic_levels / generic_frames: what holds ANY object of the scene,
// live rebuilds included), at least 1; the grid is what covers the piece, capped at COLUMN_BLOCKS_MAX blocks and at what
// COLUMN_BYTES_MAX holds, never below one block — rays beyond it are taken in strides of the grid
constexpr uint32_t BLOCK = 256;
constexpr uint32_t COLUMN_BLOCKS_MAX = 1024;            // 262 144 lanes: four waves per SIMD of 256 CUs
constexpr uint64_t COLUMN_BYTES_MAX = 512ull << 20;     // of both arrays together
constexpr uint32_t DEFER_WORDS = 8, FRAME_WORDS = 12;

struct Columns {
  uint32_t threads, levels, frames; // threads: a multiple of BLOCK, >= BLOCK
  uint64_t defer_words, frame_words; // f64 words to allocate
};
inline uint64_t column_bytes_per_thread(uint32_t levels, uint32_t frames) {
  return ((uint64_t)levels * DEFER_WORDS + (uint64_t)frames * FRAME_WORDS) * 8u;
}
inline Columns columns(uint64_t piece, uint32_t gen_levels, uint32_t gen_frames) {
  Columns c{};
  c.levels = std::max(1u, gen_levels);
  c.frames = std::max(1u, gen_frames);
  const uint64_t blocks_piece = std::max<uint64_t>(1, (piece + BLOCK - 1) / BLOCK);
  const uint64_t blocks_mem = std::max<uint64_t>(1, COLUMN_BYTES_MAX / (column_bytes_per_thread(c.levels, c.frames) * BLOCK));
  c.threads = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(blocks_piece, COLUMN_BLOCKS_MAX), blocks_mem) * BLOCK;
  c.defer_words = (uint64_t)c.levels * DEFER_WORDS * c.threads;
  c.frame_words = (uint64_t)c.frames * FRAME_WORDS * c.threads;
  return c;
}
// the blocks of a launch over m rays with these columns: every thread of the grid owns a column
inline uint32_t launch_blocks(uint64_t m, const Columns& c) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (m + BLOCK - 1) / BLOCK), c.threads / BLOCK);
}

// ---- channels (include/rpt_gpu_hit_surface.h RPT_SURFACE_*)
constexpr uint32_t CH_T = 1u, CH_OBJECT = 2u, CH_CHILD = 4u, CH_PRIMITIVE = 8u, CH_BARYCENTRIC = 16u, CH_ALL = 31u;
// does the call need the resolve walk at all?  (T and OBJECT are the first-hit query's)
inline bool needs_walk(uint32_t channels) { return (channels & (CH_CHILD | CH_PRIMITIVE | CH_BARYCENTRIC)) != 0; }

// ---- a piece's arrays inside ONE f64 allocation: offsets in f64 words, each array 16-byte aligned, the f64 channels first.
// `stage`: which of the caller's channels are staged there (a host caller: all it named; a device caller: none).  T and
// OBJECT are always present for a piece that walks — the walk reads them —: staged, or as the handle's scratch pair
struct Layout {
  uint64_t t, barycentric, object, child, primitive; // valid where `has` names the channel
  uint32_t has;
  uint64_t words;
};
inline uint64_t even(uint64_t w) { return (w + 1) / 2 * 2; }
inline uint64_t i32_words(uint64_t piece) { return even((piece + 1) / 2); } // `piece` int32 values, in f64 words
inline Layout layout(uint64_t piece, uint32_t channels, bool on_device) {
  Layout l{};
  uint32_t has = on_device ? 0u : (channels & CH_ALL);
  if (needs_walk(channels)) { // the scratch pair, where the caller's own arrays do not serve (not named, or host memory)
    if (!on_device || !(channels & CH_T)) has |= CH_T;
    if (!on_device || !(channels & CH_OBJECT)) has |= CH_OBJECT;
  }
  uint64_t off = 0;
  if (has & CH_T) { l.t = off; off += even(piece); }
  if (has & CH_BARYCENTRIC) { l.barycentric = off; off += even(3 * piece); }
  if (has & CH_OBJECT) { l.object = off; off += i32_words(piece); }
  if (has & CH_CHILD) { l.child = off; off += i32_words(piece); }
  if (has & CH_PRIMITIVE) { l.primitive = off; off += i32_words(piece); }
  l.has = has;
  l.words = off;
  return l;
}

} // namespace rptsurface
