// surface_plan.h — the host-only arithmetic of rptgpu_hit_surface (api_surface.cpp): the columns of
// rpt_hit_surface's walk (kernels/hit_surface.inc), RptSurfaceArrays' channel table (channel_plan.h) and which of its arrays
// the handle keeps for a piece: the scratch pair for T and OBJECT, a host caller's staging.  No HIP, no handle:
// tests/cpp/surface_plan_check.cpp builds it alone, with the host sanitizers too.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/rpt_gpu.h"
#include "channel_plan.h"

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

// ---- RptSurfaceArrays' channels in staging order (channel_plan.h), and a piece's arrays inside one allocation of the handle.
// `stage`: which of the caller's channels are staged there (a host caller: all it named; a device caller: none).  T and
// OBJECT are always present for a piece that walks — the walk reads them —: staged, or as the handle's scratch pair
enum { R_T, R_BARYCENTRIC, R_OBJECT, R_CHILD, R_PRIMITIVE };
constexpr rptchan::Row ROWS[] = {RPT_CHANNEL_ROW(RptSurfaceArrays, RPT_SURFACE_T, t, 1, 8, 0),
                                 RPT_CHANNEL_ROW(RptSurfaceArrays, RPT_SURFACE_BARYCENTRIC, barycentric, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptSurfaceArrays, RPT_SURFACE_OBJECT, object, 1, 4, 0),
                                 RPT_CHANNEL_ROW(RptSurfaceArrays, RPT_SURFACE_CHILD, child, 1, 4, 0),
                                 RPT_CHANNEL_ROW(RptSurfaceArrays, RPT_SURFACE_PRIMITIVE, primitive, 1, 4, 0)};
struct Layout : rptchan::Layout {
  uint64_t t, barycentric, object, child, primitive; // the rows' offsets by name (0: not there)
};
inline Layout layout(uint64_t piece, uint32_t channels, bool on_device) {
  uint32_t has = on_device ? 0u : (channels & CH_ALL);
  if (needs_walk(channels)) { // the scratch pair, where the caller's own arrays do not serve (not named, or host memory)
    if (!on_device || !(channels & CH_T)) has |= CH_T;
    if (!on_device || !(channels & CH_OBJECT)) has |= CH_OBJECT;
  }
  Layout l{};
  static_cast<rptchan::Layout&>(l) = rptchan::layout(ROWS, has, piece);
  l.t = rptchan::off_or_0(l, R_T); l.barycentric = rptchan::off_or_0(l, R_BARYCENTRIC);
  l.object = rptchan::off_or_0(l, R_OBJECT); l.child = rptchan::off_or_0(l, R_CHILD);
  l.primitive = rptchan::off_or_0(l, R_PRIMITIVE);
  return l;
}

} // namespace rptsurface
