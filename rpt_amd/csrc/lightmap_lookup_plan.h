// lightmap_lookup_plan.h — the host-only arithmetic of rptgpu_lookup_lightmap (api_lightmap_lookup.cpp):
// RptLookupArrays' channel table (channel_plan.h) and which of its arrays the handle keeps for a piece — what rpt_hit_surface
// leaves for rpt_lightmap_lookup, and a host caller's staged channels —, a host caller's bindings staged whole, and the
// launch's grid.  No HIP, no handle:
// tests/cpp/lightmap_lookup_plan_check.cpp builds it alone, with the host sanitizers too.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/rpt_gpu.h"
#include "channel_plan.h"

namespace rptlookup {
using rptchan::even;
using rptchan::i32_words;
using rptchan::u8_words;

constexpr uint32_t BLOCK = 256;

// ---- channels and filters (include/rpt_gpu_lightmap_lookup.h RPT_LOOKUP_*)
constexpr uint32_t CH_T = 1u, CH_OBJECT = 2u, CH_BINDING = 4u, CH_COVERED = 8u, CH_UV = 16u, CH_VALUE = 32u, CH_ALL = 63u;
constexpr uint32_t FILTER_NEAREST = 0u, FILTER_BILINEAR = 1u;
// what the lookup kernel itself writes (T and OBJECT are the first-hit query's)
constexpr uint32_t CH_KERNEL = CH_BINDING | CH_COVERED | CH_UV | CH_VALUE;
inline bool needs_lookup(uint32_t channels) { return (channels & CH_KERNEL) != 0; }

// the blocks of a launch over m rays, one lane per ray
inline uint32_t launch_blocks(uint64_t m) { return (uint32_t)std::max<uint64_t>(1, (m + BLOCK - 1) / BLOCK); }

// ---- RptLookupArrays' channels in staging order (channel_plan.h) — BARYCENTRIC stands between T and UV —, and a piece's
// arrays inside one allocation of the handle.  `has` names what lies there.  The hit's own four — T, OBJECT, and
// rpt_hit_surface's PRIMITIVE and BARYCENTRIC (rows with bits of their own here: the caller never sees them) — are there
// whenever the lookup kernel runs; T and OBJECT too when a host caller named them, and NOT when a device caller did: the query
// then writes the caller's arrays and the kernels read those.  BINDING, COVERED, UV, VALUE are there for a host caller that
// named them (its staging)
constexpr uint32_t IN_PRIMITIVE = 64u, IN_BARYCENTRIC = 128u;
enum { R_T, R_BARYCENTRIC, R_UV, R_VALUE, R_OBJECT, R_PRIMITIVE, R_BINDING, R_COVERED };
constexpr rptchan::Row ROWS[] = {RPT_CHANNEL_ROW(RptLookupArrays, RPT_LOOKUP_T, t, 1, 8, 0),
                                 RPT_INTERNAL_ROW(IN_BARYCENTRIC, 3, 8),
                                 RPT_CHANNEL_ROW(RptLookupArrays, RPT_LOOKUP_UV, uv, 2, 8, 0),
                                 RPT_CHANNEL_ROW(RptLookupArrays, RPT_LOOKUP_VALUE, value, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptLookupArrays, RPT_LOOKUP_OBJECT, object, 1, 4, 0),
                                 RPT_INTERNAL_ROW(IN_PRIMITIVE, 1, 4),
                                 RPT_CHANNEL_ROW(RptLookupArrays, RPT_LOOKUP_BINDING, binding, 1, 4, 0),
                                 RPT_CHANNEL_ROW(RptLookupArrays, RPT_LOOKUP_COVERED, covered, 1, 1, 0)};
struct Layout : rptchan::Layout {
  uint64_t t, barycentric, uv, value, object, primitive, binding, covered; // the rows' offsets by name (0: not there)
};
inline Layout layout(uint64_t piece, uint32_t channels, bool on_device) {
  uint32_t has = on_device ? 0u : (channels & CH_ALL);
  if (needs_lookup(channels)) {
    has |= IN_PRIMITIVE | IN_BARYCENTRIC;
    if (!on_device || !(channels & CH_T)) has |= CH_T;
    if (!on_device || !(channels & CH_OBJECT)) has |= CH_OBJECT;
  }
  Layout l{};
  static_cast<rptchan::Layout&>(l) = rptchan::layout(ROWS, has, piece);
  l.t = rptchan::off_or_0(l, R_T); l.barycentric = rptchan::off_or_0(l, R_BARYCENTRIC);
  l.uv = rptchan::off_or_0(l, R_UV); l.value = rptchan::off_or_0(l, R_VALUE); l.object = rptchan::off_or_0(l, R_OBJECT);
  l.primitive = rptchan::off_or_0(l, R_PRIMITIVE); l.binding = rptchan::off_or_0(l, R_BINDING);
  l.covered = rptchan::off_or_0(l, R_COVERED);
  return l;
}

// ---- a host caller's binding, staged whole behind the ones before it: offsets in f64 words from `base`; ok == false: the sizes
// do not fit 2^60 words (no such map exists; the call is refused)
struct Staged {
  uint64_t uvs, map, valid; // valid: meaningful with has_valid
  uint64_t uv_words, map_words, valid_bytes;
  uint64_t end;             // where the next binding starts
  bool ok;
};
constexpr uint64_t WORDS_MAX = 1ull << 60;
inline Staged stage_binding(uint64_t base, uint32_t n_tris, uint32_t width, uint32_t height, uint32_t components, bool has_valid) {
  Staged s{};
  const uint64_t texels = (uint64_t)width * height; // < 2^64: both are 32-bit
  if (base > WORDS_MAX || texels > WORDS_MAX / 4 || components > 3) return s;
  s.uv_words = 6ull * n_tris;
  s.map_words = texels * components;
  s.valid_bytes = has_valid ? texels : 0;
  s.uvs = base;
  s.map = s.uvs + even(s.uv_words);
  s.valid = s.map + even(s.map_words);
  s.end = s.valid + u8_words(s.valid_bytes);
  s.ok = s.end <= WORDS_MAX;
  return s;
}

} // namespace rptlookup
