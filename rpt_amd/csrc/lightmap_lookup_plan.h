// lightmap_lookup_plan.h — the host-only arithmetic of rptgpu_lookup_lightmap (api_lightmap_lookup.cpp): a piece's
// arrays inside one allocation of the handle — what rpt_hit_surface leaves for rpt_lightmap_lookup, and a host caller's staged
// channels —, a host caller's bindings staged whole, and the launch's grid.  No HIP, no handle:
// tests/cpp/lightmap_lookup_plan_check.cpp builds it alone, with the host sanitizers too.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rptlookup {

constexpr uint32_t BLOCK = 256;

// ---- channels and filters (include/rpt_gpu_lightmap_lookup.h RPT_LOOKUP_*)
constexpr uint32_t CH_T = 1u, CH_OBJECT = 2u, CH_BINDING = 4u, CH_COVERED = 8u, CH_UV = 16u, CH_VALUE = 32u, CH_ALL = 63u;
constexpr uint32_t FILTER_NEAREST = 0u, FILTER_BILINEAR = 1u;
// what the lookup kernel itself writes (T and OBJECT are the first-hit query's)
constexpr uint32_t CH_KERNEL = CH_BINDING | CH_COVERED | CH_UV | CH_VALUE;
inline bool needs_lookup(uint32_t channels) { return (channels & CH_KERNEL) != 0; }

// the blocks of a launch over m rays, one lane per ray
inline uint32_t launch_blocks(uint64_t m) { return (uint32_t)std::max<uint64_t>(1, (m + BLOCK - 1) / BLOCK); }

inline uint64_t even(uint64_t w) { return (w + 1) / 2 * 2; }
inline uint64_t i32_words(uint64_t count) { return even((count + 1) / 2); } // `count` int32 values, in f64 words
inline uint64_t u8_words(uint64_t count) { return even((count + 7) / 8); }  // `count` bytes, in f64 words

// ---- a piece's arrays inside ONE f64 allocation: offsets in f64 words, each array 16-byte aligned, the f64 arrays first.
// `has` names what lies there.  The hit's own four — T, OBJECT, and rpt_hit_surface's PRIMITIVE and BARYCENTRIC (bits of their
// own here: the caller never sees them) — are there whenever the lookup kernel runs; T and OBJECT too when a host caller named
// them, and NOT when a device caller did: the query then writes the caller's arrays and the kernels read those.  BINDING,
// COVERED, UV, VALUE are there for a host caller that named them (its staging)
constexpr uint32_t IN_PRIMITIVE = 64u, IN_BARYCENTRIC = 128u;
struct Layout {
  uint64_t t, barycentric, uv, value, object, primitive, binding, covered; // valid where `has` names the array
  uint32_t has;
  uint64_t words;
};
inline Layout layout(uint64_t piece, uint32_t channels, bool on_device) {
  Layout l{};
  uint32_t has = on_device ? 0u : (channels & CH_ALL);
  if (needs_lookup(channels)) {
    has |= IN_PRIMITIVE | IN_BARYCENTRIC;
    if (!on_device || !(channels & CH_T)) has |= CH_T;
    if (!on_device || !(channels & CH_OBJECT)) has |= CH_OBJECT;
  }
  uint64_t off = 0;
  if (has & CH_T) { l.t = off; off += even(piece); }
  if (has & IN_BARYCENTRIC) { l.barycentric = off; off += even(3 * piece); }
  if (has & CH_UV) { l.uv = off; off += even(2 * piece); }
  if (has & CH_VALUE) { l.value = off; off += even(3 * piece); }
  if (has & CH_OBJECT) { l.object = off; off += i32_words(piece); }
  if (has & IN_PRIMITIVE) { l.primitive = off; off += i32_words(piece); }
  if (has & CH_BINDING) { l.binding = off; off += i32_words(piece); }
  if (has & CH_COVERED) { l.covered = off; off += u8_words(piece); }
  l.has = has;
  l.words = off;
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
