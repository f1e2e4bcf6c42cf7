// probe_volume_plan.h — the host-only arithmetic of rptgpu_sample_probe_volume, rptgpu_lookup_probe_volume and
// rptgpu_render_views_probe_lit (api_probe_volume.cpp): the checks of a volume's numbers, the points or rays
// per piece, RptVolumeArrays' channel table (channel_plan.h) and which of its arrays the handle keeps for a piece — what the
// first-hit query leaves for rpt_probe_volume_lookup, and a host caller's staged channels —, a host caller's volume staged
// whole, and the launch's grid.  No HIP, no handle:
// tests/cpp/probe_volume_plan_check.cpp builds it alone, with the host sanitizers too.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/rpt_gpu.h"
#include "channel_plan.h"

namespace rptvolume {
using rptchan::even;
using rptchan::u8_words;

constexpr uint32_t BLOCK = 256;

// ---- channels (include/rpt_gpu_probe_volume.h RPT_VOLUME_*)
constexpr uint32_t CH_T = 1u, CH_OBJECT = 2u, CH_POSITION = 4u, CH_NORMAL = 8u, CH_VALUE = 16u, CH_COVERED = 32u, CH_INSIDE = 64u;
constexpr uint32_t CH_ALL = 127u;
// what the point form knows (no ray, no hit), and what of a ray's record is the first-hit query's own
constexpr uint32_t CH_POINT = CH_VALUE | CH_COVERED | CH_INSIDE;
constexpr uint32_t CH_HIT = CH_T | CH_OBJECT | CH_POSITION | CH_NORMAL;

// the blocks of a launch over m points, one lane per point
inline uint32_t launch_blocks(uint64_t m) { return (uint32_t)std::max<uint64_t>(1, (m + BLOCK - 1) / BLOCK); }

// ---- the volume's numbers: what is wrong with them (nullptr: nothing), in the header's order.  The pointers are the caller's
// business (api_probe_volume.cpp); PROBES_MAX keeps 27 f64 per probe inside 2^60 words
constexpr uint64_t PROBES_MAX = 1ull << 55;
inline uint64_t probe_count(uint32_t nx, uint32_t ny, uint32_t nz, bool& fits) { // nx, ny, nz >= 1
  const uint64_t xy = (uint64_t)nx * ny; // < 2^64: both are 32-bit
  fits = xy <= PROBES_MAX / nz;
  return fits ? xy * nz : 0;
}
inline const char* bad_grid(uint32_t nx, uint32_t ny, uint32_t nz, const double origin[3], const double spacing[3]) {
  if (!nx || !ny || !nz) return "RptProbeVolume: a count of 0 (nx, ny and nz are each >= 1)";
  for (int a = 0; a < 3; a++)
    if (!(std::isfinite(spacing[a]) && spacing[a] > 0.0)) return "RptProbeVolume: spacing is not finite and positive";
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(origin[a])) return "RptProbeVolume: origin is not finite";
  return nullptr;
}

// ---- the points or rays per piece: what the environment asks for (0: nothing), else `bound` — the first-hit query's own
// piece for rays, POINTS_PIECE for points —, never more than n or than a launch's 32-bit index, never 0
constexpr uint64_t POINTS_PIECE = 1ull << 22;
inline uint64_t piece(uint64_t n, uint64_t asked, uint64_t bound) {
  uint64_t p = asked ? std::min(asked, bound) : bound;
  p = std::min<uint64_t>(p, 1ull << 30);
  return std::max<uint64_t>(1, std::min(p, n));
}

// ---- RptVolumeArrays' channels in staging order (channel_plan.h), and a piece's arrays inside one allocation of the handle.
// `has` names what lies there.  The first-hit query's four — T, OBJECT, NORMAL, POSITION — are there whenever a ray form
// runs (`rays`): the query writes them and rpt_probe_volume_lookup reads them; a host caller's T, OBJECT, POSITION and NORMAL
// are those same arrays, rewritten in place by the lane that read them.  VALUE, COVERED, INSIDE are there for a host caller
// that named them (its staging)
enum { R_T, R_POSITION, R_NORMAL, R_VALUE, R_OBJECT, R_COVERED, R_INSIDE };
constexpr rptchan::Row ROWS[] = {RPT_CHANNEL_ROW(RptVolumeArrays, RPT_VOLUME_T, t, 1, 8, 0),
                                 RPT_CHANNEL_ROW(RptVolumeArrays, RPT_VOLUME_POSITION, position, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptVolumeArrays, RPT_VOLUME_NORMAL, normal, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptVolumeArrays, RPT_VOLUME_VALUE, value, 3, 8, 0),
                                 RPT_CHANNEL_ROW(RptVolumeArrays, RPT_VOLUME_OBJECT, object, 1, 4, 0),
                                 RPT_CHANNEL_ROW(RptVolumeArrays, RPT_VOLUME_COVERED, covered, 1, 1, 0),
                                 RPT_CHANNEL_ROW(RptVolumeArrays, RPT_VOLUME_INSIDE, inside, 1, 1, 0)};
struct Layout : rptchan::Layout {
  uint64_t t, position, normal, value, object, covered, inside; // the rows' offsets by name (0: not there)
};
inline Layout layout(uint64_t piece, uint32_t channels, bool rays, bool on_device) {
  uint32_t has = on_device ? 0u : (channels & CH_POINT);
  if (rays) has |= CH_HIT;
  Layout l{};
  static_cast<rptchan::Layout&>(l) = rptchan::layout(ROWS, has, piece);
  l.t = rptchan::off_or_0(l, R_T); l.position = rptchan::off_or_0(l, R_POSITION);
  l.normal = rptchan::off_or_0(l, R_NORMAL); l.value = rptchan::off_or_0(l, R_VALUE);
  l.object = rptchan::off_or_0(l, R_OBJECT); l.covered = rptchan::off_or_0(l, R_COVERED);
  l.inside = rptchan::off_or_0(l, R_INSIDE);
  return l;
}

// ---- a host caller's volume, staged whole: offsets in f64 words; ok == false: the probes fit no allocation
struct Staged {
  uint64_t coeffs, valid;         // valid: meaningful with has_valid
  uint64_t coeff_words, valid_bytes;
  uint64_t words;
  bool ok;
};
inline Staged stage_volume(uint64_t probes, bool has_valid) {
  Staged s{};
  if (probes > PROBES_MAX) return s;
  s.coeff_words = 27 * probes;
  s.valid_bytes = has_valid ? probes : 0;
  s.coeffs = 0;
  s.valid = even(s.coeff_words);
  s.words = s.valid + u8_words(s.valid_bytes);
  s.ok = true;
  return s;
}

} // namespace rptvolume
