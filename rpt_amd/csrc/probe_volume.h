// probe_volume.h — the device half of rptgpu_sample_probe_volume, rptgpu_lookup_probe_volume and
// rptgpu_render_views_probe_lit (kernels_probe_volume.hip, kernels_probe_volume_views.hip, kernels/probe_volume.inc,
// kernels/probe_volume_views.inc; the contract: include/rpt_gpu_probe_volume.h): a grid of SH9 probes interpolated at a point
// and convolved with the clamped cosine about a direction, one lane per point, on gfx950.  Every launcher enqueues on st and
// returns hipGetLastError() of its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rptvolume {

// a volume as the kernels read it (RptProbeVolume with its arrays on the device)
struct Volume {
  const double* coeffs;  // [nz][ny][nx][9][3]
  const uint8_t* valid;  // [nz][ny][nx] or nullptr
  uint32_t nx, ny, nz;
  double origin[3], spacing[3];
  double normal_bias;
};

// rptgpu_sample_probe_volume: a piece's points and the named channels' arrays offset to the piece
struct Points {
  const double* positions; // [n][3]
  const double* normals;   // [n][3]
  double fallback[3];
  uint32_t channels;       // of RPT_VOLUME_VALUE | _COVERED | _INSIDE
  double* value;           // [n][3]
  uint8_t* covered;        // [n]
  uint8_t* inside;         // [n]
};
hipError_t sample(hipStream_t st, uint32_t n, const Volume& v, const Points& p);

// rptgpu_lookup_probe_volume: a piece's rays' directions, their first hits as rptgpu_first_hits' query left them, and the named
// channels' arrays offset to the piece.  An output array may BE the hit array of its channel (a host caller's staging): a lane
// reads its ray's record before it writes anything
struct Hits {
  const double* dirs;      // [n][3]
  const double* t;         // [n]
  const int32_t* object;   // [n]
  const double* normal;    // [n][3]
  const double* position;  // [n][3]
  double fallback[3];
  uint32_t channels;       // RPT_VOLUME_*
  double* o_t;             // [n]
  int32_t* o_object;       // [n]
  double* o_position;      // [n][3]
  double* o_normal;        // [n][3]
  double* o_value;         // [n][3]
  uint8_t* o_covered;      // [n]
  uint8_t* o_inside;       // [n]
};
hipError_t lookup(hipStream_t st, uint32_t n, const Volume& v, const Hits& r);

} // namespace rptvolume

namespace rptvolumeviews {

// rptgpu_render_views_probe_lit: one sample of a piece of m indices between rpt_lightmap_lookup and
// rpt_views_lightmapped_fold.  For every hit the lookup left uncovered (lightmaps == 0: it did not run, nothing is covered) the
// volume rule at the hit: covered -> value = E cut at zero and covered = 1; else covered = 0
struct Merge {
  const double* dirs;      // [m][3]
  const int32_t* object;   // [m] -1: a miss (left alone)
  const double* normal;    // [m][3] rptgpu_first_hits' NORMAL
  const double* position;  // [m][3] ... and POSITION
  uint32_t lightmaps;
  uint8_t* covered;        // [m] the lookup's COVERED, updated
  double* value;           // [m][3] ... and VALUE
};
hipError_t merge(hipStream_t st, uint32_t m, const rptvolume::Volume& v, const Merge& g);

} // namespace rptvolumeviews
