// lightmap_views.h — the device half of rptgpu_render_views_lightmapped[_device] beside the ray form's (lightmap_lookup.h):
// the views' rays laid out interleaved, and the fold of a sample's shading into the frame (kernels_lightmap_views.hip,
// kernels/lightmap_views.inc; the contract: include/rpt_gpu_lightmap_lookup.h).  Every launcher enqueues on st and returns
// hipGetLastError() of its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"

namespace rptlookupviews {

// rays[6][cap] (rpt_raygen_views' SoA: ox oy oz dx dy dz) -> origins[m][3], dirs[m][3]
hipError_t gather_rays(hipStream_t st, const double* rays, uint64_t cap, uint32_t m, double* origins, double* dirs);

// one sample of a piece of m indices into out[m][3]
struct Sample {
  const int32_t* object;   // [m] the first hits' objects, -1: a miss
  const double* dirs;      // [m][3] the rays' directions (the environment's argument)
  const uint8_t* covered;  // [m] the lookup's COVERED
  const double* value;     // [m][3] ... and VALUE
  double unbound[3];       // I of a hit that is not covered
  uint32_t first, last;    // the call's first sample: the sums start from +0.0; its last: they are scaled
  double iterations, ev_scale;
};
hipError_t fold(hipStream_t st, const rptdev::Scene& sc, uint32_t m, const Sample& s, double* out);

} // namespace rptlookupviews
