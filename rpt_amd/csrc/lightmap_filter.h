// lightmap_filter.h — the device half of rptgpu_filter_lightmap[_device] (kernels_lightmap_filter.hip,
// kernels/lightmap_filter.inc; the contract: include/rpt_gpu_lightmap_filter.h): the guides laid down as columns, one a-trous
// level, and the columns written back, on gfx950.  Every launcher enqueues on st and returns hipGetLastError() of its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rptlightmapfilter {

// the caller's arrays (RptLightmapFilterArrays' inputs, on the device)
struct Inputs {
  const int32_t* owner;   // [n]
  const double* position; // [n][3]
  const double* normal;   // [n][3]
  const double* values;   // [n][words]
  const double* variance; // [n] or nullptr
};
// the guides as columns: component k of texel p at [k * stride + p]; valid: one byte per texel
struct Guides {
  double* position;
  double* normal;
  uint8_t* valid;
  uint64_t stride; // = width * height
  uint32_t width, height;
};
struct Sigmas {
  double normal, plane, distance, color; // color: read only with a variance
};

// g's columns and valid bytes from `in`, values as columns into c (words columns), and with in.variance the prefiltered
// variance into v (a texel that is not valid: its variance as it is)
hipError_t prepare(hipStream_t st, const Inputs& in, uint32_t words, const Guides& g, double* c, double* v);
// one level with tap spacing `step` from (c_in, v_in) into (c_out, v_out); v_in == nullptr: no variance
hipError_t level(hipStream_t st, const Guides& g, uint32_t words, const double* c_in, const double* v_in, double* c_out,
                 double* v_out, uint32_t step, const Sigmas& sg);
// out[p][0, words) from c's columns, and out_variance[p] = v[p] where out_variance is given
hipError_t finish(hipStream_t st, uint64_t n, uint32_t words, const double* c, const double* v, double* out, double* out_variance);

} // namespace rptlightmapfilter
