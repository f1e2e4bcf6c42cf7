// lightmap_lookup.h — the device half of rptgpu_lookup_lightmap[_device] (kernels_lightmap_lookup.hip,
// kernels/lightmap_lookup.inc; the contract: include/rpt_gpu_lightmap_lookup.h): one kernel with one lane per ray that turns a
// first hit's object, triangle and barycentrics into a uv and a filtered texel of the map bound to that object, on gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rptlookup {

// a binding as the kernel reads it (RptLightmapBinding with its arrays on the device)
struct Binding {
  const double* uvs;    // [n_tris][3][2]
  const double* map;    // [height][width][components]
  const uint8_t* valid; // [height][width] or nullptr
  uint32_t n_tris, width, height, components;
};
// a piece's rays as rpt_hit_surface left them, the call's tables, and the named channels' arrays offset to the piece
struct Rays {
  const int32_t* object;      // [n]
  const int32_t* primitive;   // [n]
  const double* barycentric;  // [n][3]
  const int32_t* binding_of;  // [num_objects]: the binding of a top-level object, -1 without one
  const Binding* bindings;    // [n_bindings]
  uint32_t num_objects;
  uint32_t filter;            // RPT_LOOKUP_NEAREST / _BILINEAR
  double fallback[3];
  uint32_t channels;          // of RPT_LOOKUP_BINDING | _COVERED | _UV | _VALUE
  int32_t* binding;           // [n]
  uint8_t* covered;           // [n]
  double* uv;                 // [n][2]
  double* value;              // [n][3]
};

// enqueues rpt_lightmap_lookup over n rays on st -> hipGetLastError() of the launch
hipError_t lookup(hipStream_t st, uint32_t n, const Rays& r);

} // namespace rptlookup
