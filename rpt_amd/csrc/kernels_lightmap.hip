// kernels_lightmap.hip — rptgpu_bake_lightmap's kernels in a translation unit of their own (kernels/lightmap.inc, DESIGN.md
// §22): every other code object of the library stays what it was without them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#define RPT_LIGHTMAP_HD __host__ __device__
#include "lightmap_plan.h"
#include "lightmap.h"

namespace rptlightmap {
#include "kernels/lightmap.inc"
} // namespace rptlightmap
