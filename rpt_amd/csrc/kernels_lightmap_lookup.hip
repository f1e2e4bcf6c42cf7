// kernels_lightmap_lookup.hip — rptgpu_lookup_lightmap's kernel in a translation unit of its own
// (kernels/lightmap_lookup.inc): every other code object of the library stays what it was without it.
#include <hip/hip_runtime.h>

#include "../../include/rpt_gpu.h"
#include "lightmap_lookup_plan.h"
#include "lightmap_lookup.h"

namespace rptlookup {
#define LK_DEV __device__ __forceinline__
constexpr double LK_INF = __builtin_huge_val();
#include "kernels/lightmap_lookup.inc"
} // namespace rptlookup
