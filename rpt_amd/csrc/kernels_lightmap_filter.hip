// kernels_lightmap_filter.hip — rptgpu_filter_lightmap's kernels in a translation unit of their own
// (kernels/lightmap_filter.inc): every other code object of the library, kernels_lightmap.o included, stays
// what it was without them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "math_converged.h"
#include "lightmap_filter_plan.h"
#include "lightmap_filter.h"

namespace rptlightmapfilter {
constexpr double LF_INF = __builtin_huge_val();
#include "kernels/lightmap_filter.inc"
} // namespace rptlightmapfilter
