// kernels_lightmap_views.hip — rptgpu_render_views_lightmapped's kernels in a translation unit of their own
// (kernels/lightmap_views.inc): every other code object of the library stays what it was without them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rpt_gpu.h"
#include "../../include/rpt_math.h"
#include "math_converged.h"
#include "lightmap_views.h"

namespace rptlookupviews {
using namespace rptdev;
#define RPT_DEV __device__ __forceinline__
constexpr double PI = 3.14159265358979323846264338327950288;
constexpr double TAU = 6.28318530717958647692528676655900577;
#include "kernels/vec.inc"
#include "kernels/lightmap_views.inc"
} // namespace rptlookupviews
