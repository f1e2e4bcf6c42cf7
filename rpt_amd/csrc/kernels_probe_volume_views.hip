// kernels_probe_volume_views.hip — rptgpu_render_views_probe_lit's kernel in a translation unit of its own
// (kernels/probe_volume_views.inc over the rule of kernels/probe_volume.inc): every other code object of the
// library stays what it was without it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rpt_gpu.h"
#include "probe_volume.h"

namespace rptvolumeviews {
using rptvolume::Volume;
#define RPT_DEV __device__ __forceinline__
constexpr double PV_INF = __builtin_huge_val();
#include "kernels/vec.inc"
#include "kernels/sh9_basis.inc"
#define PV_RULE_ONLY
#include "kernels/probe_volume.inc"
#include "kernels/probe_volume_views.inc"
} // namespace rptvolumeviews
