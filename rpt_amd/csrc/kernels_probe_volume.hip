// kernels_probe_volume.hip — rptgpu_sample_probe_volume's and rptgpu_lookup_probe_volume's kernels in a translation unit of
// their own (kernels/probe_volume.inc): every other code object of the library stays what it was without them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rpt_gpu.h"
#include "probe_volume_plan.h"
#include "probe_volume.h"

namespace rptvolume {
#define RPT_DEV __device__ __forceinline__
constexpr double PV_INF = __builtin_huge_val();
#include "kernels/vec.inc"
#include "kernels/sh9_basis.inc"
#include "kernels/probe_volume.inc"
} // namespace rptvolume
