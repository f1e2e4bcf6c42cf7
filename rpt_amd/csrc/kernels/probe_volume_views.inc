// kernels/probe_volume_views.inc — rptgpu_render_views_probe_lit's one kernel of its own (include/rpt_gpu_probe_volume.h,
// DESIGN.md §26).  rpt_views_probe_lit_merge stands between rpt_lightmap_lookup and rpt_views_lightmapped_fold, both unchanged:
// per index of the piece whose sample hit something and whose hit no lightmap covers, the volume rule (kernels/probe_volume.inc
// volume_rule) at the hit's position and its normal faced to the ray; where that covers the hit, E cut at zero goes to the
// lookup's VALUE and 1 to its COVERED — the arrays the fold reads —, else COVERED is 0 and the fold takes unbound_irradiance.
// Compiled in a translation unit of its own (kernels_probe_volume_views.hip, inside namespace rptvolumeviews).

__global__ void __launch_bounds__(256) rpt_views_probe_lit_merge(uint32_t m, Volume v, Merge g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  if (g.object[i] < 0) return;                    // a miss: the fold reads neither array
  if (g.lightmaps && g.covered[i] != 0) return;   // a lightmap covers the hit
  const D3 nrm = ld3(g.normal + 3ull * i), dir = ld3(g.dirs + 3ull * i);
  const double d = (nrm.x * dir.x + nrm.y * dir.y) + nrm.z * dir.z;
  const D3 N = d > 0.0 ? mk(-nrm.x, -nrm.y, -nrm.z) : nrm;
  const Lit r = volume_rule(v, ld3(g.position + 3ull * i), N);
  g.covered[i] = r.covered ? 1 : 0;
  if (r.covered) {
    double* __restrict__ o = g.value + 3ull * i;
    o[0] = r.e0 < 0.0 ? 0.0 : r.e0; o[1] = r.e1 < 0.0 ? 0.0 : r.e1; o[2] = r.e2 < 0.0 ? 0.0 : r.e2;
  }
}

#ifndef __HIP_DEVICE_COMPILE__
hipError_t merge(hipStream_t st, uint32_t m, const rptvolume::Volume& v, const Merge& g) {
  hipLaunchKernelGGL(rpt_views_probe_lit_merge, dim3((m + 255u) / 256u), dim3(256), 0, st, m, v, g);
  return hipGetLastError();
}
#endif
