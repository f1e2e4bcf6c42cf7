// kernels/paths_rays.inc — rpt_paths_rays: the persistent path kernel over a piece of the caller's rays or light probes
// (rptgpu_trace_rays / rptgpu_bake_probes under RPT_FLAG_RAYS_PERSISTENT, DESIGN.md §13.1 and §14.1).  The loop is
// paths_loop.inc's, the text rpt_paths is compiled from; here are what only this form needs — where a work item's ray comes
// from —, its instantiations, and the two small kernels beside it: rpt_rays_ids and rpt_project_probes.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// a caller without stream ids: ray or probe i of its WHOLE array has stream i, so the piece's ids are id_base + i (the
// wavefront route lets rpt_raygen_rays / rpt_raygen_probes write them)
__global__ void __launch_bounds__(256) rpt_rays_ids(uint32_t id_base, uint32_t n, uint32_t* __restrict__ ids) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ids[i] = id_base + i;
}

// the ray of sample `smp` of the piece's index p_local, whose stream id is `id` (fr.pixels[p_local]); cr.kind is wave-uniform.
// Rays: rpt_raygen_rays' ray — origin and direction as the caller gave them, the stream (fr.seed, id, fr.sample_base + smp)
// standing at draw first_draw.  Probes: rpt_raygen_probes' ray — from the position along probe_direction's direction, drawn
// from the stream's draw 0 on; the path continues the stream behind those draws.  Everything is read here, at the fetch:
// nothing of the record lives across a query
RPT_DEV void caller_ray(const Frame& fr, const CallerRays& cr, uint32_t p_local, uint32_t id, uint32_t smp, D3& ro, D3& rd, Rng& rr) {
  if (cr.kind < 0) {
    ro = ld3(cr.origins + 3 * (uint64_t)p_local);
    rd = ld3(cr.dirs + 3 * (uint64_t)p_local);
    rr = rng_make(fr.seed, id, fr.sample_base + smp, cr.first_draw);
  } else {
    const D3 normal = cr.kind == (int32_t)RPT_PROBE_IRRADIANCE ? ld3(cr.dirs + 3 * (uint64_t)p_local) : mk(0, 0, 0);
    Rng rng = rng_make(fr.seed, id, fr.sample_base + smp, 0);
    rd = probe_direction((uint32_t)cr.kind, normal, rng);
    ro = ld3(cr.origins + 3 * (uint64_t)p_local);
    rr = rng;
  }
}

#define RPT_PATHS_FORM RPT_PATHS_FORM_RAYS
#include "paths_loop.inc"
#undef RPT_PATHS_FORM

// every instantiation paths_kernel() can pick (kernels/launch_paths.inc), as rpt_paths' own (kernels/buffer.inc)
template __global__ void rpt_paths_rays<KdLds, false>(Scene, Frame, CallerRays, PersistArgs);
template __global__ void rpt_paths_rays<KdFlat, false>(Scene, Frame, CallerRays, PersistArgs);
template __global__ void rpt_paths_rays<KdFlat, true>(Scene, Frame, CallerRays, PersistArgs);
#if RPT_FUSE_QUERY && RPT_RAY_STASH >= 2
template __global__ void rpt_paths_rays<KdFlat, false, true>(Scene, Frame, CallerRays, PersistArgs);
#if RPT_SCENE_CONSTS
template __global__ void rpt_paths_rays<KdFlat, false, true, true>(Scene, Frame, CallerRays, PersistArgs);
#endif
#endif
template __global__ void rpt_paths_rays<KdFlatG, false>(Scene, Frame, CallerRays, PersistArgs);
template __global__ void rpt_paths_rays<KdFlatG, true>(Scene, Frame, CallerRays, PersistArgs);
template __global__ void rpt_paths_rays<KdFlatF, false>(Scene, Frame, CallerRays, PersistArgs);
template __global__ void rpt_paths_rays<KdFlatF, true>(Scene, Frame, CallerRays, PersistArgs);

// rpt_sum_samples' step for light probes: one thread per probe of the piece, the launch's samples in ascending order.  L is
// the sample's radiance where rpt_paths_rays left it (lbuf, [spp][3][npix]); the sums are rpt_resolve_probes' (fr.accum, SoA
// over the piece, [27 or 3][npix], continued from the launch before) with ITS expressions in ITS order — IRRADIANCE: acc + L;
// SH9: acc + L.c * Y[j], the direction made again from the stream —, so a launch border falls where a pass border does
__global__ void __launch_bounds__(256) rpt_project_probes(Frame fr, const double* __restrict__ lbuf, uint32_t spp, uint32_t kind) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= fr.npix) return;
  const double* lb = lbuf + p;
  if (kind == RPT_PROBE_IRRADIANCE) {
    double* a = fr.accum + p; // (wf_state.inc's ld_soa3 / st_soa3 over [3][npix], written out: that file is the wavefront's)
    D3 acc = mk(a[0], a[fr.npix], a[2 * (uint64_t)fr.npix]);
    for (uint32_t s = 0; s < spp; s++) {
      acc = acc + mk(lb[0], lb[fr.npix], lb[2 * (uint64_t)fr.npix]);
      lb += 3 * (uint64_t)fr.npix;
    }
    a[0] = acc.x; a[fr.npix] = acc.y; a[2 * (uint64_t)fr.npix] = acc.z;
    return;
  }
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] = fr.accum[(uint64_t)k * fr.npix + p];
  const uint32_t id = fr.pixels[p];
  for (uint32_t s = 0; s < spp; s++) {
    const D3 L = mk(lb[0], lb[fr.npix], lb[2 * (uint64_t)fr.npix]);
    lb += 3 * (uint64_t)fr.npix;
    Rng rng = rng_make(fr.seed, id, fr.sample_base + s, 0);
    double Y[9];
    sh9_basis(probe_direction(RPT_PROBE_SH9, mk(0, 0, 0), rng), Y);
#pragma unroll
    for (int j = 0; j < 9; j++) {
      acc[3 * j] = acc[3 * j] + L.x * Y[j];
      acc[3 * j + 1] = acc[3 * j + 1] + L.y * Y[j];
      acc[3 * j + 2] = acc[3 * j + 2] + L.z * Y[j];
    }
  }
#pragma unroll
  for (int k = 0; k < 27; k++) fr.accum[(uint64_t)k * fr.npix + p] = acc[k];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the launchers the kernel tables point to (kernels.h)
#define RPT_PATHS_FORM RPT_PATHS_FORM_RAYS
#include "launch_paths.inc"
#undef RPT_PATHS_FORM
void launch_rays_ids(hipStream_t st, uint32_t id_base, uint32_t n, uint32_t* ids) {
  if (n) hipLaunchKernelGGL(rpt_rays_ids, dim3((n + 255u) / 256u), dim3(256), 0, st, id_base, n, ids);
}
void launch_project_probes(hipStream_t st, const Frame& fr, const double* lbuf, uint32_t spp, uint32_t kind) {
  hipLaunchKernelGGL(rpt_project_probes, dim3((fr.npix + 255u) / 256u), dim3(256), 0, st, fr, lbuf, spp, kind);
}
#endif // !__HIP_DEVICE_COMPILE__
