/*
 * rpt_gpu_rays_persistent.h — caller-supplied rays and light probes in the persistent path kernel, on request:
 * RPT_FLAG_RAYS_PERSISTENT for rptgpu_trace_rays, rptgpu_bake_probes and their _device forms.  Part of rpt_gpu.h, which
 * includes this file behind its own declarations: include rpt_gpu.h, not this file.  The flag is an addition within ABI
 * version 7 and OPTIONAL: a library without it IGNORES the bit and runs the wavefront pipeline, so a binding detects it by
 * symbol (dlsym "rptgpu_rays_persistent_supported") before it relies on the route — a library without the symbol is still
 * ABI 7.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_RAYS_PERSISTENT_H
#define RPT_GPU_RAYS_PERSISTENT_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_rays_persistent.h behind the declarations this file needs"
#endif

/* RPT_FLAG_RAYS_PERSISTENT in RptRayQuery::flags of rptgpu_trace_rays[_device] and in RptProbeQuery::flags of
 * rptgpu_bake_probes[_device]: run the call's paths in the persistent path kernel (the whole path in registers), as
 * RPT_FLAG_PERSISTENT does for a render — on any scene a render accepts RPT_FLAG_PERSISTENT for: flat scenes through the
 * kernel's flat forms, others through its general one; a scene with a group that has tree children, which only the
 * wavefront pipeline walks, ignores the request as it ignores a render's.  One launch per sample slice covers a whole
 * piece of the call's rays or probes; a ray is read, and a probe's direction drawn, where the kernel hands out its work.
 * THE SAME BITS: the radiance, the SH9 coefficients and the irradiance are the ones the call gives without the flag — the
 * same streams, the same draws, the same fold and the same order of sums; only the route differs.  Everything those calls
 * promise holds: streams given or NULL, any first_draw and any sample_index_base (across 2^32 too), exposure_value, both
 * probe kinds, host and device arrays with the device forms' stream rule, the pieces and their RPTGPU_RAYS_PIECE /
 * RPTGPU_PROBES_PIECE overrides (a piece is also at most what the kernel's 32-bit work counter holds: about 2^32 /
 * iterations rays or probes), RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS.  RptStats advances as for a render
 * through that kernel: samples, the ray counts, kernel_launches[RPT_K_PATHS] >= 1 — and no launch of the wavefront kinds.
 * WITHOUT the flag nothing changes: the wavefront pipeline stays the route, and RPT_FLAG_PERSISTENT in an RptRayQuery or
 * an RptProbeQuery stays refused.  Which route is faster depends on the scene and on how coherent the rays are (DESIGN.md
 * §13.1 and §14.1 have the measurements).
 * RPTGPU_E_INVALID_ARGUMENT, before any device work and with the arrays untouched: the flag together with
 * RPT_FLAG_WAVEFRONT; the flag in a call of rptgpu_trace_vertices[_device], which has a flag of its own
 * (RPT_FLAG_VERTICES_PERSISTENT, rpt_gpu_vertices_persistent.h).  No other call reads
 * the bit.
 * (The constant stands with the other RPT_FLAG_* in rpt_gpu.h: RPT_FLAG_RAYS_PERSISTENT = 32u.) */

/* 1: this library reads RPT_FLAG_RAYS_PERSISTENT.  No handle, no device. */
int rptgpu_rays_persistent_supported(void);

#endif /* RPT_GPU_RAYS_PERSISTENT_H */
