/*
 * rpt_gpu_vertices_persistent.h — path vertices from the persistent path kernel, on request: RPT_FLAG_VERTICES_PERSISTENT for
 * rptgpu_trace_vertices and its _device form.  Part of rpt_gpu.h, which includes this file behind its own declarations:
 * include rpt_gpu.h, not this file.  The flag is an addition within ABI version 7 and OPTIONAL: a library without it IGNORES
 * the bit and runs the wavefront pipeline, so a binding detects it by symbol (dlsym "rptgpu_vertices_persistent_supported")
 * before it relies on the route — a library without the symbol is still ABI 7.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_VERTICES_PERSISTENT_H
#define RPT_GPU_VERTICES_PERSISTENT_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_vertices_persistent.h behind the declarations this file needs"
#endif

/* RPT_FLAG_VERTICES_PERSISTENT in RptVertexQuery::flags of rptgpu_trace_vertices[_device]: run the call's paths in the
 * persistent path kernel (the whole path in registers), as RPT_FLAG_RAYS_PERSISTENT does for rptgpu_trace_rays — on any scene
 * a render accepts RPT_FLAG_PERSISTENT for: flat scenes through the kernel's flat forms, others through its general one; a
 * scene with a group that has tree children, which only the wavefront pipeline walks, ignores the request as it ignores a
 * render's.  The kernel writes every value of a vertex where it has it in a register — the hit behind its closest-hit
 * query, the radiance and the three factors where the depth's record is made, the last vertex's radiance and the length
 * where the path ends —, so no second pass reads the paths back.
 * THE SAME BYTES: every named array — LENGTH, the ten per-vertex channels with the filler behind each path's last vertex,
 * RGB — holds what the call writes without the flag; a channel that is not named is not computed, its pointer is not read
 * and its array is not written.  Everything rptgpu_trace_vertices promises holds: streams given or NULL, any first_draw and
 * any sample_index_base (across 2^32 too), exposure_value, host and device arrays with the device form's stream rule, the
 * pieces and RPTGPU_VERTICES_PIECE (a piece is also at most what the kernel's 32-bit work counter holds: about 2^32 /
 * iterations rays), RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS, live updates.  RptStats advances as for
 * rptgpu_trace_rays under RPT_FLAG_RAYS_PERSISTENT: samples = n * iterations, the ray counts,
 * kernel_launches[RPT_K_PATHS] >= 1 — and no launch of the wavefront kinds.  There is no CPU fallback.
 * WITHOUT the flag nothing changes: the wavefront pipeline stays the route, and RPT_FLAG_PERSISTENT and
 * RPT_FLAG_RAYS_PERSISTENT in an RptVertexQuery stay refused, whatever stands beside them.  Which route is faster depends
 * on the scene and the channels (DESIGN.md §19.1 has the measurements).
 * RPTGPU_E_INVALID_ARGUMENT, before any device work and with the arrays untouched: the flag together with
 * RPT_FLAG_WAVEFRONT.  No other call reads the bit.
 * (The constant stands with the other RPT_FLAG_* in rpt_gpu.h: RPT_FLAG_VERTICES_PERSISTENT = 64u.) */

/* 1: this library reads RPT_FLAG_VERTICES_PERSISTENT.  No handle, no device. */
int rptgpu_vertices_persistent_supported(void);

#endif /* RPT_GPU_VERTICES_PERSISTENT_H */
