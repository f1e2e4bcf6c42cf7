/*
 * rpt_gpu_views_persistent.h — a batch of views in the persistent path kernel, on request: RPT_FLAG_VIEWS_PERSISTENT for
 * rptgpu_render_views, rptgpu_render_views_seeded and their _device forms.  Part of rpt_gpu.h, which includes this file
 * behind its own declarations: include rpt_gpu.h, not this file.  The flag is an addition within ABI version 7 and OPTIONAL:
 * a library without it IGNORES the bit and runs the wavefront pipeline, so a binding detects it by symbol (dlsym
 * "rptgpu_views_persistent_supported") before it relies on the route — a library without the symbol is still ABI 7.  The
 * conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_VIEWS_PERSISTENT_H
#define RPT_GPU_VIEWS_PERSISTENT_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_views_persistent.h behind the declarations this file needs"
#endif

/* RPT_FLAG_VIEWS_PERSISTENT in RptViewQuery::flags of rptgpu_render_views[_seeded][_device]: run the batch in the
 * persistent path kernel (the whole path in registers), as RPT_FLAG_PERSISTENT does for a render — on any scene a render accepts RPT_FLAG_PERSISTENT for: flat
 * scenes through the kernel's flat forms, others through its general one; a scene with a group that has mesh children, which
 * only the wavefront pipeline walks, ignores the request as it ignores a render's.  One launch per sample slice covers a
 * whole piece of the call's (view, pixel) indices, every view the piece holds.
 * THE SAME BITS: the frames are the ones the call gives without the flag — the same streams, the same draws, the same
 * fold; only the route differs.  Everything rptgpu_render_views promises holds: the three projections, the lens, seed and
 * seed_stride, a seed per view, host and device outputs in f64 and f32, any sample_index_base, the pieces and
 * RPTGPU_VIEWS_PIECE (a piece is also at most what the kernel's 32-bit work counter holds: about 2^32 / iterations
 * indices).  RptStats advances as for a render through that kernel: samples, the ray counts,
 * kernel_launches[RPT_K_PATHS] >= 1 — and no launch of the wavefront kinds.
 * WITHOUT the flag nothing changes: the wavefront pipeline stays the route, and RPT_FLAG_PERSISTENT in an RptViewQuery
 * stays refused.  Which route is faster depends on the scene (DESIGN.md §15.2 has the measurements).
 * RPTGPU_E_INVALID_ARGUMENT, before any device work and with the outputs untouched: the flag together with
 * RPT_FLAG_WAVEFRONT; the flag in a call of rptgpu_render_views_aov[_seeded][_device] or
 * rptgpu_render_views_denoised[_device], which have no such route.
 * (The constant stands with the other RPT_FLAG_* in rpt_gpu.h: RPT_FLAG_VIEWS_PERSISTENT = 16u.) */

/* 1: this library reads RPT_FLAG_VIEWS_PERSISTENT.  No handle, no device. */
int rptgpu_views_persistent_supported(void);

#endif /* RPT_GPU_VIEWS_PERSISTENT_H */
