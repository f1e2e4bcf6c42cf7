/*
 * rpt_gpu_views_seeded.h — a seed per view for the batches of views of rpt_gpu.h: rptgpu_render_views_seeded,
 * rptgpu_render_views_aov_seeded and their _device forms.  Part of rpt_gpu.h, which includes this file behind its own
 * declarations (RptView, RptViewQuery, RptAovBuffers): include rpt_gpu.h, not this file.  The four entry points are
 * additions within ABI version 7 and OPTIONAL — a binding detects them by symbol (dlsym "rptgpu_render_views_seeded")
 * and a library without them is still ABI 7 —, which is why they stand in a file of their own: rpt_gpu.h's own text lists the
 * entry points every ABI-7 library exports.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_VIEWS_SEEDED_H
#define RPT_GPU_VIEWS_SEEDED_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_views_seeded.h behind the declarations this file needs"
#endif

/* A SEED PER VIEW: resuming a data set, rendering view 731 of an earlier job again, seeds from the caller's own generator.
 * View v is rendered EXACTLY as rptgpu_render_views renders it with q->seed = seeds[v] and seed_stride = 0: sample s of
 * pixel p draws from the stream keyed by seeds[v] with the counter (p, sample_index_base + s, draw block), from draw 0 on.
 * q->seed and q->seed_stride are not read.  Equal seeds in different views are allowed.  A view's pixels depend on that
 * view, its seed, the query and the scene and on nothing else: not on the other views, their seeds, their order, the
 * pieces or the passes; a perspective view is rptgpu_render_batch of its camera with seed = seeds[v], bit for bit.
 * rptgpu_render_views with seed_stride != 0 IS this call with seeds[v] = seed + v*seed_stride (wrapping in 64 bits), formed
 * on the host.  Everything else — layout, rays, pieces, flags, RptStats, what is not in scope — is rptgpu_render_views'.
 * RPTGPU_E_INVALID_ARGUMENT, before any device work and with `out` untouched: everything rptgpu_render_views refuses
 * (RPT_FLAG_PERSISTENT included), and NULL seeds with n_views > 0.  n_views == 0 returns RPTGPU_OK. */
int rptgpu_render_views_seeded(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                               const uint64_t* seeds /* [n_views], host */,
                               double* out /* [n_views][height][width][3], host */);
/* The same into device memory, as rptgpu_render_views_device; `views` and `seeds` stay in host memory. */
int rptgpu_render_views_seeded_device(rptgpu_scene* h, uint64_t n_views, const RptView* views /* host */,
                                      const RptViewQuery* q, const uint64_t* seeds /* [n_views], host */, void* d_out,
                                      int out_is_f32, void* stream);

/* A SEED PER VIEW for rptgpu_render_views_aov, as rptgpu_render_views_seeded: view v's buffers are EXACTLY those
 * rptgpu_render_views_aov gives it with q->seed = seeds[v] and seed_stride = 0 — under RPT_VIEW_PERSPECTIVE
 * rptgpu_render_aov of its camera with seed = seeds[v], bit for bit.  q->seed and q->seed_stride are not read; equal seeds
 * are allowed; a view's buffers depend on that view, its seed, the query and the scene and on nothing else.
 * rptgpu_render_views_aov with seed_stride != 0 IS this call with seeds[v] = seed + v*seed_stride (wrapping in 64 bits).
 * RPTGPU_E_INVALID_ARGUMENT, before any device work and with the arrays untouched: everything rptgpu_render_views_aov
 * refuses (RPT_FLAG_PERSISTENT included), and NULL seeds with n_views > 0.  n_views == 0 returns RPTGPU_OK. */
int rptgpu_render_views_aov_seeded(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                   const uint64_t* seeds /* [n_views], host */,
                                   const RptAovBuffers* out /* host arrays, [n_views][height][width](x 3) */);
/* The same into device arrays, as rptgpu_render_views_aov_device; `views`, `seeds`, q and the struct stay in host memory. */
int rptgpu_render_views_aov_seeded_device(rptgpu_scene* h, uint64_t n_views, const RptView* views /* host */,
                                          const RptViewQuery* q, const uint64_t* seeds /* [n_views], host */,
                                          const RptAovBuffers* d_out /* device arrays */, void* stream);

#endif /* RPT_GPU_VIEWS_SEEDED_H */
