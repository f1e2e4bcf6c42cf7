/*
 * rpt_gpu_views_denoised.h — a denoised frame per view for the batches of views of rpt_gpu.h: rptgpu_render_views_denoised and
 * its _device form.  Part of rpt_gpu.h, which includes this file behind its own declarations (RptView, RptViewQuery,
 * RptDenoise): include rpt_gpu.h, not this file.  The two entry points are additions within ABI version 7 and OPTIONAL — a
 * binding detects them by symbol (dlsym "rptgpu_render_views_denoised") and a library without them is still ABI 7 —, which is
 * why they stand in a file of their own, as rpt_gpu_views_seeded.h does.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_VIEWS_DENOISED_H
#define RPT_GPU_VIEWS_DENOISED_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_views_denoised.h behind the declarations this file needs"
#endif

/* A DENOISED FRAME PER VIEW in one call: what a caller of rptgpu_render_views had to build per view from a device Buffer —
 * `batches` calls of rptgpu_buffer_sample, rptgpu_buffer_features, rptgpu_buffer_denoise — over the whole batch of views in
 * shared passes and one filter launch per step.  There is NO NEW ARITHMETIC here: every value is defined by
 * text that already stands in rpt_gpu.h.
 *   BATCHES.  View v has the seed s_v = seeds[v], or with seeds == NULL q->seed + v*q->seed_stride (wrapping in 64 bits).
 *     Batch b = 0 .. batches-1 of view v is x_b[v][p] = the frame rptgpu_render_views_seeded gives view v under s_v with
 *     iterations = q->iterations and sample_index_base = q->sample_index_base + b*q->iterations (q->exposure_value
 *     included) — for a perspective view rptgpu_render_batch's frame, which is the batch rptgpu_buffer_sample accumulates:
 *     the Buffer's batch value and a view's frame are the same expressions.
 *   PER-PIXEL STATE.  total_p = the sum of x_b[v][p] over b ascending from +0.0, per component; n_p = batches; (m, M2) = the
 *     Welford state of RptAdaptive's comment after those batches in that order — the sequence rpt_buffer_accumulate runs.
 *   FEATURES.  rptgpu_render_views_aov_seeded's sums and hits for the same views and seeds with iterations =
 *     feature_iterations, sample_index_base = feature_sample_index_base and the channels DEPTH | NORMAL | ALBEDO | POSITION.
 *   THE FILTER of rpt_gpu.h (rptgpu_buffer_denoise's comment) with these inputs, applied to EACH VIEW ON ITS OWN: "the
 *     frame" is the view's own width x height pixels, a tap outside it is skipped.  A view's outputs depend on that view,
 *     its seed, the query, the RptViewDenoise and the scene and on nothing else: not on the other views, their order, the
 *     pieces or the passes.
 *   OUTPUTS, each [n_views][height][width](x 3), v in the order of `views`:
 *     denoised = the last level's c';  rgb8 = color_bytes of it through the thresholds rptgpu_buffer_image uses;
 *     mean = c_p = total_p / n per component (the unfiltered frame);  variance = u_p = (M2_p / (n - 1.0)) / n (the
 *     unfiltered variance of that mean).  Any of the four may be NULL, but not both denoised and rgb8.
 *   CONSEQUENCE.  An RPT_VIEW_PERSPECTIVE view's `denoised` frame is, bit for bit, what a Buffer of width x height on the
 *     same handle returns from rptgpu_buffer_denoise (out_linear; rgb8 likewise out_rgb8) after `batches` calls of
 *     rptgpu_buffer_sample with the view's camera, seed s_v and the sample bases above, and one call of
 *     rptgpu_buffer_features with feature_iterations and feature_sample_index_base.
 * The renders run the wavefront pipeline as rptgpu_render_views does (pieces, passes, flags, RPTGPU_VIEWS_PIECE); RptStats
 * advances as `batches` calls of rptgpu_render_views would.  The working set lives on the handle and grows on demand:
 * per (view, pixel) 60 B of state (total, mean, M2, count), 24 B of a batch's frame, 84 B of feature sums and 145 B of
 * filter columns (18 f64 and the hit flag) — 313 B, and for the host form 24 + 3 + 24 + 8 B per requested output;
 * an allocation that fails is RPTGPU_E_OUT_OF_MEMORY as rptgpu_render_views reports it.
 * RPTGPU_E_INVALID_ARGUMENT, before any device work, with a detail naming the reason and the output arrays untouched:
 * everything rptgpu_render_views refuses (RPT_FLAG_PERSISTENT included); a NULL RptViewDenoise, a wrong struct_size,
 * batches < 2, feature_iterations == 0, an embedded RptDenoise that rptgpu_buffer_denoise refuses (its own struct_size,
 * levels outside 1..8, a sigma that is not finite or not > 0); a NULL RptViewDenoiseOut or a wrong struct_size; denoised and
 * rgb8 both NULL; n_views * width * height > 2^32 - 1 (the accumulation indexes the batch in 32 bits); a sample range
 * (sample_index_base + batches * iterations, or feature_sample_index_base + feature_iterations) that does not fit 64 bits.
 * n_views == 0 returns RPTGPU_OK.  There is no CPU fallback. */
typedef struct RptViewDenoise {
  uint32_t struct_size;               /* sizeof(RptViewDenoise) */
  uint32_t batches;                   /* >= 2: renders of q->iterations samples per pixel each */
  uint32_t feature_iterations;        /* > 0: first-hit samples per pixel behind the features */
  uint32_t _pad;                      /* reserved: write 0; not read */
  uint64_t feature_sample_index_base; /* index of every pixel's first feature sample */
  RptDenoise filter;                  /* struct_size, levels 1..8 and the four sigmas, as for rptgpu_buffer_denoise */
} RptViewDenoise;
typedef struct RptViewDenoiseOut {
  uint32_t struct_size; /* sizeof(RptViewDenoiseOut) */
  uint32_t _pad;        /* reserved: write 0; not read */
  double* denoised;     /* [n_views][height][width][3] or NULL */
  uint8_t* rgb8;        /* [n_views][height][width][3] or NULL */
  double* mean;         /* [n_views][height][width][3] or NULL */
  double* variance;     /* [n_views][height][width]    or NULL */
} RptViewDenoiseOut;
int rptgpu_render_views_denoised(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                 const uint64_t* seeds /* [n_views] host, or NULL: q->seed + v*q->seed_stride */,
                                 const RptViewDenoise* d, const RptViewDenoiseOut* out /* host arrays */);
/* The same into device arrays; `views`, `seeds`, q and both structs stay in host memory.  `stream` and the
 * synchronisation rule are rptgpu_trace_rays_device's. */
int rptgpu_render_views_denoised_device(rptgpu_scene* h, uint64_t n_views, const RptView* views /* host */,
                                        const RptViewQuery* q, const uint64_t* seeds /* [n_views] host, or NULL */,
                                        const RptViewDenoise* d, const RptViewDenoiseOut* d_out /* device arrays */,
                                        void* stream);

#endif /* RPT_GPU_VIEWS_DENOISED_H */
