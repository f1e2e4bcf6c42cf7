// api_views_denoise.cpp — rptgpu_render_views_denoised[_device]: a denoised frame per view of a batch in one call
// (include/rpt_gpu_views_denoised.h; see api_internal.h).  Nothing here computes a value of its own: per batch
// the views driver (api_views.cpp render_views) renders every view into one device frame and ONE rpt_buffer_accumulate launch
// over the flat (view, pixel) index space adds it to the Buffer's per-pixel state; then the views' feature driver
// (api_hits.cpp render_views_aov) fills the feature sums, and the Buffer's filter runs over the whole batch with one launch
// per step (kernels/denoise.inc with RPT_DN_VIEWS 1), each view inside its own frame.  The working set lives on the handle
// (rptplan::views_denoise_plan has its bytes) and grows on demand.
#include "api_internal.h"

namespace rptapi {
namespace {

// what is wrong with an RptViewDenoise / an RptViewDenoiseOut (nullptr: nothing)
const char* bad_view_denoise(const RptViewDenoise* d) {
  if (!d) return "null RptViewDenoise";
  if (d->struct_size != sizeof(RptViewDenoise)) return "RptViewDenoise: struct_size is not sizeof(RptViewDenoise)";
  if (d->batches < 2) return "RptViewDenoise: batches < 2 (there is no variance of one batch)";
  if (!d->feature_iterations) return "RptViewDenoise: feature_iterations == 0";
  return bad_denoise(&d->filter);
}
const char* bad_view_denoise_out(const RptViewDenoiseOut* o) {
  if (!o) return "null RptViewDenoiseOut";
  if (o->struct_size != sizeof(RptViewDenoiseOut)) return "RptViewDenoiseOut: struct_size is not sizeof(RptViewDenoiseOut)";
  if (!o->denoised && !o->rgb8) return "RptViewDenoiseOut: denoised and rgb8 are both NULL";
  return nullptr;
}

// out's arrays: host memory, or — on_device — device memory (user_stream: the stream their producer ran on); views, seeds
// and the structs are host memory either way
int render_views_denoised(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q, const uint64_t* seeds,
                          const RptViewDenoise* d, const RptViewDenoiseOut* out, bool on_device, hipStream_t user_stream) {
  // (the query, the two structs, then the views: each is refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_view_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_view_denoise(d)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_view_denoise_out(out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n_views && !views) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  const uint64_t npix = (uint64_t)q->width * q->height;
  if (n_views > (1ull << 58) / npix) // (rptgpu_render_views' own bound and words)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "n_views * width * height does not fit: the frames would not fit any memory");
  const rptplan::ViewsDenoisePlan plan =
      rptplan::views_denoise_plan(n_views, npix, !on_device, out->denoised != nullptr, out->rgb8 != nullptr, out->mean != nullptr,
                                  out->variance != nullptr);
  if (n_views && !plan.n)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "n_views * width * height > 2^32 - 1: the batches are accumulated over 32-bit indices");
  if (!rptplan::sample_range_fits(q->sample_index_base, (uint64_t)d->batches * q->iterations))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "sample_index_base + batches * iterations does not fit 64 bits");
  if (!rptplan::sample_range_fits(d->feature_sample_index_base, d->feature_iterations))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "feature_sample_index_base + feature_iterations does not fit 64 bits");
  for (uint64_t v = 0; v < n_views; v++)
    if (const char* why = bad_view(views[v], *q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n_views) return RPTGPU_OK;

  const uint64_t n = plan.n;
  hipStream_t st = h->stream;
  const KernelTable* kt = table_for(q->precision_mode, h->ext_shapes);
  const bool seeded = seeds != nullptr;
  // the working set and the state's start: every sum at +0.0, every count at 0
  int rc = guarded(h, h->device, [&]() -> int {
    if (user_stream) HIP_TRY(hipStreamSynchronize(user_stream));
    if (!h->vd_thr.p) {
      bool clean = true;
      const std::vector<double> thr = byte_thresholds(clean);
      if (!clean) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "host pow() is not monotone around a u8 threshold");
      h->vd_thr.upload(thr, st);
      HIP_TRY(hipStreamSynchronize(st)); // (thr is this frame's)
    }
    h->vd_total.alloc(3 * n); h->vd_mean.alloc(3 * n); h->vd_m2.alloc(n); h->vd_counts.alloc(n);
    h->vd_stage.alloc(3 * n);
    h->vd_cols.alloc(18 * n); h->vd_hit.alloc(n);
    if (!on_device) {
      if (out->denoised) h->vd_linear.alloc(3 * n);
      if (out->rgb8) h->vd_rgb8.alloc(3 * n);
      if (out->mean) h->vd_out_mean.alloc(3 * n);
      if (out->variance) h->vd_out_var.alloc(n);
    }
    HIP_TRY(hipMemsetAsync(h->vd_total.p, 0, 3 * n * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(h->vd_mean.p, 0, 3 * n * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(h->vd_m2.p, 0, n * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(h->vd_counts.p, 0, n * sizeof(uint32_t), st));
    return RPTGPU_OK;
  });
  if (rc != RPTGPU_OK) return rc;

  // the batches: rptgpu_render_views[_seeded]_device into the staging frame, then the Buffer's accumulation over all views
  for (uint32_t b = 0; b < d->batches; b++) {
    RptViewQuery qb = *q;
    qb.sample_index_base = q->sample_index_base + (uint64_t)b * q->iterations;
    rc = render_views(h, n_views, views, &qb, seeded, seeds, h->vd_stage.p, true, false, nullptr);
    if (rc != RPTGPU_OK) return rc;
    rc = guarded(h, h->device, [&]() -> int {
      kt->buffer_accumulate(st, h->vd_total.p, h->vd_stage.p, nullptr, nullptr, (uint32_t)n, h->vd_counts.p, h->vd_mean.p, h->vd_m2.p);
      HIP_TRY(hipGetLastError());
      return RPTGPU_OK;
    });
    if (rc != RPTGPU_OK) return rc;
  }

  // the features: rptgpu_render_views_aov[_seeded]_device into the handle's arrays
  rptdev::AovOut feat{};
  rc = guarded(h, h->device, [&]() -> int {
    feat = aov_arrays(h->vd_feat, st, n, FEATURE_CHANNELS);
    return RPTGPU_OK;
  });
  if (rc != RPTGPU_OK) return rc;
  {
    RptViewQuery qf = *q;
    qf.iterations = d->feature_iterations;
    qf.sample_index_base = d->feature_sample_index_base;
    RptAovBuffers fb{};
    fb.struct_size = sizeof(RptAovBuffers); fb.channels = FEATURE_CHANNELS;
    fb.hits = feat.hits; fb.depth = feat.depth; fb.normal = feat.normal; fb.albedo = feat.albedo; fb.position = feat.position;
    rc = render_views_aov(h, n_views, views, &qf, seeded, seeds, &fb, true, nullptr);
    if (rc != RPTGPU_OK) return rc;
  }

  // the filter, as rptgpu_buffer_denoise runs it, one launch per step for the whole batch
  return guarded(h, h->device, [&]() -> int {
    double* col = h->vd_cols.p;
    double *c[2] = {col, col + 4 * n}, *v[2] = {col + 3 * n, col + 7 * n};
    double *g_normal = col + 8 * n, *g_position = col + 11 * n, *g_albedo = col + 14 * n, *g_depth = col + 17 * n;
    kt->denoise_views_prepare(st, h->vd_total.p, h->vd_counts.p, h->vd_m2.p, feat, q->width, q->height, n_views, n, c[0], v[0],
                              g_normal, g_position, g_albedo, g_depth, h->vd_hit.p);
    rptdev::DenoiseGuide g{};
    g.normal = g_normal; g.position = g_position; g.albedo = g_albedo; g.depth = g_depth; g.hit = h->vd_hit.p;
    g.stride = n; g.width = q->width; g.height = q->height;
    const RptDenoise& f = d->filter;
    rptdev::DenoiseSigmas sg{};
    sg.color2 = f.sigma_color * f.sigma_color; sg.normal = f.sigma_normal; sg.depth = f.sigma_depth;
    sg.albedo2 = f.sigma_albedo * f.sigma_albedo;
    int cur = 0;
    for (uint32_t l = 0; l < f.levels; l++, cur ^= 1)
      kt->denoise_views_level(st, g, n_views, c[cur], v[cur], c[cur ^ 1], v[cur ^ 1], 1u << l, sg);
    RptViewDenoiseOut o = *out; // where the kernel writes: the caller's device arrays, or the staging of a host caller's
    if (!on_device) {
      o.denoised = out->denoised ? h->vd_linear.p : nullptr;
      o.rgb8 = out->rgb8 ? h->vd_rgb8.p : nullptr;
      o.mean = out->mean ? h->vd_out_mean.p : nullptr;
      o.variance = out->variance ? h->vd_out_var.p : nullptr;
    }
    kt->denoise_views_finish(st, c[cur], n, n, h->vd_thr.p, o.denoised, o.rgb8, h->vd_total.p, h->vd_counts.p, h->vd_m2.p, o.mean,
                             o.variance);
    HIP_TRY(hipGetLastError());
    if (!on_device) {
      if (out->denoised) HIP_TRY(hipMemcpyAsync(out->denoised, o.denoised, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
      if (out->rgb8) HIP_TRY(hipMemcpyAsync(out->rgb8, o.rgb8, 3 * n, hipMemcpyDeviceToHost, st));
      if (out->mean) HIP_TRY(hipMemcpyAsync(out->mean, o.mean, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
      if (out->variance) HIP_TRY(hipMemcpyAsync(out->variance, o.variance, n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return RPTGPU_OK;
  });
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_render_views_denoised(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                 const uint64_t* seeds, const RptViewDenoise* d, const RptViewDenoiseOut* out) {
  return render_views_denoised(h, n_views, views, q, seeds, d, out, false, nullptr);
}

int rptgpu_render_views_denoised_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                        const uint64_t* seeds, const RptViewDenoise* d, const RptViewDenoiseOut* d_out,
                                        void* stream) {
  return render_views_denoised(h, n_views, views, q, seeds, d, d_out, true, (hipStream_t)stream);
}

} // extern "C"
