// api_buffer.cpp — the device-resident Buffer (buffer.rs:9-93 on the device: add_samples, add_sample by adaptive rounds,
// image, variance; see api_internal.h), the first-hit features it can hold and the filter they guide
#include "api_internal.h"

// ------------------------------------------------------------------ device-resident Buffer
struct rptgpu_buffer {
  rptgpu_scene* h = nullptr;
  uint32_t width = 0, height = 0, radius = 0;
  std::vector<DevBuf<double>> batches; // one W*H*3 frame per batch, on the device (zero where a round did not sample a pixel)
  DevBuf<double> total, thr, pix_var;
  DevBuf<const double*> batch_ptrs;
  DevBuf<uint8_t> image;
  // per pixel: n_p, the batches it holds, and the Welford state of their values (mean m_p, M2_p): DESIGN.md §10
  DevBuf<uint32_t> counts;
  DevBuf<double> mean, m2;
  // adaptive rounds: the active pixels (active[cur], n_active of them, in the order of the round-0 list), the list the
  // next round compacts into, the compaction's scratch and the round's packed values
  DevBuf<uint32_t> active[2], block_cnt, active_n;
  DevBuf<uint8_t> keep;
  DevBuf<double> packed;
  int cur = 0;
  uint32_t n_active = 0;
  bool listed = false;  // active[cur] has been made (by the first adaptive round)
  bool retired = false; // some pixel has retired: a full-frame batch would break the prefix property
  // rptgpu_buffer_features: the sums rptgpu_render_aov would return (depth, normal, albedo, position; hits), kept here
  DevBuf<double> feat_arrays;
  rptdev::AovOut feat{};
  bool has_features = false;
  // rptgpu_buffer_denoise's working set: 18 f64 columns of width*height (colour + variance twice, normal, position,
  // albedo, depth), the hit flags, and the outputs before they are copied to the host
  DevBuf<double> dn_cols, dn_linear;
  DevBuf<uint8_t> dn_hit, dn_rgb8;

  ~rptgpu_buffer() {
    if (h) (void)hipSetDevice(h->device);
    // every DevBuf frees itself (after this body, on the handle's device)
  }
};

namespace rptapi {
// color_bytes (color.rs:18-24) as the host computes it; the device reproduces it from thresholds
static inline int color_byte_host(double v) {
  double t = std::pow(std::fmin(std::fmax(v, 0.0), 1.0), 1.0 / 2.2) * 255.0;
  return !(t > 0.0) ? 0 : (t >= 255.0 ? 255 : (int)t);
}
// smallest v in [0,1] with color_byte_host(v) >= k, by bisection over the doubles; `clean` reports
// whether the conversion is a step function in a window of +-256 ulps around every threshold
std::vector<double> byte_thresholds(bool& clean) {
  std::vector<double> thr(256, 0.0);
  clean = true;
  for (int k = 1; k < 256; k++) {
    uint64_t lo = 0, hi;
    double one = 1.0;
    std::memcpy(&hi, &one, 8); // positive doubles order like their bit patterns
    while (lo < hi) {
      uint64_t mid = lo + (hi - lo) / 2;
      double v;
      std::memcpy(&v, &mid, 8);
      if (color_byte_host(v) >= k) hi = mid;
      else lo = mid + 1;
    }
    std::memcpy(&thr[k], &lo, 8);
    for (int d = -256; d <= 256; d++) {
      uint64_t u = lo + (uint64_t)(int64_t)d;
      double v;
      std::memcpy(&v, &u, 8);
      if (v >= 0.0 && v <= 1.0 && (color_byte_host(v) >= k) != (d >= 0)) clean = false;
    }
  }
  return thr;
}
// what is wrong with an RptAdaptive (nullptr: nothing)
static const char* bad_adaptive(const RptAdaptive* a) {
  if (!a) return "null RptAdaptive";
  if (a->struct_size != sizeof(RptAdaptive)) return "RptAdaptive: struct_size is not sizeof(RptAdaptive)";
  if (a->min_batches < 2) return "RptAdaptive: min_batches < 2";
  if (!(std::isfinite(a->abs_tol) && a->abs_tol >= 0.0) || !(std::isfinite(a->rel_tol) && a->rel_tol >= 0.0))
    return "RptAdaptive: abs_tol and rel_tol must be finite and >= 0";
  return nullptr;
}
// what is wrong with an RptDenoise (nullptr: nothing)
const char* bad_denoise(const RptDenoise* d) {
  if (!d) return "null RptDenoise";
  if (d->struct_size != sizeof(RptDenoise)) return "RptDenoise: struct_size is not sizeof(RptDenoise)";
  if (d->levels < 1 || d->levels > 8) return "RptDenoise: levels outside 1..8";
  for (double s : {d->sigma_color, d->sigma_normal, d->sigma_depth, d->sigma_albedo})
    if (!(std::isfinite(s) && s > 0.0)) return "RptDenoise: every sigma must be finite and > 0";
  return nullptr;
}
} // namespace rptapi

extern "C" {

int rptgpu_buffer_create(rptgpu_scene* h, uint32_t width, uint32_t height, uint32_t filter_radius, rptgpu_buffer** out) {
  if (!h || !out || !width || !height) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "bad argument");
  *out = nullptr;
  rptgpu_buffer* b = new (std::nothrow) rptgpu_buffer();
  if (!b) return fail(h, RPTGPU_E_OUT_OF_MEMORY, "host allocation failed");
  b->h = h; b->width = width; b->height = height; b->radius = filter_radius;
  const int rc = guarded(h, h->device, [&]() -> int {
    bool clean = true;
    std::vector<double> thr = byte_thresholds(clean);
    if (!clean) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "host pow() is not monotone around a u8 threshold");
    b->thr.upload(thr, h->stream);
    uint64_t npix = (uint64_t)width * height, n = npix * 3;
    b->total.alloc(n);
    HIP_TRY(hipMemsetAsync(b->total.p, 0, n * sizeof(double), h->stream));
    b->counts.alloc(npix); b->mean.alloc(n); b->m2.alloc(npix);
    HIP_TRY(hipMemsetAsync(b->counts.p, 0, npix * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(b->mean.p, 0, n * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(b->m2.p, 0, npix * sizeof(double), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RPTGPU_OK;
  });
  if (rc != RPTGPU_OK) {
    delete b;
    return rc;
  }
  *out = b;
  return RPTGPU_OK;
}

void rptgpu_buffer_destroy(rptgpu_buffer* b) { delete b; }

int rptgpu_buffer_sample(rptgpu_buffer* b, const RptCamera* camera, const RptRenderParams* params) {
  if (!b || !camera || !params) return RPTGPU_E_INVALID_ARGUMENT;
  rptgpu_scene* h = b->h;
  if (params->width != b->width || params->height != b->height)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "Invalid sample dimension"); // buffer.rs:33-36
  if (b->retired)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "a pixel of this buffer has retired (rptgpu_buffer_sample_adaptive): a "
                                              "full-frame batch would give it a batch its earlier rounds skipped");
  DevBuf<double> frame; // the batch's: the buffer's once it is accumulated
  const uint64_t n = (uint64_t)b->width * b->height * 3;
  if (hipSetDevice(h->device) != hipSuccess || hipMalloc((void**)&frame.p, n * sizeof(double)) != hipSuccess)
    return fail(h, RPTGPU_E_OUT_OF_MEMORY, "hipMalloc of a batch frame failed");
  frame.n = n;
  const int rc = render_impl(h, camera, params, frame.p, false, nullptr, nullptr);
  if (rc != RPTGPU_OK) return rc;
  return guarded(h, h->device, [&]() -> int {
    table_for(RPT_PRECISION_F64_STRICT)->buffer_accumulate(h->stream, b->total.p, frame.p, nullptr, nullptr, b->width * b->height,
                                                           b->counts.p, b->mean.p, b->m2.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    b->batches.push_back(std::move(frame));
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_sample_adaptive(rptgpu_buffer* b, const RptCamera* camera, const RptRenderParams* params,
                                  const RptAdaptive* a, uint32_t* out_active) {
  rptgpu_scene* h = b ? b->h : nullptr;
  if (const char* why = bad_adaptive(a)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!b || !camera || !params || !out_active) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (params->width != b->width || params->height != b->height)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "Invalid sample dimension"); // buffer.rs:33-36
  if (params->part_count > 1)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "part_count > 1: adaptive rounds render the whole frame on one device");
  if (const char* why = bad_params(params)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  REFUSE_IF_ABANDONED(h);
  const uint32_t npix = b->width * b->height;
  hipStream_t st = h->stream;
  const KernelTable* kt = table_for(RPT_PRECISION_F64_STRICT);
  DevBuf<double> frame; // the round's, zero where it samples no pixel: the buffer's once it is accumulated
  int rc = guarded(h, h->device, [&]() -> int {
    if (!b->listed) { // round 0: every pixel, in the 8x8-block order of a full-frame render
      b->active[0].upload(pixel_list(b->width, b->height, 32, 8, 0, 1), st);
      b->active[1].alloc(npix);
      b->keep.alloc(npix);
      b->block_cnt.alloc((npix + RPT_RETIRE_TILE - 1) / RPT_RETIRE_TILE);
      b->active_n.alloc(1);
      HIP_TRY(hipStreamSynchronize(st));
      b->cur = 0;
      b->n_active = npix;
      b->listed = true;
    }
    if (b->n_active) {
      b->packed.alloc((uint64_t)b->n_active * 3);
      frame.alloc((uint64_t)npix * 3);
      HIP_TRY(hipMemsetAsync(frame.p, 0, (uint64_t)npix * 3 * sizeof(double), st));
    }
    return RPTGPU_OK;
  });
  if (rc != RPTGPU_OK) return rc;
  if (b->n_active == 0) {
    *out_active = 0;
    return RPTGPU_OK;
  }
  const uint32_t n = b->n_active;
  const uint32_t* list = b->active[b->cur].p;
  rc = render_impl(h, camera, params, b->packed.p, false, nullptr, nullptr, true, list, n);
  if (rc != RPTGPU_OK) return rc;
  return guarded(h, h->device, [&]() -> int {
    uint32_t left = 0;
    kt->buffer_accumulate(st, b->total.p, frame.p, b->packed.p, list, n, b->counts.p, b->mean.p, b->m2.p);
    kt->buffer_retire(st, list, n, b->counts.p, b->mean.p, b->m2.p, a->min_batches, a->abs_tol, a->rel_tol, b->keep.p,
                      b->block_cnt.p, b->active[b->cur ^ 1].p, b->active_n.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&left, b->active_n.p, sizeof left, hipMemcpyDeviceToHost, st)); // plans the next round
    HIP_TRY(hipStreamSynchronize(st));
    b->batches.push_back(std::move(frame));
    b->cur ^= 1;
    b->n_active = left;
    if (left < npix) b->retired = true;
    *out_active = left;
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_sample_counts(const rptgpu_buffer* b, uint32_t* out_counts) {
  if (!b || !out_counts) return RPTGPU_E_INVALID_ARGUMENT;
  rptgpu_scene* h = b->h;
  return guarded(h, h->device, [&]() -> int {
    HIP_TRY(hipMemcpyAsync(out_counts, b->counts.p, (uint64_t)b->width * b->height * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_totals(const rptgpu_buffer* b, double* out_totals) {
  if (!b || !out_totals) return RPTGPU_E_INVALID_ARGUMENT;
  rptgpu_scene* h = b->h;
  return guarded(h, h->device, [&]() -> int {
    HIP_TRY(hipMemcpyAsync(out_totals, b->total.p, (uint64_t)b->width * b->height * 3 * sizeof(double),
                           hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_image(rptgpu_buffer* b, uint8_t* out_rgb8) {
  if (!b || !out_rgb8) return RPTGPU_E_INVALID_ARGUMENT;
  rptgpu_scene* h = b->h;
  if (b->batches.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "Pixel found with no samples"); // buffer.rs:89
  return guarded(h, h->device, [&]() -> int {
    uint64_t n = (uint64_t)b->width * b->height * 3;
    b->image.alloc(n);
    table_for(RPT_PRECISION_F64_STRICT)->buffer_image(h->stream, b->total.p, b->counts.p, b->width, b->height, b->radius,
                                                      b->thr.p, b->image.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_rgb8, b->image.p, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_variance(rptgpu_buffer* b, double* out_variance) {
  if (!b || !out_variance) return RPTGPU_E_INVALID_ARGUMENT;
  rptgpu_scene* h = b->h;
  if (b->batches.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "no samples");
  return guarded(h, h->device, [&]() -> int {
    uint64_t npix = (uint64_t)b->width * b->height;
    std::vector<const double*> ptrs;
    for (const DevBuf<double>& frame : b->batches) ptrs.push_back(frame.p);
    b->batch_ptrs.upload(ptrs, h->stream);
    b->pix_var.alloc(npix);
    table_for(RPT_PRECISION_F64_STRICT)->buffer_variance(h->stream, b->total.p, b->batch_ptrs.p, b->counts.p, npix,
                                                         b->pix_var.p);
    HIP_TRY(hipGetLastError());
    std::vector<double> pv(npix);
    HIP_TRY(hipMemcpyAsync(pv.data(), b->pix_var.p, npix * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double variance = 0.0, count = 0.0; // buffer.rs:60-72: sequential sum over pixels in index order
    for (uint64_t p = 0; p < npix; p++) {
      variance += pv[p];
      count += 1.0;
    }
    *out_variance = variance / count;
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_num_batches(const rptgpu_buffer* b, uint32_t* out) {
  if (!b || !out) return RPTGPU_E_INVALID_ARGUMENT;
  *out = (uint32_t)b->batches.size();
  return RPTGPU_OK;
}

int rptgpu_buffer_features(rptgpu_buffer* b, const RptCamera* camera, const RptRenderParams* params) {
  rptgpu_scene* h = b ? b->h : nullptr;
  if (!b) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null buffer");
  if (const char* why = bad_aov_params(params)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!camera) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null camera");
  if (params->width != b->width || params->height != b->height)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "Invalid sample dimension"); // buffer.rs:33-36
  if (params->part_count > 1)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "part_count > 1: a buffer holds the features of the whole frame");
  if (h->abandoned)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "an aborted batch's device work never drained on this handle: destroy it");
  b->has_features = false; // (until the new ones are complete)
  return guarded(h, h->device, [&]() -> int {
    ensure_partition(h, *params);
    b->feat = aov_arrays(b->feat_arrays, h->stream, (uint64_t)b->width * b->height, FEATURE_CHANNELS);
    const bool read_overflow = aov_enqueue(h, *camera, *params, b->feat);
    if (int rc = drain_call(h, read_overflow)) return rc;
    b->has_features = true;
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_feature_sums(const rptgpu_buffer* b, const RptAovBuffers* out) {
  rptgpu_scene* h = b ? b->h : nullptr;
  if (const char* why = bad_aov(out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (out->channels & RPT_AOV_OBJECT)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "RptAovBuffers: RPT_AOV_OBJECT is named, but a buffer does not hold `object`");
  if (!b) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null buffer");
  if (!b->has_features) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "the buffer holds no features (rptgpu_buffer_features)");
  REFUSE_IF_ABANDONED(h);
  return guarded(h, h->device, [&]() -> int {
    copy_aov_out(b->feat, out->channels, ptrs_at(rptplan::AOV_ROWS, out, out->channels | rptplan::AOV_HITS, 0), (uint64_t)b->width * b->height, h->stream);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RPTGPU_OK;
  });
}

int rptgpu_buffer_denoise(rptgpu_buffer* b, const RptDenoise* d, double* out_linear, uint8_t* out_rgb8) {
  rptgpu_scene* h = b ? b->h : nullptr;
  if (const char* why = bad_denoise(d)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!b) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null buffer");
  if (!out_linear && !out_rgb8) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "out_linear and out_rgb8 are both NULL");
  if (!b->has_features) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "the buffer holds no features (rptgpu_buffer_features)");
  // n_p of every pixel is min(batches, the count it retired with), and a pixel only retires with n_p >= min_batches >= 2
  if (b->batches.size() < 2)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "a pixel holds fewer than two batches: there is no variance of one batch");
  REFUSE_IF_ABANDONED(h);
  return guarded(h, h->device, [&]() -> int {
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(RPT_PRECISION_F64_STRICT);
    const uint64_t n = (uint64_t)b->width * b->height;
    b->dn_cols.alloc(18 * n);
    b->dn_hit.alloc(n);
    if (out_linear) b->dn_linear.alloc(3 * n);
    if (out_rgb8) b->dn_rgb8.alloc(3 * n);
    double* col = b->dn_cols.p;
    double *c[2] = {col, col + 4 * n}, *v[2] = {col + 3 * n, col + 7 * n};
    double *g_normal = col + 8 * n, *g_position = col + 11 * n, *g_albedo = col + 14 * n, *g_depth = col + 17 * n;
    kt->denoise_prepare(st, b->total.p, b->counts.p, b->m2.p, b->feat, b->width, b->height, n, c[0], v[0], g_normal, g_position,
                        g_albedo, g_depth, b->dn_hit.p);
    rptdev::DenoiseGuide g{};
    g.normal = g_normal; g.position = g_position; g.albedo = g_albedo; g.depth = g_depth; g.hit = b->dn_hit.p;
    g.stride = n; g.width = b->width; g.height = b->height;
    rptdev::DenoiseSigmas sg{};
    sg.color2 = d->sigma_color * d->sigma_color; sg.normal = d->sigma_normal; sg.depth = d->sigma_depth;
    sg.albedo2 = d->sigma_albedo * d->sigma_albedo;
    int cur = 0;
    for (uint32_t l = 0; l < d->levels; l++, cur ^= 1) kt->denoise_level(st, g, c[cur], v[cur], c[cur ^ 1], v[cur ^ 1], 1u << l, sg);
    kt->denoise_finish(st, c[cur], n, n, b->thr.p, out_linear ? b->dn_linear.p : nullptr, out_rgb8 ? b->dn_rgb8.p : nullptr);
    HIP_TRY(hipGetLastError());
    if (out_linear) HIP_TRY(hipMemcpyAsync(out_linear, b->dn_linear.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_rgb8) HIP_TRY(hipMemcpyAsync(out_rgb8, b->dn_rgb8.p, 3 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RPTGPU_OK;
  });
}

} // extern "C" (buffer)
