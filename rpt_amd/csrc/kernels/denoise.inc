// kernels/denoise.inc — the feature-guided à-trous filter of the device-resident Buffer (rptgpu_buffer_denoise,
// DESIGN.md §12; the contract with every order of operations is the comment in include/rpt_gpu.h).  Part of kernels.inc
// (inside namespace RPT_NS).
//
// Three kernels, one lane per pixel, no atomics and no LDS.  A block is 64 x 4 pixels, so a wave is 64 consecutive x of
// ONE row and a tap at any spacing is, per value, one contiguous 512-byte read of a column (DenoiseGuide).  A lane walks
// its taps in the contract's order (dx outer, dy inner, ascending) and adds in that order: the result is defined to
// the bit whatever the schedule.  The tap loops are NOT unrolled: the body holds an inlined exp, and 25 copies of it
// would be an instruction-cache problem for no arithmetic saved.
//
// ONE text, included twice by kernels.inc: RPT_DN_VIEWS 0 gives the Buffer's three kernels, one camera's frame per launch; 1
// gives rpt_denoise_views_prepare / _level / _finish (rptgpu_render_views_denoised, DESIGN.md §18), one launch for a batch of
// views of one size.  There the arrays and columns hold n_views * w * h elements, view after view; a block's view is view0 +
// blockIdx.z, a pixel's index is view * (w * h) + y * w + x, and x, y and every tap's bounds are those of the view's own
// frame: a tap never reads another view.  (Why not a template: wf_raygen_views.inc.)
#if RPT_DN_VIEWS
#define RPT_DN_KERNEL(name) rpt_denoise_views_##name
#else
#define RPT_DN_KERNEL(name) rpt_denoise_##name

// the kernel of a level, k = [1/16, 1/4, 3/8, 1/4, 1/16], and of the variance prefilter, g = [1/4, 1/2, 1/4]
RPT_DEV double atrous_k(int d) { return d == 0 ? 0.375 : ((d == 1 || d == -1) ? 0.25 : 0.0625); }
RPT_DEV double prefilter_g(int d) { return d == 0 ? 0.5 : 0.25; }
// the scalar variance of pixel q's mean: (M2 / (n - 1)) / n
RPT_DEV double mean_variance(const uint32_t* __restrict__ counts, const double* __restrict__ m2, uint64_t q) {
  const double n = (double)counts[q];
  return (m2[q] / (n - 1.0)) / n;
}
#endif

// the filter's inputs as columns: c = total / n, v = the 3x3 prefilter of the neighbours' mean_variance (taps outside
// the frame skipped, dx outer / dy inner), the means of the held feature sums and the hit flag (0 everywhere for a miss)
__global__ void __launch_bounds__(256) RPT_DN_KERNEL(prepare)(const double* __restrict__ total, const uint32_t* __restrict__ counts,
                                                           const double* __restrict__ m2, AovOut feat, uint32_t w, uint32_t h,
                                                           uint64_t stride, double* __restrict__ c_out, double* __restrict__ v_out,
                                                           double* __restrict__ g_normal, double* __restrict__ g_position,
                                                           double* __restrict__ g_albedo, double* __restrict__ g_depth,
                                                           uint8_t* __restrict__ g_hit
#if RPT_DN_VIEWS
                                                           , uint32_t view0 /* the launch's first view */
#endif
                                                           ) {
  const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
  if (x >= w || y >= h) return;
#if RPT_DN_VIEWS
  const uint64_t base = ((uint64_t)view0 + blockIdx.z) * ((uint64_t)w * h); // the view's first element
  const uint64_t p = base + (uint64_t)y * w + x;
#else
  const uint64_t p = (uint64_t)y * w + x;
#endif
  const D3 c = ld3(total + 3 * p) / (double)counts[p];
  c_out[p] = c.x; c_out[stride + p] = c.y; c_out[2 * stride + p] = c.z;
  double acc = 0.0, ws = 0.0;
  for (int dx = -1; dx <= 1; dx++) {
    const int64_t qx = (int64_t)x + dx;
    if (qx < 0 || qx >= (int64_t)w) continue;
    for (int dy = -1; dy <= 1; dy++) {
      const int64_t qy = (int64_t)y + dy;
      if (qy < 0 || qy >= (int64_t)h) continue;
      const double wgt = prefilter_g(dx) * prefilter_g(dy);
#if RPT_DN_VIEWS
      acc = acc + wgt * mean_variance(counts, m2, base + (uint64_t)qy * w + (uint64_t)qx);
#else
      acc = acc + wgt * mean_variance(counts, m2, (uint64_t)qy * w + (uint64_t)qx);
#endif
      ws = ws + wgt;
    }
  }
  v_out[p] = acc / ws;
  const uint32_t hits = feat.hits[p];
  D3 nrm = mk(0, 0, 0), pos = mk(0, 0, 0), alb = mk(0, 0, 0);
  double z = 0.0;
  if (hits) {
    const double hd = (double)hits;
    nrm = ld3(feat.normal + 3 * p) / hd;
    pos = ld3(feat.position + 3 * p) / hd;
    alb = ld3(feat.albedo + 3 * p) / hd;
    z = feat.depth[p] / hd;
  }
  g_normal[p] = nrm.x; g_normal[stride + p] = nrm.y; g_normal[2 * stride + p] = nrm.z;
  g_position[p] = pos.x; g_position[stride + p] = pos.y; g_position[2 * stride + p] = pos.z;
  g_albedo[p] = alb.x; g_albedo[stride + p] = alb.y; g_albedo[2 * stride + p] = alb.z;
  g_depth[p] = z;
  g_hit[p] = hits ? 1 : 0;
}

// one level: taps q = p + step * (dx, dy), dx, dy in -2..2.  The centre tap weighs k(0) k(0) without an exponent; any
// other tap is skipped when hit_q != hit_p or when its exponent e is not in [0, +inf) (a NaN fails both comparisons)
__global__ void __launch_bounds__(256) RPT_DN_KERNEL(level)(DenoiseGuide g, const double* __restrict__ c_in,
                                                         const double* __restrict__ v_in, double* __restrict__ c_out,
                                                         double* __restrict__ v_out, uint32_t step, DenoiseSigmas sg
#if RPT_DN_VIEWS
                                                         , uint32_t view0 /* the launch's first view */
#endif
                                                         ) {
  const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
  if (x >= g.width || y >= g.height) return;
  const uint64_t np = g.stride;
#if RPT_DN_VIEWS
  const uint64_t base = ((uint64_t)view0 + blockIdx.z) * ((uint64_t)g.width * g.height); // the view's first element
  const uint64_t p = base + (uint64_t)y * g.width + x;
#else
  const uint64_t p = (uint64_t)y * g.width + x;
#endif
  const D3 cp = ld_soa3(c_in, np, p);
  const double vp = v_in[p];
  const bool hit_p = g.hit[p] != 0;
  D3 n_p = mk(0, 0, 0), p_p = mk(0, 0, 0), a_p = mk(0, 0, 0);
  double z_den = 0.0;
  if (hit_p) {
    n_p = ld_soa3(g.normal, np, p);
    p_p = ld_soa3(g.position, np, p);
    a_p = ld_soa3(g.albedo, np, p);
    z_den = sg.depth * g.depth[p] + 1e-12;
  }
  D3 sum_c = mk(0, 0, 0);
  double sum_w = 0.0, sum_v = 0.0;
#pragma unroll 1
  for (int dx = -2; dx <= 2; dx++) {
    const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)step;
    if (qx < 0 || qx >= (int64_t)g.width) continue;
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
      const int64_t qy = (int64_t)y + (int64_t)dy * (int64_t)step;
      if (qy < 0 || qy >= (int64_t)g.height) continue;
#if RPT_DN_VIEWS
      const uint64_t q = base + (uint64_t)qy * g.width + (uint64_t)qx;
#else
      const uint64_t q = (uint64_t)qy * g.width + (uint64_t)qx;
#endif
      const D3 cq = ld_soa3(c_in, np, q);
      const double vq = v_in[q];
      double wgt = atrous_k(dx) * atrous_k(dy);
      if (dx != 0 || dy != 0) {
        if ((g.hit[q] != 0) != hit_p) continue;
        const D3 dc = cq - cp;
        double e = dot(dc, dc) / (sg.color2 * (vp + vq) + 1e-12);
        if (hit_p) {
          const D3 n_q = ld_soa3(g.normal, np, q);
          const D3 p_q = ld_soa3(g.position, np, q);
          const D3 a_q = ld_soa3(g.albedo, np, q);
          const double t = 1.0 - dot(n_p, n_q);
          const double en = (t > 0.0 ? t : 0.0) / sg.normal;
          const double ez = fabs(dot(n_p, p_q - p_p)) / z_den;
          const D3 da = a_q - a_p;
          const double ea = dot(da, da) / sg.albedo2;
          e = e + ((en + ez) + ea);
        }
        if (!(e >= 0.0 && e < INF)) continue;
        wgt = wgt * rptc_exp(-e);
      }
      sum_c = sum_c + wgt * cq;
      sum_w = sum_w + wgt;
      sum_v = sum_v + (wgt * wgt) * vq;
    }
  }
  const D3 c = sum_c / sum_w;
  c_out[p] = c.x; c_out[np + p] = c.y; c_out[2 * np + p] = c.z;
  v_out[p] = sum_v / (sum_w * sum_w);
}

// the last level's colour columns as the caller's arrays: [pixel][3] f64, and / or color_bytes of it through the
// buffer's staircase (thr[k]: the smallest v in [0, 1] whose byte is >= k, as rpt_buffer_image uses it).
// rpt_denoise_views_finish: over the batch's npix = n_views * w * h elements, and beside them the filter's two unfiltered
// inputs for the caller, either may be null: out_mean = c_p = total / n as [pixel][3], out_variance = u_p (mean_variance)
__global__ void __launch_bounds__(256) RPT_DN_KERNEL(finish)(const double* __restrict__ c_in, uint64_t stride, uint64_t npix,
                                                          const double* __restrict__ thr, double* __restrict__ out_linear,
                                                          uint8_t* __restrict__ out_rgb8
#if RPT_DN_VIEWS
                                                          , const double* __restrict__ total, const uint32_t* __restrict__ counts,
                                                          const double* __restrict__ m2, double* __restrict__ out_mean,
                                                          double* __restrict__ out_variance
#endif
                                                          ) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
#if RPT_DN_VIEWS
  if (out_mean) {
    const D3 c = ld3(total + 3 * p) / (double)counts[p];
    out_mean[3 * p] = c.x; out_mean[3 * p + 1] = c.y; out_mean[3 * p + 2] = c.z;
  }
  if (out_variance) out_variance[p] = mean_variance(counts, m2, p);
#endif
  const double v[3] = {c_in[p], c_in[stride + p], c_in[2 * stride + p]};
  for (int ch = 0; ch < 3; ch++) {
    if (out_linear) out_linear[3 * p + ch] = v[ch];
    if (out_rgb8) {
      const double t = fmin(fmax(v[ch], 0.0), 1.0); // .max(0.0).min(1.0): NaN -> 0
      int lo = 0, hi = 255;                         // largest k with thr[k] <= t
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (thr[mid] <= t) lo = mid;
        else hi = mid - 1;
      }
      out_rgb8[3 * p + ch] = (uint8_t)lo;
    }
  }
}
#undef RPT_DN_KERNEL
