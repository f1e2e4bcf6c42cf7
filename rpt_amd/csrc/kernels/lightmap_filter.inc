// kernels/lightmap_filter.inc — the geometry-guided a-trous filter of a baked lightmap (rptgpu_filter_lightmap, DESIGN.md
// §24; the contract with every order of operations is the comment in include/rpt_gpu_lightmap_filter.h).  Part of
// kernels_lightmap_filter.hip (inside namespace rptlightmapfilter).
//
// Three kernels, one lane per texel, no atomics and no LDS — kernels/denoise.inc's shape.  A block is 64 x 4 texels, so a wave
// is 64 consecutive x of ONE row and a tap at any spacing is, per value, one contiguous 512-byte read of a column (Guides;
// the ping-pong sets c and v are columns too).  A lane walks its taps in the contract's order (dx outer, dy inner,
// ascending) and adds in that order: the result is defined to the bit whatever the schedule.  The tap loops are NOT
// unrolled: the body holds an inlined exp, and 25 copies of it would be an instruction-cache problem for no arithmetic
// saved.  At steps of 4 and more a tile would not hold the taps anyway; the L2 takes the re-reads.
//
// A block's rows: blockIdx.y * 4 + threadIdx.y, then on in strides of 4 * gridDim.y (lightmap_filter_plan.h grid cuts
// gridDim.y to the launch limit), so a map of any height is one launch.

#define RPT_LF_DEV __device__ __forceinline__

struct F3 {
  double x, y, z;
};
RPT_LF_DEV F3 lf_ld3(const double* __restrict__ p) { return F3{p[0], p[1], p[2]}; }
RPT_LF_DEV F3 lf_col3(const double* __restrict__ col, uint64_t stride, uint64_t p) {
  return F3{col[p], col[stride + p], col[2 * stride + p]};
}
RPT_LF_DEV F3 lf_sub(const F3& a, const F3& b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RPT_LF_DEV double lf_dot(const F3& a, const F3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// the kernel of a level, k = [1/16, 1/4, 3/8, 1/4, 1/16], and of the variance prefilter, g = [1/4, 1/2, 1/4]
RPT_LF_DEV double lf_atrous_k(int d) { return d == 0 ? 0.375 : ((d == 1 || d == -1) ? 0.25 : 0.0625); }
RPT_LF_DEV double lf_prefilter_g(int d) { return d == 0 ? 0.5 : 0.25; }
RPT_LF_DEV bool lf_finite(double x) { return fabs(x) < LF_INF; }

// the filter's inputs as columns: position, normal, the validity byte, c = values, and v = the 3x3 prefilter of the valid
// neighbours' variance (taps outside the map skipped, dx outer / dy inner); a texel that is not valid: its variance
template <uint32_t WORDS>
__global__ void __launch_bounds__(256) rpt_lightmap_filter_prepare(Inputs in, Guides g, double* __restrict__ c_out,
                                                                   double* __restrict__ v_out) {
  const uint32_t x = blockIdx.x * 64u + threadIdx.x;
  if (x >= g.width) return;
  const uint64_t np = g.stride;
  for (uint64_t y = (uint64_t)blockIdx.y * 4u + threadIdx.y; y < g.height; y += (uint64_t)gridDim.y * 4u) {
    const uint64_t p = y * g.width + x;
    const bool valid = in.owner[p] >= 0;
    g.valid[p] = valid ? 1 : 0;
    const F3 pos = lf_ld3(in.position + 3 * p), nrm = lf_ld3(in.normal + 3 * p);
    g.position[p] = pos.x; g.position[np + p] = pos.y; g.position[2 * np + p] = pos.z;
    g.normal[p] = nrm.x; g.normal[np + p] = nrm.y; g.normal[2 * np + p] = nrm.z;
    for (uint32_t k = 0; k < WORDS; k++) c_out[k * np + p] = in.values[WORDS * p + k];
    if (!in.variance) continue;
    if (!valid) {
      v_out[p] = in.variance[p];
      continue;
    }
    double acc = 0.0, ws = 0.0;
    for (int dx = -1; dx <= 1; dx++) {
      const int64_t qx = (int64_t)x + dx;
      if (qx < 0 || qx >= (int64_t)g.width) continue;
      for (int dy = -1; dy <= 1; dy++) {
        const int64_t qy = (int64_t)y + dy;
        if (qy < 0 || qy >= (int64_t)g.height) continue;
        const uint64_t q = (uint64_t)qy * g.width + (uint64_t)qx;
        if (in.owner[q] < 0) continue;
        const double wgt = lf_prefilter_g(dx) * lf_prefilter_g(dy);
        acc = acc + wgt * in.variance[q];
        ws = ws + wgt;
      }
    }
    v_out[p] = acc / ws; // (the centre is valid: ws >= 0.25)
  }
}

// one level: taps q = p + step * (dx, dy), dx, dy in -2..2.  A tap's validity byte is loaded first and nothing else of a
// skipped tap; the centre tap weighs k(0) k(0) without an exponent; any other tap is skipped when a component of c_q is
// not finite or when its exponent e is not in [0, +inf) (a NaN fails both comparisons)
template <uint32_t WORDS, bool VARIANCE>
__global__ void __launch_bounds__(256) rpt_lightmap_filter_level(Guides g, const double* __restrict__ c_in,
                                                                 const double* __restrict__ v_in, double* __restrict__ c_out,
                                                                 double* __restrict__ v_out, uint32_t step, Sigmas sg) {
  const uint32_t x = blockIdx.x * 64u + threadIdx.x;
  if (x >= g.width) return;
  const uint64_t np = g.stride;
  const double sd = sg.distance * (double)step;
  const double sd2 = sd * sd, color2 = sg.color * sg.color;
  for (uint64_t y = (uint64_t)blockIdx.y * 4u + threadIdx.y; y < g.height; y += (uint64_t)gridDim.y * 4u) {
    const uint64_t p = y * g.width + x;
    double cp[WORDS];
    for (uint32_t k = 0; k < WORDS; k++) cp[k] = c_in[k * np + p];
    double vp = 0.0;
    if (VARIANCE) vp = v_in[p];
    if (!g.valid[p]) { // keeps its bits, and is nobody's tap
      for (uint32_t k = 0; k < WORDS; k++) c_out[k * np + p] = cp[k];
      if (VARIANCE) v_out[p] = vp;
      continue;
    }
    const F3 n_p = lf_col3(g.normal, np, p), p_p = lf_col3(g.position, np, p);
    double sum_c[WORDS];
    for (uint32_t k = 0; k < WORDS; k++) sum_c[k] = 0.0;
    double sum_w = 0.0, sum_v = 0.0;
#pragma unroll 1
    for (int dx = -2; dx <= 2; dx++) {
      const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)step;
      if (qx < 0 || qx >= (int64_t)g.width) continue;
#pragma unroll 1
      for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)dy * (int64_t)step;
        if (qy < 0 || qy >= (int64_t)g.height) continue;
        const uint64_t q = (uint64_t)qy * g.width + (uint64_t)qx;
        if (!g.valid[q]) continue;
        double cq[WORDS];
        for (uint32_t k = 0; k < WORDS; k++) cq[k] = c_in[k * np + q];
        double vq = 0.0;
        if (VARIANCE) vq = v_in[q];
        double wgt = lf_atrous_k(dx) * lf_atrous_k(dy);
        if (dx != 0 || dy != 0) {
          bool finite = true;
          for (uint32_t k = 0; k < WORDS; k++) finite = finite && lf_finite(cq[k]);
          if (!finite) continue;
          const F3 n_q = lf_col3(g.normal, np, q);
          const F3 d_pos = lf_sub(lf_col3(g.position, np, q), p_p);
          const double t = 1.0 - lf_dot(n_p, n_q);
          const double en = (t > 0.0 ? t : 0.0) / sg.normal;
          const double ez = fabs(lf_dot(n_p, d_pos)) / sg.plane;
          const double ed = lf_dot(d_pos, d_pos) / sd2;
          double e = (en + ez) + ed;
          if (VARIANCE) {
            double d2;
            if constexpr (WORDS == 3) {
              const F3 dc = F3{cq[0] - cp[0], cq[1] - cp[1], cq[2] - cp[2]};
              d2 = lf_dot(dc, dc);
            } else {
              const double dc = cq[0] - cp[0];
              d2 = dc * dc;
            }
            e = e + d2 / (color2 * (vp + vq) + 1e-12);
          }
          if (!(e >= 0.0 && e < LF_INF)) continue;
          wgt = wgt * rptc_exp(-e);
        }
        for (uint32_t k = 0; k < WORDS; k++) sum_c[k] = sum_c[k] + wgt * cq[k];
        sum_w = sum_w + wgt;
        if (VARIANCE) sum_v = sum_v + (wgt * wgt) * vq;
      }
    }
    for (uint32_t k = 0; k < WORDS; k++) c_out[k * np + p] = sum_c[k] / sum_w;
    if (VARIANCE) v_out[p] = sum_v / (sum_w * sum_w);
  }
}

// the last level's columns as the caller's arrays: [texel][WORDS], and the variance column beside them where it is wanted
template <uint32_t WORDS>
__global__ void __launch_bounds__(256) rpt_lightmap_filter_finish(uint64_t n, const double* __restrict__ c_in,
                                                                  const double* __restrict__ v_in, double* __restrict__ out,
                                                                  double* __restrict__ out_variance) {
  const uint64_t threads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += threads) {
    for (uint32_t k = 0; k < WORDS; k++) out[WORDS * p + k] = c_in[k * n + p];
    if (out_variance) out_variance[p] = v_in[p];
  }
}

// ---- the launchers (lightmap_filter.h)
hipError_t prepare(hipStream_t st, const Inputs& in, uint32_t words, const Guides& g, double* c, double* v) {
  const Grid gr = grid(g.width, g.height);
  const dim3 blocks(gr.x, gr.y), lanes(BLOCK_X, BLOCK_Y);
  if (words == 3) rpt_lightmap_filter_prepare<3><<<blocks, lanes, 0, st>>>(in, g, c, v);
  else rpt_lightmap_filter_prepare<1><<<blocks, lanes, 0, st>>>(in, g, c, v);
  return hipGetLastError();
}

hipError_t level(hipStream_t st, const Guides& g, uint32_t words, const double* c_in, const double* v_in, double* c_out,
                 double* v_out, uint32_t step, const Sigmas& sg) {
  const Grid gr = grid(g.width, g.height);
  const dim3 blocks(gr.x, gr.y), lanes(BLOCK_X, BLOCK_Y);
  if (words == 3) {
    if (v_in) rpt_lightmap_filter_level<3, true><<<blocks, lanes, 0, st>>>(g, c_in, v_in, c_out, v_out, step, sg);
    else rpt_lightmap_filter_level<3, false><<<blocks, lanes, 0, st>>>(g, c_in, v_in, c_out, v_out, step, sg);
  } else {
    if (v_in) rpt_lightmap_filter_level<1, true><<<blocks, lanes, 0, st>>>(g, c_in, v_in, c_out, v_out, step, sg);
    else rpt_lightmap_filter_level<1, false><<<blocks, lanes, 0, st>>>(g, c_in, v_in, c_out, v_out, step, sg);
  }
  return hipGetLastError();
}

hipError_t finish(hipStream_t st, uint64_t n, uint32_t words, const double* c, const double* v, double* out, double* out_variance) {
  const uint32_t blocks = finish_blocks(n);
  if (words == 3) rpt_lightmap_filter_finish<3><<<blocks, FINISH_BLOCK, 0, st>>>(n, c, v, out, out_variance);
  else rpt_lightmap_filter_finish<1><<<blocks, FINISH_BLOCK, 0, st>>>(n, c, v, out, out_variance);
  return hipGetLastError();
}
#undef RPT_LF_DEV
