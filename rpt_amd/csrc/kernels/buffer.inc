// kernels/buffer.inc — device-resident Buffer kernels (accumulate, retire, image, variance).
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ device-resident Buffer
// One batch into the buffer (DESIGN.md §10).  list == nullptr: a full frame `frame`, pixel i at i (rptgpu_buffer_sample);
// otherwise the n listed pixels of an adaptive round, the i-th one's value at packed[3i..] (rpt_finish's packed output),
// scattered into `frame` (zero elsewhere).  Per pixel: total += x element-wise in insertion order (samples[index].iter()
// .sum(), buffer.rs:86) and the Welford update n += 1, d = x - m, m += d / n, M2 += dot(d, x - m).
__global__ void __launch_bounds__(256) rpt_buffer_accumulate(double* __restrict__ total, double* __restrict__ frame,
                                                             const double* __restrict__ packed,
                                                             const uint32_t* __restrict__ list, uint32_t n,
                                                             uint32_t* __restrict__ counts, double* __restrict__ mean,
                                                             double* __restrict__ m2) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t p = list ? (uint64_t)list[i] : (uint64_t)i;
  D3 x;
  if (list) {
    x = ld3(packed + 3 * (uint64_t)i);
    frame[3 * p] = x.x; frame[3 * p + 1] = x.y; frame[3 * p + 2] = x.z;
  } else {
    x = ld3(frame + 3 * p);
  }
  const D3 t = ld3(total + 3 * p) + x;
  total[3 * p] = t.x; total[3 * p + 1] = t.y; total[3 * p + 2] = t.z;
  const uint32_t c = counts[p] + 1u;
  counts[p] = c;
  const D3 m0 = ld3(mean + 3 * p);
  const D3 d = x - m0;
  const D3 m = m0 + d / (double)c;
  mean[3 * p] = m.x; mean[3 * p + 1] = m.y; mean[3 * p + 2] = m.z;
  m2[p] = m2[p] + dot(d, x - m);
}

// ---- retiring converged pixels: the active list without them, in its own order (the round-0 list's 8x8 blocks);
// RPT_RETIRE_TILE (kernels.h) list entries per 256-thread block, RPT_RETIRE_ITEMS per thread
// the stopping rule: n >= min_batches and (M2 / (n - 1)) / n <= t * t, t = abs_tol + rel_tol * ((m.x + m.y) + m.z); a NaN
// makes the comparison false, so such a pixel stays
RPT_DEV bool stays_active(uint32_t p, const uint32_t* __restrict__ counts, const double* __restrict__ mean,
                          const double* __restrict__ m2, uint32_t min_batches, double abs_tol, double rel_tol) {
  const uint32_t n = counts[p];
  const D3 m = ld3(mean + 3 * (uint64_t)p);
  const double e = (m2[p] / ((double)n - 1.0)) / (double)n;
  const double t = abs_tol + rel_tol * ((m.x + m.y) + m.z);
  return !(n >= min_batches && e <= t * t);
}
// pass 1: the rule for every listed pixel (keep[i]) and how many of a block's RPT_RETIRE_TILE entries stay (block_cnt)
__global__ void __launch_bounds__(256) rpt_retire_count(const uint32_t* __restrict__ list, uint32_t n,
                                                        const uint32_t* __restrict__ counts, const double* __restrict__ mean,
                                                        const double* __restrict__ m2, uint32_t min_batches, double abs_tol,
                                                        double rel_tol, uint8_t* __restrict__ keep,
                                                        uint32_t* __restrict__ block_cnt) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = blockIdx.x * RPT_RETIRE_TILE;
  uint32_t cnt = 0; // (the same in every lane of a wave)
  for (uint32_t k = 0; k < RPT_RETIRE_ITEMS; k++) {
    const uint32_t i = tile + k * 256u + threadIdx.x;
    bool kp = false;
    if (i < n) {
      kp = stays_active(list[i], counts, mean, m2, min_batches, abs_tol, rel_tol);
      keep[i] = kp ? 1 : 0;
    }
    cnt += (uint32_t)__popcll(__ballot(kp));
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}
// pass 2: the block's offset (the kept entries of the blocks before it), then per group of 256 entries a ballot, the
// lane's rank among the kept lanes below it and an LDS scan over the four waves: every kept entry lands at its rank in
// the old list's order, whatever the schedule.  The last block writes the new length.
__global__ void __launch_bounds__(256) rpt_retire_scatter(const uint32_t* __restrict__ list, uint32_t n,
                                                          const uint8_t* __restrict__ keep,
                                                          const uint32_t* __restrict__ block_cnt,
                                                          uint32_t* __restrict__ out_list, uint32_t* __restrict__ out_n) {
  __shared__ uint32_t s_sum[256];
  __shared__ uint32_t s_cnt[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t sum = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256u) sum += block_cnt[j];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t s = 128u; s > 0; s >>= 1) {
    if (threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
    __syncthreads();
  }
  uint32_t off = s_sum[0];
  const uint32_t tile = blockIdx.x * RPT_RETIRE_TILE;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t k = 0; k < RPT_RETIRE_ITEMS; k++) {
    const uint32_t i = tile + k * 256u + threadIdx.x;
    const bool kp = i < n && keep[i] != 0;
    const uint64_t mask = __ballot(kp);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t wave_off = 0;
    for (uint32_t w = 0; w < wave; w++) wave_off += s_cnt[w];
    if (kp) out_list[off + wave_off + (uint32_t)__popcll(mask & below)] = list[i];
    off += (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    __syncthreads(); // (s_cnt is written again by the next group)
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *out_n = off;
}

// Buffer::image: box filter (buffer.rs:75-93) + color_bytes (color.rs:18-24).  thr[k] is the
// smallest double v in [0,1] with trunc(255 * v^(1/2.2)) >= k, found on the host with the host's
// own pow: the conversion is a 256-step staircase, so a binary search reproduces it exactly.
// counts[q]: the batches pixel q holds (samples[index].len(): the buffer's batch count in every pixel until one retires)
__global__ void __launch_bounds__(256) rpt_buffer_image(const double* __restrict__ total,
                                                        const uint32_t* __restrict__ counts, uint32_t w, uint32_t h,
                                                        uint32_t radius, const double* __restrict__ thr,
                                                        uint8_t* __restrict__ out) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= w * h) return;
  uint32_t y = p / w, x = p - y * w;
  D3 color = mk(0, 0, 0);
  uint64_t count = 0;
  uint32_t i0 = x >= radius ? x - radius : 0, j0 = y >= radius ? y - radius : 0;
  for (uint32_t i = i0; i <= x + radius; i++)
    for (uint32_t j = j0; j <= y + radius; j++)
      if (i < w && j < h) {
        color = color + ld3(total + 3 * ((uint64_t)j * w + i));
        count += counts[(uint64_t)j * w + i];
      }
  D3 c = color / (double)count;
  double v[3] = {c.x, c.y, c.z};
  for (int ch = 0; ch < 3; ch++) {
    double t = fmin(fmax(v[ch], 0.0), 1.0); // .max(0.0).min(1.0): NaN -> 0
    int lo = 0, hi = 255;                   // largest k with thr[k] <= t
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (thr[mid] <= t) lo = mid;
      else hi = mid - 1;
    }
    out[3 * (uint64_t)p + ch] = (uint8_t)lo;
  }
}

// per-pixel sample variance of the batch means (buffer.rs:62-70) over the pixel's own counts[p] batches — batches 0 ..
// counts[p] - 1 of the buffer, since a retired pixel is never sampled again; the host adds the pixels up
__global__ void __launch_bounds__(256) rpt_buffer_variance(const double* __restrict__ total,
                                                           const double* const* __restrict__ batches,
                                                           const uint32_t* __restrict__ counts, uint64_t npix,
                                                           double* __restrict__ out) {
  uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const uint32_t nb = counts[p];
  D3 mean = ld3(total + 3 * p) / (double)nb;
  double ss = 0.0;
  for (uint32_t b = 0; b < nb; b++) {
    D3 dlt = ld3(batches[b] + 3 * p) - mean;
    ss += dot(dlt, dlt); // magnitude_squared
  }
  out[p] = ss / ((double)nb - 1.0);
}

// fn 8-11 of rpt_eval_math: y / x through div_ieee<N> (vec.inc), N = 2, 3, 4, 6.  The n pairs are cut into N blocks of
// t = n / N; thread i < t fills slot s from block s, at the block's position (i + s * 4099) % t — every slot of a batch
// from another place, so that a mix-up of slots shows — and writes each quotient where its operands stand.  The
// n - N * t pairs behind the blocks get the plain quotient
template <int N> RPT_DEV void eval_div_batch(uint64_t i, uint64_t n, const double* x, const double* y, double* out) {
  const uint64_t t = n / N;
  if (i < t) {
    uint64_t p[N];
    double nn[N], dd[N], q[N];
#pragma unroll
    for (int s = 0; s < N; s++) {
      p[s] = (uint64_t)s * t + (i + (uint64_t)s * 4099ull) % t;
      nn[s] = y[p[s]];
      dd[s] = x[p[s]];
    }
    div_ieee<N>(nn, dd, q);
#pragma unroll
    for (int s = 0; s < N; s++) out[p[s]] = q[s];
  }
  if (i < n - t * N) out[t * N + i] = y[t * N + i] / x[t * N + i];
}

#if RPT_SHADE_SPLIT
// fn 12 and 13 of rpt_eval_math: a hit's draws (paths_shade.inc hit_draws).  The arrays hold raw 64-bit words, nine per
// element (include/rpt_gpu.h has the layout); thread e < n / 9 runs element e.  hit_draws_reference is the reference's
// sequence written with next_u64 alone, one draw per call
RPT_DEV void hit_draws_reference(Rng& r, bool sf, uint64_t n, uint64_t zone, double f, HitDraws& o) {
  for (;;) {
    const uint64_t v = next_u64(r);
    if (v * n <= zone) { o.tri = __umul64hi(v, n); break; }
  }
  do {
    o.a = next_u64(r);
    o.b = next_u64(r);
  } while (uv_rejected(o.a, o.b));
  o.th = 1ull << 63; o.qa = 0; o.qb = 0; o.spec = false;
  if (!sf) return;
  o.spec = f == 1.0 ? true : next_u64(r) < (uint64_t)(f * 18446744073709551616.0);
  if (o.spec) o.th = next_u64(r);
  for (;;) {
    o.qa = next_u64(r);
    o.qb = next_u64(r);
    const double px = u52_of(o.qa) * 2.0 + -1.0, py = u52_of(o.qb) * 2.0 + -1.0;
    const double sum = px * px + py * py;
    if (o.spec ? sum < 1.0 : sum <= 1.0) break;
  }
}
RPT_DEV void eval_hit_draws(bool reference, uint64_t e, uint64_t n, const double* x, double* out) {
  if (e < n - n / 9 * 9) out[n / 9 * 9 + e] = 0.0; // the words behind the last whole element
  if (e >= n / 9) return;
  uint64_t in[9];
#pragma unroll
  for (int k = 0; k < 9; k++) in[k] = (uint64_t)__double_as_longlong(x[e * 9 + k]);
  Rng r = rng_make(in[0], (uint32_t)in[1], in[2], (uint32_t)in[3]);
  const double f = __longlong_as_double((long long)in[6]);
  const bool sf = in[7] & 1ull;
  HitDraws o;
  if (reference) {
    hit_draws_reference(r, sf, in[4], in[5], f, o);
  } else if (in[7] & 2ull) { // as the kernels with the material's constants call it
    MatConsts mc{};
    mc.fs = f;
    mc.p_int = f == 1.0 ? 0ull : (uint64_t)(f * 18446744073709551616.0);
    hit_draws<true>(r, sf, in[4], in[5], f, o, &mc);
  } else {
    hit_draws<false>(r, sf, in[4], in[5], f, o);
  }
  const uint64_t res[9] = {o.tri, o.a, o.b, o.th, o.qa, o.qb, o.spec ? 1ull : 0ull, (uint64_t)r.draw, (r.draw & 1u) ? r.hi : 0ull};
#pragma unroll
  for (int k = 0; k < 9; k++) out[e * 9 + k] = __longlong_as_double((long long)res[k]);
}
#endif

__global__ void __launch_bounds__(256) rpt_eval_math(int fn, uint64_t n, const double* __restrict__ x,
                                                     const double* __restrict__ y, double* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s, c;
  switch (fn) {
#if RPT_SHADE_SPLIT
    case 12: eval_hit_draws(false, i, n, x, out); break;
    case 13: eval_hit_draws(true, i, n, x, out); break;
#endif
    case 0: out[i] = rptc_exp(x[i]); break; // (0, 2-6: the converged forms the kernels call, math_converged.h)
    case 1: out[i] = rpt_log(x[i]); break;
    case 2: out[i] = rptc_atan(x[i]); break;
    case 3: rptc_sincos_pio2(x[i], &s, &c); out[i] = s; break;
    case 4: rptc_sincos_pio2(x[i], &s, &c); out[i] = c; break;
    case 5: out[i] = rptc_acos(x[i]); break;
    case 6: out[i] = rptc_atan2(y[i], x[i]); break;
    case 8: eval_div_batch<2>(i, n, x, y, out); break;
    case 9: eval_div_batch<3>(i, n, x, y, out); break;
    case 10: eval_div_batch<4>(i, n, x, y, out); break;
    case 11: eval_div_batch<6>(i, n, x, y, out); break;
    default: { // 7: y / x through the shared reciprocal wherever the kernels' range predicate allows it
      RcpD rc = rcp_make(x[i]);
      double a = fabs(y[i]);
      out[i] = (rc.ok && safe_range(a, a)) ? div_fast(y[i], rc) : y[i] / x[i];
      break;
    }
  }
}

// explicit instantiations: the launchers below are compiled in the host pass only, so the
// device pass needs these to emit the two kernels
template __global__ void rpt_paths<KdLds, false>(Scene, Frame, Camera, PersistArgs);
template __global__ void rpt_paths<KdFlat, false>(Scene, Frame, Camera, PersistArgs);
template __global__ void rpt_paths<KdFlat, true>(Scene, Frame, Camera, PersistArgs);
#if RPT_FUSE_QUERY && RPT_RAY_STASH >= 2
template __global__ void rpt_paths<KdFlat, false, true>(Scene, Frame, Camera, PersistArgs); // (C2: one light)
#if RPT_SCENE_CONSTS
template __global__ void rpt_paths<KdFlat, false, true, true>(Scene, Frame, Camera, PersistArgs); // (C2: its constants in tables)
#endif
#endif
template __global__ void rpt_paths<KdFlatG, false>(Scene, Frame, Camera, PersistArgs);
template __global__ void rpt_paths<KdFlatG, true>(Scene, Frame, Camera, PersistArgs);
template __global__ void rpt_paths<KdFlatF, false>(Scene, Frame, Camera, PersistArgs);
template __global__ void rpt_paths<KdFlatF, true>(Scene, Frame, Camera, PersistArgs);
template __global__ void rpt_rays_objects<false, KdLdsW>(Scene, RayBatch, const uint32_t*, uint32_t, int, int);
template __global__ void rpt_rays_objects<true, KdLdsW>(Scene, RayBatch, const uint32_t*, uint32_t, int, int);
template __global__ void rpt_rays_objects<false, KdFlat>(Scene, RayBatch, const uint32_t*, uint32_t, int, int);
template __global__ void rpt_rays_objects<true, KdFlat>(Scene, RayBatch, const uint32_t*, uint32_t, int, int);
#ifdef RPT_EXT_SHAPES
template __global__ void rpt_nest_trace<false>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_nest_trace<true>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, StackSpill);
#endif
template __global__ void rpt_tree_enter<false>(Scene, RayBatch, const uint32_t*, uint32_t, int, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, double*, uint32_t);
template __global__ void rpt_tree_enter<true>(Scene, RayBatch, const uint32_t*, uint32_t, int, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, double*, uint32_t);
template __global__ void rpt_tree_trace<true, false, false>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_trace<true, false, true>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_trace<true, true, false>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_trace<true, true, true>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_trace<false, false, false>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_trace<false, false, true>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_trace<false, true, false>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_trace<false, true, true>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, StackSpill);
template __global__ void rpt_tree_generic<false>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, GenericStack, uint32_t*, uint32_t*);
template __global__ void rpt_tree_generic<true>(Scene, RayBatch, int, const uint32_t*, const uint32_t*, GenericStack, uint32_t*, uint32_t*);
template __global__ void rpt_finish<float>(Frame, double, double, float*, int);
template __global__ void rpt_finish<double>(Frame, double, double, double*, int);
