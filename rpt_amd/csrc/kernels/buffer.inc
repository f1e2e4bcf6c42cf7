// kernels/buffer.inc — device-resident Buffer kernels (add, image, variance).
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ device-resident Buffer
// total += batch, element-wise, in insertion order (samples[index].iter().sum(), buffer.rs:86)
__global__ void __launch_bounds__(256) rpt_buffer_add(double* __restrict__ total, const double* __restrict__ batch,
                                                      uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) total[i] = total[i] + batch[i];
}

// Buffer::image: box filter (buffer.rs:75-93) + color_bytes (color.rs:18-24).  thr[k] is the
// smallest double v in [0,1] with trunc(255 * v^(1/2.2)) >= k, found on the host with the host's
// own pow: the conversion is a 256-step staircase, so a binary search reproduces it exactly.
__global__ void __launch_bounds__(256) rpt_buffer_image(const double* __restrict__ total, uint32_t w, uint32_t h,
                                                        uint32_t radius, uint32_t nbatches,
                                                        const double* __restrict__ thr, uint8_t* __restrict__ out) {
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
        count += nbatches;
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

// per-pixel sample variance of the batch means (buffer.rs:62-70); the host adds the pixels up
__global__ void __launch_bounds__(256) rpt_buffer_variance(const double* __restrict__ total,
                                                           const double* const* __restrict__ batches, uint32_t nb,
                                                           uint64_t npix, double* __restrict__ out) {
  uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  D3 mean = ld3(total + 3 * p) / (double)nb;
  double ss = 0.0;
  for (uint32_t b = 0; b < nb; b++) {
    D3 dlt = ld3(batches[b] + 3 * p) - mean;
    ss += dot(dlt, dlt); // magnitude_squared
  }
  out[p] = ss / ((double)nb - 1.0);
}

__global__ void __launch_bounds__(256) rpt_eval_math(int fn, uint64_t n, const double* __restrict__ x,
                                                     const double* __restrict__ y, double* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s, c;
  switch (fn) {
    case 0: out[i] = rptc_exp(x[i]); break; // (0, 2-6: the converged forms the kernels call, math_converged.h)
    case 1: out[i] = rpt_log(x[i]); break;
    case 2: out[i] = rptc_atan(x[i]); break;
    case 3: rptc_sincos_pio2(x[i], &s, &c); out[i] = s; break;
    case 4: rptc_sincos_pio2(x[i], &s, &c); out[i] = c; break;
    case 5: out[i] = rptc_acos(x[i]); break;
    case 6: out[i] = rptc_atan2(y[i], x[i]); break;
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
