// kernels/wf_raygen_views.inc — rpt_raygen_views and rpt_raygen_views_seeded: ONE text, included twice by wavefront.inc, with
// RPT_WF_SEEDED 0 and 1.  (A template <bool SEEDED> device function under two __global__ wrappers reads better and was
// tried; it changed the instructions of the unseeded kernels — DESIGN.md §15.1 — and those have to stay the parent's.)
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// The first step for a batch of views (rptgpu_render_views, include/rpt_gpu.h): slot = s_local * npix + p_local is sample
// fr.sample_base + s_local of index j = j_base + p_local of the CALL, and j = v * (width * height) + pixel names the view and
// its pixel.  The ray is made from the pixel's own stream (seed, pixel, sample) from draw 0 on, and the path continues that
// stream behind the camera's draws, as rpt_raygen's does.  The seed is fr.seed, the seed of every view of the call
// (rpt_raygen_views) — or view_seeds[v] (rpt_raygen_views_seeded: the call's views have seeds of their own, a piece may hold
// indices of several views, and the first sample's lanes write each index's seed to seeds_out[p_local], where
// rpt_shade_seeded will look for it; fr.seed is not read.  A launch makes the rays of the piece's indices p_lo .. p_lo +
// p_len - 1 alone, n_paths = p_len x the pass's samples of them in the slots the whole piece's launch would give them: the
// driver launches it once for every view a piece holds — RptStats' raygen count stays at least the number of views
// rendered under seeds of their own, as it was when such a view was a piece).  PERSPECTIVE is rpt_raygen's ray, expression for expression;
// ORTHOGRAPHIC and PANORAMA are the header's.  ids_out (= fr.pixels): the first sample's lanes write the stream id `pixel`
// where rpt_shade will look for it.
#if RPT_WF_SEEDED
#define RPT_WF_KERNEL(name) name##_seeded
#else
#define RPT_WF_KERNEL(name) name
#endif
__global__ void __launch_bounds__(256) RPT_WF_KERNEL(rpt_raygen_views)(Frame fr, const View* __restrict__ views, uint32_t width, uint32_t height,
                                                        uint64_t j_base, uint32_t* __restrict__ ids_out,
#if RPT_WF_SEEDED
                                                        const uint64_t* __restrict__ view_seeds, uint64_t* __restrict__ seeds_out,
                                                        uint32_t p_lo, uint32_t p_len,
#endif
                                                        PathState ps, uint32_t n_paths) {
#if RPT_WF_SEEDED
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_paths) return;
  uint32_t s_local = t / p_len, p_local = p_lo + (t - s_local * p_len);
  const uint32_t slot = s_local * fr.npix + p_local;
#else
  uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_paths) return;
  uint32_t s_local = slot / fr.npix, p_local = slot - s_local * fr.npix;
#endif
  const uint64_t npix_view = (uint64_t)width * height, j = j_base + p_local;
  const uint64_t v = j / npix_view;
  const uint32_t pixel = (uint32_t)(j - v * npix_view);
  uint32_t y = pixel / width, x = pixel - y * width;
  const View& view = views[v];
  const Camera& cam = view.cam;
#if RPT_WF_SEEDED
  const uint64_t seed = view_seeds[v];
#else
  const uint64_t seed = fr.seed;
#endif
  Rng rng = rng_make(seed, pixel, fr.sample_base + s_local, 0);
  D3 origin = ld3(cam.eye), dir;
  if (view.projection == RPT_VIEW_PANORAMA) {
    double jx = gen_range(rng, -0.5, 0.5);
    double jy = gen_range(rng, -0.5, 0.5);
    const double wm = (double)(width - 1), hm = (double)(height - 1);
    double cx = (double)x + jx;
    if (cx < 0.0) cx = cx + wm;
    else if (cx > wm) cx = cx - wm;
    double cy = (double)y + jy;
    cy = fmin(fmax(cy, 0.0), hm);
    // the azimuth in turns, (-1/2, 1/2]: beyond a quarter turn the angle half a turn back, and both results negated
    const double psi = cx / wm - 0.5;
    const bool back = fabs(psi) > 0.25;
    double s, c, se, ce;
    rptc_sincos_pio2(6.283185307179586 * (back ? psi - copysign(0.5, psi) : psi), &s, &c);
    if (back) { s = -s; c = -c; }
    rptc_sincos_pio2((0.5 - cy / hm) * 3.141592653589793, &se, &ce);
    dir = mk(ce * c, se, ce * s);
  } else {
    // renderer.rs:132-138, as rpt_raygen
    double dim = (double)max(width, height);
    double xn = ((double)(2 * x + 1) - (double)width) / dim;
    double yn = ((double)(2 * (height - y) - 1) - (double)height) / dim;
    double dx = gen_range(rng, -1.0 / dim, 1.0 / dim);
    double dy = gen_range(rng, -1.0 / dim, 1.0 / dim);
    double px = xn + dx, py = yn + dy;
    D3 direction = ld3(cam.direction), up = ld3(cam.up), right = ld3(cam.right);
    if (view.projection == RPT_VIEW_ORTHOGRAPHIC) {
      origin = origin + (px * right + py * up) * view.ortho_scale; // the form of camera.rs:74
      dir = normalize(direction);
    } else { // Camera::cast_ray camera.rs:64-81
      D3 new_dir = cam.d * direction + px * right + py * up;
      if (cam.aperture > 0.0) {
        D3 focal_point = origin + normalize(new_dir) * cam.focal_distance;
        double a, b;
        unit_disc(rng, a, b);
        origin = origin + (a * right + b * up) * cam.aperture;
        new_dir = focal_point - origin;
      }
      dir = normalize(new_dir);
    }
  }
  st_soa3(ps.ray, ps.cap, slot, origin);
  st_soa3(ps.ray + 3 * ps.cap, ps.cap, slot, dir);
  ps.draw[slot] = rng.draw;
  ps.pid[slot] = slot;
  if (s_local == 0) ids_out[p_local] = pixel;
#if RPT_WF_SEEDED
  if (s_local == 0) seeds_out[p_local] = seed;
#endif
}
#undef RPT_WF_KERNEL
