// kernels/paths_views.inc — rpt_paths_views: the persistent path kernel over a piece of a batch of views (rptgpu_render_views
// under RPT_FLAG_VIEWS_PERSISTENT, DESIGN.md §15.2).  The loop is paths_loop.inc's, the text rpt_paths is compiled from; here
// are what only the views form needs — the piece's ids, the camera ray, the per-lane key — and its instantiations.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// the piece's indices i = 0 .. n - 1 are the call's j = j_base + i = view * npix_view + pixel: pixels[i] = pixel (the stream id,
// Frame::pixels of the piece) and view_of[i] = view - j_base / npix_view (ViewRays::view_of).  One 64-bit quotient per index
// here instead of one per camera ray and per taken path in the 256-VGPR kernel
__global__ void __launch_bounds__(256) rpt_views_ids(uint64_t j_base, uint64_t npix_view, uint32_t n, uint32_t* __restrict__ pixels,
                                                     uint32_t* __restrict__ view_of) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t v0 = j_base / npix_view, j = j_base + i, v = j / npix_view;
  pixels[i] = (uint32_t)(j - v * npix_view);
  view_of[i] = (uint32_t)(v - v0);
}

// the stream of a path of the piece's index p_local is keyed by its view's seed (Rng::k0, k1: rng_make's split)
RPT_DEV void views_rekey(const ViewRays& vr, uint32_t p_local, Rng& r) {
  const uint64_t seed = vr.seeds[vr.view_of[p_local]];
  r.k0 = (uint32_t)seed;
  r.k1 = (uint32_t)(seed >> 32);
}

// camera ray of sample `smp` of the piece's index p_local, whose pixel in its view is `pixel`: rpt_raygen_views' ray
// (kernels/wf_raygen_views.inc), expression for expression — PERSPECTIVE is camera_ray's, ORTHOGRAPHIC and PANORAMA are the
// header's — from the stream (the view's seed, pixel, sample) from draw 0 on; the path continues it behind these draws
RPT_DEV void views_camera_ray(const Frame& fr, const ViewRays& vr, uint32_t p_local, uint32_t pixel, uint32_t smp, D3& ro, D3& rd,
                              Rng& rr) {
  const uint32_t width = vr.width, height = vr.height;
  const uint32_t vi = vr.view_of[p_local];
  uint32_t y = pixel / width, x = pixel - y * width;
  const View& view = vr.views[vi];
  const Camera& cam = view.cam;
  const uint64_t seed = vr.seeds[vi];
  Rng rng = rng_make(seed, pixel, fr.sample_base + smp, 0);
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
  ro = origin;
  rd = dir;
  rr = rng;
}

#define RPT_PATHS_FORM RPT_PATHS_FORM_VIEWS
#include "paths_loop.inc"
#undef RPT_PATHS_FORM

// every instantiation paths_kernel() can pick (kernels/launch_paths.inc), as rpt_paths' own (kernels/buffer.inc)
template __global__ void rpt_paths_views<KdLds, false>(Scene, Frame, ViewRays, PersistArgs);
template __global__ void rpt_paths_views<KdFlat, false>(Scene, Frame, ViewRays, PersistArgs);
template __global__ void rpt_paths_views<KdFlat, true>(Scene, Frame, ViewRays, PersistArgs);
#if RPT_FUSE_QUERY && RPT_RAY_STASH >= 2
template __global__ void rpt_paths_views<KdFlat, false, true>(Scene, Frame, ViewRays, PersistArgs);
#if RPT_SCENE_CONSTS
template __global__ void rpt_paths_views<KdFlat, false, true, true>(Scene, Frame, ViewRays, PersistArgs);
#endif
#endif
template __global__ void rpt_paths_views<KdFlatG, false>(Scene, Frame, ViewRays, PersistArgs);
template __global__ void rpt_paths_views<KdFlatG, true>(Scene, Frame, ViewRays, PersistArgs);
template __global__ void rpt_paths_views<KdFlatF, false>(Scene, Frame, ViewRays, PersistArgs);
template __global__ void rpt_paths_views<KdFlatF, true>(Scene, Frame, ViewRays, PersistArgs);

#if !defined(__HIP_DEVICE_COMPILE__)
// the launchers the kernel tables point to (kernels.h)
#define RPT_PATHS_FORM RPT_PATHS_FORM_VIEWS
#include "launch_paths.inc"
#undef RPT_PATHS_FORM
void launch_views_ids(hipStream_t st, uint64_t j_base, uint64_t npix_view, uint32_t n, uint32_t* pixels, uint32_t* view_of) {
  hipLaunchKernelGGL(rpt_views_ids, dim3((n + 255u) / 256u), dim3(256), 0, st, j_base, npix_view, n, pixels, view_of);
}
#endif // !__HIP_DEVICE_COMPILE__
