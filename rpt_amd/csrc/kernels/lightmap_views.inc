// kernels/lightmap_views.inc — rptgpu_render_views_lightmapped's two kernels (include/rpt_gpu_lightmap_lookup.h, DESIGN.md §25).
// rpt_views_rays_gather: the rays rpt_raygen_views wrote as columns, interleaved for the ray form's steps.
// rpt_views_lightmapped_fold: per index of the piece the sample's radiance — the environment at a miss, else the hit
// material's emission plus its Lambert term under the looked-up irradiance — added to the sum `out` keeps between passes.
// Compiled in a translation unit of its own (kernels_lightmap_views.hip, inside namespace rptlookupviews, over kernels/vec.inc).

__global__ void __launch_bounds__(256) rpt_views_rays_gather(const double* __restrict__ rays, uint64_t cap, uint32_t m,
                                                             double* __restrict__ origins, double* __restrict__ dirs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double* __restrict__ o = origins + 3ull * i;
  double* __restrict__ d = dirs + 3ull * i;
  o[0] = rays[i]; o[1] = rays[cap + i]; o[2] = rays[2 * cap + i];
  d[0] = rays[3 * cap + i]; d[1] = rays[4 * cap + i]; d[2] = rays[5 * cap + i];
}

// Environment::get_color (environment.rs:25-52, 72-77): kernels/light.inc's env_color restated, expression for expression
RPT_DEV uint32_t sat_u32(double v) { // Rust `as u32`: saturating, NaN -> 0
  if (!(v > 0.0)) return 0u;
  if (v >= 4294967295.0) return 4294967295u;
  return (uint32_t)v;
}
RPT_DEV D3 env_color(const Scene& sc, D3 dir_in) {
  if (sc.env_kind == RPT_ENV_COLOR) return ld3(sc.env_color);
  D3 dir = normalize(dir_in);
  double azimuth = rptc_atan2(dir.z, dir.x) + PI;
  double polar = rptc_acos(dir.y);
  double x = azimuth / TAU * (double)(sc.env_width - 1);
  double y = polar / PI * (double)(sc.env_height - 1);
  uint32_t x0 = min(sat_u32(x), sc.env_width - 1);
  uint32_t y0 = min(sat_u32(y), sc.env_height - 1);
  double ax = x - (double)x0;
  double ay = y - (double)y0;
  uint64_t w = sc.env_width;
  const double* t = sc.env_texels;
  D3 top = lerp(ld3(t + 3 * (y0 * w + x0)), ld3(t + 3 * (y0 * w + x0 + 1)), ax);
  D3 bot = lerp(ld3(t + 3 * ((y0 + 1) * w + x0)), ld3(t + 3 * ((y0 + 1) * w + x0 + 1)), ax);
  return lerp(top, bot, ay);
}

__global__ void __launch_bounds__(256) rpt_views_lightmapped_fold(Scene sc, uint32_t m, Sample s, double* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int32_t obj = s.object[i];
  D3 L;
  if (obj < 0 || obj >= sc.num_objects) {
    L = env_color(sc, ld3(s.dirs + 3ull * i));
  } else {
    const Material& mat = sc.materials[sc.insts[obj].material];
    const bool cov = s.covered[i] != 0;
    const double* __restrict__ v = s.value + 3ull * i;
    const double i0 = cov ? v[0] : s.unbound[0], i1 = cov ? v[1] : s.unbound[1], i2 = cov ? v[2] : s.unbound[2];
    const double e = mat.emittance;
    L = mk(e * mat.color[0] + (mat.color[0] / 3.141592653589793) * i0, e * mat.color[1] + (mat.color[1] / 3.141592653589793) * i1,
           e * mat.color[2] + (mat.color[2] / 3.141592653589793) * i2);
  }
  double* __restrict__ o = out + 3ull * i;
  double a0 = (s.first ? 0.0 : o[0]) + L.x, a1 = (s.first ? 0.0 : o[1]) + L.y, a2 = (s.first ? 0.0 : o[2]) + L.z;
  if (s.last) { // rpt_finish's expression
    a0 = a0 / s.iterations * s.ev_scale; a1 = a1 / s.iterations * s.ev_scale; a2 = a2 / s.iterations * s.ev_scale;
  }
  o[0] = a0; o[1] = a1; o[2] = a2;
}

#ifndef __HIP_DEVICE_COMPILE__
hipError_t gather_rays(hipStream_t st, const double* rays, uint64_t cap, uint32_t m, double* origins, double* dirs) {
  hipLaunchKernelGGL(rpt_views_rays_gather, dim3((m + 255u) / 256u), dim3(256), 0, st, rays, cap, m, origins, dirs);
  return hipGetLastError();
}
hipError_t fold(hipStream_t st, const Scene& sc, uint32_t m, const Sample& s, double* out) {
  hipLaunchKernelGGL(rpt_views_lightmapped_fold, dim3((m + 255u) / 256u), dim3(256), 0, st, sc, m, s, out);
  return hipGetLastError();
}
#endif
