/*
 * rpt_gpu_lightmap_filter.h — a baked lightmap denoised on the device with a geometry-guided filter: rptgpu_filter_lightmap
 * and its _device form.  Part of rpt_gpu.h, which includes this file behind rpt_gpu_lightmap.h: include rpt_gpu.h, not this
 * file.  The two entry points are additions within ABI version 7 and OPTIONAL — a binding detects them by symbol (dlsym
 * "rptgpu_filter_lightmap") and a library without them is still ABI 7 —, which is why they stand in a file of their own.
 * The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_LIGHTMAP_FILTER_H
#define RPT_GPU_LIGHTMAP_FILTER_H

#ifndef RPT_GPU_LIGHTMAP_H
#error "include rpt_gpu.h: it includes rpt_gpu_lightmap_filter.h behind rpt_gpu_lightmap.h, whose channels this file names"
#endif

/* ---- A LIGHTMAP FILTER.  rptgpu_bake_lightmap and rptgpu_bake_lightmap_direct return maps that are right to the bit and, at
 * the sample counts a bake can afford, noisy.  This call is rptgpu_buffer_denoise's edge-avoiding a-trous wavelet filter in
 * texel space: its guides are a bake's own OWNER, POSITION and NORMAL channels instead of a camera's feature sums, its
 * plane term is in world units, a texel nobody owns takes part in nothing, and a distance term that grows with the tap
 * spacing keeps two charts apart that sit side by side in the atlas and metres apart in the world.  The handle supplies the
 * device, the stream rule and the error detail; nothing of its scene is read, and the result does not depend on it.
 *
 * INPUT.  W = width, H = height, all arrays row-major over the map.  valid_p = owner_p >= 0.  P_p = position[p][0..3],
 * N_p = normal[p][0..3], c_p = values[p][0..words] — the UNDILATED map: a gutter texel's value is not read —, and, with
 * variance != NULL, u_p = variance[p]: the variance of texel p's mean, summed over its components (rpt_amd.lightmap
 * batch_variance makes one from several bakes).
 *
 * ARITHMETIC.  All of it is IEEE f64, never contracted, every expression evaluated in the order written.  exp is rpt_exp of
 * include/rpt_math.h.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  |d|^2 is dot(d, d) for words == 3 and d*d for words == 1.
 * Every sum starts at +0.0.  Taps are visited dx outer, dy inner, both ascending (rptgpu_buffer_denoise's order).  A tap
 * outside the map is skipped; a tap on a texel that is not valid is skipped.
 *
 * VARIANCE PREFILTER, only with variance.  g(-1) = g(1) = 0.25, g(0) = 0.5.  For every valid p, over the valid
 * q = p + (dx, dy) with dx, dy in -1..1:  a = a + (g(dx)*g(dy)) * u_q,  s = s + g(dx)*g(dy);  v_p = a / s.
 *
 * LEVEL l = 0 .. levels-1, step = 2^l, k(0) = 0.375, k(+-1) = 0.25, k(+-2) = 0.0625.  For every valid p, over
 * q = p + step*(dx, dy) with dx, dy in -2..2 and w0 = k(dx)*k(dy):
 *   the centre tap (dx == 0 && dy == 0) has w = w0; no exponent is evaluated, and c_p is taken whatever it holds;
 *   any other tap is skipped unless every component x of c_q satisfies fabs(x) < +inf.  Otherwise, with D = P_q - P_p
 *   (per component):
 *     t  = 1.0 - dot(N_p, N_q);   en = (t > 0.0 ? t : 0.0) / sigma_normal
 *     ez = fabs(dot(N_p, D)) / sigma_plane
 *     sd = sigma_distance * (double)step;   ed = dot(D, D) / (sd * sd)
 *     e  = (en + ez) + ed
 *     with variance, and d = c_q - c_p (per component):
 *     e  = e + |d|^2 / ((sigma_color*sigma_color) * (v_p + v_q) + 1e-12)
 *   the tap is skipped unless e >= 0.0 && e < +inf (a NaN fails both); otherwise w = w0 * exp(-e);
 *   a tap that is not skipped adds  C = C + w*c_q (per component),  W = W + w,  and with variance  V = V + (w*w)*v_q.
 * Then c'_p = C / W and v'_p = V / (W*W); the next level reads c' and v' for c and v.
 * A texel that is not valid keeps values_p and variance_p bit for bit through every step, and takes part in nothing.
 * So a valid texel whose value is NaN or infinite keeps it (its own centre tap carries it) and hands it to nobody; a
 * texel with a NaN normal or position has no tap but its centre, and is nobody's tap.
 *
 * sigma_distance scales with the step: a tap inside one chart, |D| about step texels, has the same ed at every level,
 * and a tap that jumped a gutter into a chart elsewhere in the world gets none of the weight.  A caller sets it to a few
 * world distances between neighbouring texels (rpt_amd.lightmap texel_extent measures one).
 *
 * OUTPUT.  out is the last level's c' (levels == 0: values) after min(dilate, max(W, H)) rounds of rpt_gpu_lightmap.h's
 * DILATION with FILLED = valid — rptgpu_bake_lightmap's own rounds, so levels == 0 over an undilated bake is that bake with
 * `dilate`.  out_variance, where given, is the last v' (levels == 0: v, the prefilter's result; a texel that is not valid:
 * variance_p), never dilated.  Input arrays are not written.  Inputs and outputs must not overlap (not checked).
 *
 * ROUTE.  Three kernels of their own, one lane per texel in blocks of 64 x 4, no LDS and no atomics:
 * rpt_lightmap_filter_prepare lays the guides down as columns (position and normal three each, a validity byte), computes
 * the prefiltered variance and copies values into the first of two column sets; rpt_lightmap_filter_level runs once per
 * level from one set into the other and loads a tap's validity byte first, nothing else for a skipped tap;
 * rpt_lightmap_filter_finish writes [H][W][words] back.  The dilation is rpt_lightmap_dilate, one launch per round.
 * WORKSPACE, kept by the handle: 8 * (6 + 2*words + (variance ? 2 : 0)) + 1 bytes per texel — 113 B at 3 words with a
 * variance, 97 B without, 81 B and 65 B at 1 word; the dilation's second copy and flags lie inside it.  A host caller's
 * arrays are staged on the device whole beside it (4 + 8 * (6 + 2*words) bytes per texel, + 16 with a variance).
 *
 * STATS.  RptStats::total_ms advances once, by the call's time; nothing else moves.  There is no CPU fallback:
 * RPTGPU_E_NO_DEVICE.
 *
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and every array untouched —
 * the filter first, then the arrays, then the handle: a NULL RptLightmapFilter or a wrong struct_size, width == 0 or
 * height == 0, width*height > 2^32, words other than 1 or 3, levels > 8, a sigma_normal, sigma_plane or sigma_distance that is
 * not finite or not > 0; a NULL RptLightmapFilterArrays or a wrong struct_size, reserved != 0, a NULL owner, position,
 * normal, values or out, an out_variance without a variance, and — it is read only with a variance, so it is checked behind
 * the arrays — a sigma_color that is not finite or not > 0; a NULL handle.  RPTGPU_E_COMM for an abandoned handle.
 *
 * NOT IN SCOPE.  A variance out of the gathers themselves.  Filtering across UV seams.  Chart packing.  SH9 per texel.  Any
 * existing call filtering by default.  The Rust binding.  Multi-GPU. */
typedef struct RptLightmapFilter {
  uint32_t struct_size;   /* sizeof(RptLightmapFilter) */
  uint32_t width, height; /* texels, both > 0, width*height <= 2^32 */
  uint32_t words;         /* components per texel of values / out: 1 (AO) or 3 (irradiance, direct light) */
  uint32_t levels;        /* 0 .. 8 a-trous passes, tap spacing 1, 2, 4, ...; 0 = dilation only */
  uint32_t dilate;        /* gutter-fill rounds after the last level, rpt_gpu_lightmap.h's DILATION */
  double sigma_normal;    /* finite, > 0 */
  double sigma_plane;     /* world units, finite, > 0 */
  double sigma_distance;  /* world units PER TEXEL OF TAP SPACING, finite, > 0 */
  double sigma_color;     /* finite, > 0 when variance != NULL, else not read */
} RptLightmapFilter;
typedef struct RptLightmapFilterArrays {
  uint32_t struct_size;     /* sizeof(RptLightmapFilterArrays) */
  uint32_t reserved;        /* 0 */
  const int32_t* owner;     /* [H][W]   valid_p = owner_p >= 0 (bake_lightmap's OWNER) */
  const double* position;   /* [H][W][3] bake_lightmap's POSITION */
  const double* normal;     /* [H][W][3] bake_lightmap's NORMAL */
  const double* values;     /* [H][W][words] the UNDILATED map to filter */
  const double* variance;   /* [H][W] variance of each texel's mean, summed over components; or NULL */
  double* out;              /* [H][W][words] */
  double* out_variance;     /* [H][W] or NULL; must be NULL when variance is NULL */
} RptLightmapFilterArrays;
int rptgpu_filter_lightmap(rptgpu_scene* h, const RptLightmapFilter* f, const RptLightmapFilterArrays* a /* host arrays */);
/* The same with every array in device memory (the two structs stay in host memory); `stream` and the synchronisation rule
 * are rptgpu_trace_rays_device's (NULL means NO stream, not the null stream). */
int rptgpu_filter_lightmap_device(rptgpu_scene* h, const RptLightmapFilter* f, const RptLightmapFilterArrays* d_a /* device arrays */,
                                  void* stream);

#endif /* RPT_GPU_LIGHTMAP_FILTER_H */
