/*
 * rpt_gpu_probe_volume.h — a regular grid of baked SH9 probes read at the caller's points, at the first hits of the caller's
 * rays and in shaded views: rptgpu_sample_probe_volume, rptgpu_lookup_probe_volume, rptgpu_render_views_probe_lit and their
 * _device forms.  Part of rpt_gpu.h, which includes this file behind its own declarations (RptHitQuery's channels, RptView,
 * RptViewQuery, RptLightmapBinding): include rpt_gpu.h, not this file.  The six entry points are additions within ABI version 7
 * and OPTIONAL — a binding detects them by symbol (dlsym "rptgpu_sample_probe_volume") and a library without them is still
 * ABI 7 —, which is why they stand in a file of their own.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_PROBE_VOLUME_H
#define RPT_GPU_PROBE_VOLUME_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_probe_volume.h behind the declarations this file needs"
#endif

/* ---- A PROBE VOLUME.  rptgpu_bake_probes(RPT_PROBE_SH9) writes the radiance around a point as nine SH coefficients per colour;
 * a lightmap (rpt_gpu_lightmap_lookup.h) cannot light what moves on a live handle, because a moved object has no chart that
 * stays true.  A regular grid of such probes, interpolated at the shaded point and convolved with the clamped cosine about its
 * normal, can.  RptProbeVolume describes the grid:
 *   nx, ny, nz  probes per axis, each >= 1;
 *   origin, spacing   probe (i, j, k) stands at origin + (i * spacing[0], j * spacing[1], k * spacing[2]); spacing finite, > 0;
 *   coeffs      [nz][ny][nx][9][3] f64: probe (i, j, k) has index p = (k * ny + j) * nx + i, and coeffs + 27 p is
 *               rptgpu_bake_probes' [9][3] record for it.  So `coeffs` IS that call's [n][27] output for the positions listed
 *               in index order: no copy or transpose lies between a bake and a volume;
 *   valid       [nz][ny][nx] bytes, non-zero = the probe holds a value (one baked inside a wall does not); NULL: every probe
 *               is valid.
 *
 * ARITHMETIC at a point P with direction N under query q.  Everything below is plain f64 with no contraction, IEEE division,
 * and every expression is evaluated in the order written; fmin, fmax, floor are C's.  N is used as given: NOT normalised.
 *  1. Q[a] = P[a] + q.normal_bias * N[a]                                                     (a = 0, 1, 2)
 *  2. per axis a with count n, origin o, spacing h:
 *       g = (Q[a] - o) / h;   s = fmin(fmax(g, 0.0), (double)(n - 1));   i0f = floor(s);   f = s - i0f;
 *       i0 = (int64_t)i0f;   i1 = i0 + 1, and — AFTER f is formed — i1 is clamped to n - 1.
 *     A NaN g takes the fmax's other argument (s = 0).  INSIDE = 1 iff g >= 0.0 && g <= (double)(n - 1) on all three axes (a
 *     NaN fails).  (fx, i_0, i_1), (fy, j_0, j_1), (fz, k_0, k_1) are the three axes' results.
 *  3. the eight taps in the order t = a + 2 b + 4 c, a, b, c in {0, 1}: tap t is probe (i_a, j_b, k_c) with index p_t and
 *       w_t = (X_a * Y_b) * Z_c,   X_0 = 1.0 - fx, X_1 = fx, and Y, Z likewise from fy, fz;
 *     the weight of a tap whose valid byte is 0 is replaced by +0.0;
 *       ws = ((((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5) + w_6) + w_7.
 *  4. Y_j(N), j = 0 .. 8: the nine expressions rptgpu_bake_probes fixes above (Y_0 = 0.28209479177387814, ...), at N as given;
 *       B_j = A_j * Y_j,   A_0 = 3.141592653589793,   A_1 = A_2 = A_3 = 2.0943951023931953,   A_4 .. A_8 = 0.7853981633974483
 *     (the clamped cosine's zonal factors: rpt_amd.probes.sh9_irradiance's).
 *  5. S[j][c] = (((((((w_0 * C_0 + w_1 * C_1) + w_2 * C_2) + w_3 * C_3) + w_4 * C_4) + w_5 * C_5) + w_6 * C_6) + w_7 * C_7),
 *     C_t = coeffs[p_t][j][c].  A tap of weight +0.0 still enters the sum as written: 0.0 * C is +-0.0 for a finite C and NaN
 *     for a NaN or an infinite one.  So a NaN or infinite coefficient makes NaN of every value whose eight taps include it,
 *     valid or not; keep the coefficients of probes that are not valid finite.
 *  6. M[c] = ((((((((B_0 * S[0][c] + B_1 * S[1][c]) + B_2 * S[2][c]) + ... ) + B_8 * S[8][c]   (left to right, j ascending)
 *  7. E[c] = M[c] / ws:  ONE division per channel, not one per coefficient.
 *  8. COVERED iff Q[0..3] and N[0..3] are all finite and ws > 0.  Then VALUE[c] = E[c] — nothing is clamped: SH ringing may
 *     make it negative.  Otherwise VALUE[c] = q.fallback[c].
 *
 * ENTRY POINTS.
 * rptgpu_sample_probe_volume: point i is positions[3i..], direction normals[3i..].  No ray is traced; the handle supplies the
 * device and nothing of its scene is read.  ONE kernel, rpt_probe_volume_sample, one lane per point.  Channels:
 *   VALUE (f64 x 3), COVERED (u8), INSIDE (u8).  Naming another channel is refused.
 * rptgpu_lookup_probe_volume: per ray (rptgpu_first_hits' rays, used as given) with (t, obj, n, P) = rptgpu_first_hits' T, OBJECT,
 * NORMAL and POSITION for it, bit for bit — its query is run unchanged —:
 *       d = (n[0] * dir[0] + n[1] * dir[1]) + n[2] * dir[2];   N = d > 0.0 ? (-n[0], -n[1], -n[2]) : n     (faced to the ray)
 *   and the rule above at (P, N).  A miss (obj < 0) is not covered: VALUE is the fallback, INSIDE 0, POSITION and NORMAL +0.0 —
 *   a result, not an error.  Channels:
 *   T (f64), OBJECT (i32), POSITION (f64 x 3), NORMAL (the faced N, f64 x 3), VALUE, COVERED, INSIDE.
 *   Per piece: rptgpu_first_hits' query into arrays the handle keeps, then ONE kernel, rpt_probe_volume_lookup, one lane per ray.
 *   RptStats advance as for rptgpu_first_hits.  RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured.
 * A channel that `channels` does not name is not computed, its pointer is not read and its array is not written.
 *
 * INDEPENDENCE.  A result depends on its point or ray, the volume and (rays) the scene and on nothing else: not on the other
 * points, on their order, on the pieces the library cuts the call into, on the traversal route.  Input and output arrays must
 * not overlap (not checked).  After a live update the results are those of a handle freshly created from the updated scene.
 * A host caller's volume is staged on the device whole, its points or rays and its results a piece at a time.
 * RPTGPU_VOLUME_PIECE (environment, read per call; tests): the points or rays per piece.  There is no CPU fallback:
 * RPTGPU_E_NO_DEVICE.
 *
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and every array untouched, in this
 * order.  The query: NULL, a wrong struct_size, channels == 0 or an unknown RPT_VOLUME_* bit (rptgpu_sample_probe_volume: any bit
 * but VALUE, COVERED, INSIDE), a non-finite normal_bias, a precision_mode other than RPT_PRECISION_F64_STRICT,
 * RPT_FLAG_PERSISTENT.  The volume: NULL, a wrong struct_size, reserved != 0, a count of 0, a spacing that is not finite and
 * positive or a non-finite origin, NULL coeffs, a probe count whose arrays fit no allocation (more than 2^55 probes).  The arrays:
 * a NULL RptVolumeArrays, a wrong struct_size, reserved != 0, a named channel whose pointer is NULL; NULL inputs with n > 0.
 * The handle: NULL.  RPTGPU_E_COMM for an abandoned handle.  n == 0 returns RPTGPU_OK.
 *
 * NOT IN SCOPE.  Visibility-aware or depth-weighted probes (a probe behind a thin wall leaks: mark it invalid or space the grid
 * to the walls); irregular or nested grids; more than one volume per call; lookups from inside the path tracer; f32 storage;
 * multi-GPU (a caller shards the points); the Rust binding. */
enum {
  RPT_VOLUME_T = 1u, RPT_VOLUME_OBJECT = 2u, RPT_VOLUME_POSITION = 4u, RPT_VOLUME_NORMAL = 8u, RPT_VOLUME_VALUE = 16u,
  RPT_VOLUME_COVERED = 32u, RPT_VOLUME_INSIDE = 64u
};
typedef struct RptProbeVolume {
  uint32_t struct_size;       /* sizeof(RptProbeVolume) */
  uint32_t nx, ny, nz;        /* probes per axis, each >= 1 */
  uint32_t reserved;          /* 0 */
  double origin[3];           /* probe (0, 0, 0) */
  double spacing[3];          /* finite, > 0 */
  const double* coeffs;       /* [nz][ny][nx][9][3] */
  const uint8_t* valid;       /* [nz][ny][nx], or NULL: every probe is valid */
} RptProbeVolume;
typedef struct RptVolumeQuery {
  uint32_t struct_size;       /* sizeof(RptVolumeQuery) */
  uint32_t channels;          /* RPT_VOLUME_* wanted, at least one */
  double normal_bias;         /* Q = P + normal_bias * N; finite */
  double fallback[3];         /* VALUE of a point that is not covered */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* GENERAL_TRAVERSAL, PROFILE_KERNELS honoured (rays); PERSISTENT refused */
} RptVolumeQuery;
typedef struct RptVolumeArrays { /* one array per channel; a channel not named: pointer not read, array not written */
  uint32_t struct_size;       /* sizeof(RptVolumeArrays) */
  uint32_t reserved;          /* 0 */
  double* t;                  /* [n] */
  int32_t* object;            /* [n] */
  double* position;           /* [n][3] */
  double* normal;             /* [n][3] */
  double* value;              /* [n][3] */
  uint8_t* covered;           /* [n] */
  uint8_t* inside;            /* [n] */
} RptVolumeArrays;
int rptgpu_sample_probe_volume(rptgpu_scene* h, uint64_t n, const double* positions /* [n][3] */, const double* normals /* [n][3] */,
                               const RptProbeVolume* volume, const RptVolumeQuery* q, const RptVolumeArrays* out /* host arrays */);
int rptgpu_lookup_probe_volume(rptgpu_scene* h, uint64_t n, const double* origins /* [n][3] */, const double* dirs /* [n][3] */,
                               const RptProbeVolume* volume, const RptVolumeQuery* q, const RptVolumeArrays* out /* host arrays */);
/* The same with the points or rays, the output arrays and the volume's coeffs and valid in device memory (the structs
 * themselves stay in host memory); `stream` and the synchronisation rule are rptgpu_trace_rays_device's (NULL means NO stream,
 * not the null stream). */
int rptgpu_sample_probe_volume_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals,
                                      const RptProbeVolume* d_volume /* host struct, device arrays */, const RptVolumeQuery* q,
                                      const RptVolumeArrays* d_out /* device arrays */, void* stream);
int rptgpu_lookup_probe_volume_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs,
                                      const RptProbeVolume* d_volume /* host struct, device arrays */, const RptVolumeQuery* q,
                                      const RptVolumeArrays* d_out /* device arrays */, void* stream);

/* ---- VIEWS LIT BY LIGHTMAPS WHERE BOUND AND BY THE VOLUME ELSEWHERE.  rptgpu_render_views_probe_lit is
 * rptgpu_render_views_lightmapped (rpt_gpu_lightmap_lookup.h) with ONE change, to the irradiance I of a hit:
 *   I = the lightmap lookup's VALUE under q.filter where that rule says the ray is COVERED (n_bindings == 0 is legal: no ray is);
 *   otherwise, where the volume rule above covers the hit — at (P, N) = rptgpu_first_hits' POSITION and its NORMAL faced to the
 *   ray, with q.normal_bias —, I[c] = E[c] < 0.0 ? 0.0 : E[c]  (SH ringing is cut at zero; a NaN E stays NaN);
 *   otherwise I = q.unbound_irradiance.
 * The rays, the streams, the miss term, L[c] = m.emittance * m.color[c] + (m.color[c] / 3.141592653589793) * I[c], the sample sum,
 * the scale and all three projections are that call's, word for word.
 *
 * ROUTE.  That call's pieces and passes (RPTGPU_VIEWS_PIECE, RPTGPU_LOOKUP_PIECE, and RPTGPU_VOLUME_PIECE caps them too).  Per
 * sample: rpt_raygen_views[_seeded] and rpt_views_rays_gather; rptgpu_first_hits' query for T, OBJECT, NORMAL and POSITION; with
 * bindings, rpt_hit_surface and rpt_lightmap_lookup, all unchanged; then ONE new kernel, rpt_views_probe_lit_merge, which
 * writes the volume's I and COVERED = 1 into the lookup's arrays for every hit the lookup left uncovered and the volume
 * covers; then rpt_views_lightmapped_fold, unchanged.
 *
 * RPTGPU_E_INVALID_ARGUMENT, in this order: rptgpu_render_views' refusals of the RptViewQuery (RPT_FLAG_VIEWS_PERSISTENT too); a
 * NULL RptViewsProbeLitQuery, a wrong struct_size, an unknown filter, a non-finite normal_bias; the volume's refusals (above);
 * NULL out, NULL views with n_views > 0, a frame count that fits no memory; each view's refusals; the bindings'; a NULL handle;
 * the bindings' against the scene.  n_views == 0 returns RPTGPU_OK. */
typedef struct RptViewsProbeLitQuery {
  uint32_t struct_size;          /* sizeof(RptViewsProbeLitQuery) */
  uint32_t filter;               /* RPT_LOOKUP_NEAREST or RPT_LOOKUP_BILINEAR: the lightmaps' */
  double normal_bias;            /* the volume rule's; finite */
  double unbound_irradiance[3];  /* I of a hit neither a lightmap nor the volume covers */
} RptViewsProbeLitQuery;
int rptgpu_render_views_probe_lit(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                  uint32_t n_bindings, const RptLightmapBinding* bindings, const RptProbeVolume* volume,
                                  const RptViewsProbeLitQuery* q, double* out /* host, [n_views][height][width][3] */);
/* The same with `out`, every binding's uvs, map and valid and the volume's coeffs and valid in device memory; `stream` as above. */
int rptgpu_render_views_probe_lit_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                         uint32_t n_bindings, const RptLightmapBinding* d_bindings, const RptProbeVolume* d_volume,
                                         const RptViewsProbeLitQuery* q, void* d_out, void* stream);

#endif /* RPT_GPU_PROBE_VOLUME_H */
