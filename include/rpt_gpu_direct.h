/*
 * rpt_gpu_direct.h — direct lighting baked on the device: rptgpu_bake_direct at points the caller supplies, and
 * rptgpu_bake_lightmap_direct over a mesh's UV charts, each with its _device form.  Part of rpt_gpu.h, which includes this
 * file behind its own declarations (RptAoQuery's fields, RptLightmapQuery): include rpt_gpu.h, not this file.  The four entry
 * points are additions within ABI version 7 and OPTIONAL — a binding detects them by symbol (dlsym "rptgpu_bake_direct") and a
 * library without them is still ABI 7 —, which is why they stand in a file of their own.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_DIRECT_H
#define RPT_GPU_DIRECT_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_direct.h behind the declarations this file needs"
#endif

/* ---- DIRECT LIGHT AT CALLER POINTS.  rptgpu_bake_probes, rptgpu_bake_ao and rptgpu_bake_lightmap gather, and a gather sees a
 * light only where one of its rays hits something emissive: a Light::Point or Light::Directional is never hit, and a
 * Light::Object is not among the objects a ray can hit, so the light that falls on the point ITSELF is in none of them.  This
 * call is that term: the renderer's next-event estimation (sample_lights, renderer.rs:177-204) at the caller's points, with
 * the light samples drawn by the library from the Philox stream.
 *
 * ARITHMETIC.  Plain f64 with no contraction, IEEE division and square root, and every expression evaluated in the order
 * written.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and normalize(v) = v / sqrt(dot(v, v)) are the project's.
 *
 * Point i: pos = positions[3i..], nn = normalize(normals[3i..]), acc = (+0.0, +0.0, +0.0); S = samples.
 * For k = 0 .. S-1 ascending: the stream is Philox4x32-10 keyed by `seed` with the counter (stream id, sample_index_base + k,
 * draw block), starting at draw 0; the stream id is streams[i], or i (the point's index in this call's arrays) when streams
 * is NULL — rptgpu_bake_ao's rules.  For every light l of the scene in scene order:
 *   Light::Ambient is skipped and takes no draw (it depends on no geometry: a caller adds it).  Otherwise
 *   (I, wi, dist) = Light::illuminate(pos, rng) (light.rs:23-47), continuing the stream where the light before left it.  It
 *       draws whether or not the light faces the point: the stream position never depends on the geometry.
 *   cosv = dot(wi, nn);  c = (I.x * cosv, I.y * cosv, I.z * cosv)
 *   t = what rptgpu_closest_hit returns for the ray (pos, wi), used as given: t_min = 1e-12, NO origin offset, +inf on a
 *       miss, a NaN record stays NaN
 *   if (cosv > 0.0 && t > fmin(dist, 1.7976931348623157e308)) acc = acc + c      (renderer.rs:197; both false for NaN)
 * out[i][c] = acc[c] / (double)S.
 *
 * The unit is irradiance without the 1/pi of a Lambertian surface: a surface's next-event term in the renderer is
 * bsdf * I * (wi . n) per component, so bsdf(material, n, wo, wi) * out reproduces it up to the order of two
 * multiplications.  The point is one-sided: light from below the normal adds nothing.
 *
 * INDEPENDENCE.  A point's result depends on (its position, its normal, seed, its stream id, the sample indices, the scene)
 * and on nothing else: not on the other points, their order, the pieces and passes the library cuts the call into, or the
 * route.  As for rptgpu_bake_ao the rays start AT the points: a caller lifts points off their surface.  A zero or non-finite
 * normal is not refused: cosv is NaN then and the point receives +0.0.  A scene without a non-ambient light gives +0.0
 * everywhere and runs no query.  After a live update the results are those of a handle freshly created from the updated
 * scene.  48 B in (52 B with stream ids) and 24 B out per point, whatever S and the number of lights.
 *
 * ROUTE.  rpt_raygen_direct, a lane per (sample, point) slot at a time, walks the lights and lays each light's wi, dist and c
 * where a depth's shadow rays of that light lie; a slot whose c is exactly zero for a light (cosv > 0 failed, or I is zero) is not
 * queued for it — it could add only +0.0.  The query is a render's own: one rpt_shadow_rays launch with the light as the
 * grid's y for scenes walked in-kernel, the per-tree queries per light for scenes with deep trees;
 * RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured.  rpt_direct_fold, one thread per point, adds sample
 * by sample (outer) and light by light (inner).  RPTGPU_DIRECT_PIECE (environment, read per call; tests): the points per piece.
 *
 * STATS.  shadow_rays advances by n * S * (non-ambient lights), what the reference would cast; shadow_rays_traced by the rays
 * queued; kernel_launches[RPT_K_SHADOW] by the queries; samples does not advance.  There is no CPU fallback:
 * RPTGPU_E_NO_DEVICE.
 *
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and the arrays untouched: a NULL
 * query, a wrong struct_size, samples == 0, a precision_mode other than RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT (the
 * persistent kernel makes its rays from a camera), NULL positions / normals / out with n > 0, more than 2^32 points without
 * stream ids, a NULL handle; RPTGPU_E_COMM for an abandoned handle.  n == 0 returns RPTGPU_OK.
 *
 * NOT IN SCOPE.  Per-light outputs; ambient lights in the sum; the environment's direct term (the gathers carry it);
 * two-sided points; the persistent kernel; multi-GPU (a caller shards the points: a result depends on nothing else). */
typedef struct RptDirectQuery {
  uint32_t struct_size;       /* sizeof(RptDirectQuery) */
  uint32_t samples;           /* S > 0: light samples per point and light */
  uint64_t seed;
  uint64_t sample_index_base; /* sample index of every point's first light sample */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused by name */
} RptDirectQuery;
int rptgpu_bake_direct(rptgpu_scene* h, uint64_t n, const double* positions /* [n][3] */, const double* normals /* [n][3] */,
                       const uint32_t* streams /* [n] or NULL */, const RptDirectQuery* q, double* out /* [n][3], host */);
/* The same with every array in device memory; `stream` and the synchronisation rule are rptgpu_trace_rays_device's (NULL means
 * NO stream, not the null stream). */
int rptgpu_bake_direct_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals,
                              const void* d_streams /* may be NULL */, const RptDirectQuery* q, void* d_out, void* stream);

/* ---- THE LIGHTMAP FORM.  rptgpu_bake_lightmap's triangles, normals and uvs and an RptLightmapQuery, of which width, height,
 * samples (> 0), dilate, stream_base, seed, sample_index_base, offset, precision_mode and flags are read; channels,
 * max_bounces and max_distance are NOT read.  out is one [H][W][3] f64 array.  The owner, the gather point G and the normal n
 * of a texel are rptgpu_bake_lightmap's, by rpt_gpu_lightmap.h's rules.  An owned texel holds bit for bit what
 * rptgpu_bake_direct returns at (G, n) with stream id stream_base + y*W + x and the query's seed, sample_index_base and
 * samples; an unowned texel holds +0.0; dilation follows the lightmap's rule and round count.  The pipeline is the
 * lightmap's — rasterise, compact, gather, scatter, dilate — with rptgpu_bake_direct's driver as the gather.
 * RPT_FLAG_RAYS_PERSISTENT is ignored.  Refusals, before any device work and with the array untouched — the query first, then
 * the array, then the handle: a NULL RptLightmapQuery, a wrong struct_size, width == 0 or height == 0, width*height +
 * stream_base > 2^32, samples == 0, a non-finite offset, a precision_mode other than RPT_PRECISION_F64_STRICT,
 * RPT_FLAG_PERSISTENT; a NULL out; n_tris > 2^31 - 1, NULL positions or uvs with n_tris > 0; a NULL handle.  RPTGPU_E_COMM for
 * an abandoned handle.  n_tris == 0 is legal: every texel holds +0.0. */
int rptgpu_bake_lightmap_direct(rptgpu_scene* h, uint64_t n_tris, const double* positions /* [n][3][3] world space */,
                                const double* normals /* [n][3][3] or NULL */, const double* uvs /* [n][3][2] */,
                                const RptLightmapQuery* q, double* out /* [H][W][3], host */);
int rptgpu_bake_lightmap_direct_device(rptgpu_scene* h, uint64_t n_tris, const void* d_positions, const void* d_normals /* or NULL */,
                                       const void* d_uvs, const RptLightmapQuery* q, void* d_out, void* stream);

#endif /* RPT_GPU_DIRECT_H */
