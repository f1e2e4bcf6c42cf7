/*
 * rpt_gpu_lightmap_lookup.h — a baked lightmap read back at the first hits of the caller's rays: rptgpu_lookup_lightmap and its
 * _device form.  Part of rpt_gpu.h, which includes this file behind its own declarations (RptHitQuery's fields, RptSurfaceArrays'
 * pattern): include rpt_gpu.h, not this file.  The two entry points are additions within ABI version 7 and OPTIONAL — a binding
 * detects them by symbol (dlsym "rptgpu_lookup_lightmap") and a library without them is still ABI 7 —, which is why they stand
 * in a file of their own.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_LIGHTMAP_LOOKUP_H
#define RPT_GPU_LIGHTMAP_LOOKUP_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_lightmap_lookup.h behind the declarations this file needs"
#endif

/* ---- A LIGHTMAP AT A HIT.  rptgpu_bake_lightmap, rptgpu_bake_lightmap_direct and rptgpu_filter_lightmap write maps over a mesh's
 * uv charts; rptgpu_hit_surface names the triangle and the barycentrics behind a ray's first hit.  This call joins the two on
 * the device: per ray the first hit, its uv on the mesh's chart, and the map's value there by a stated filter rule.
 *
 * INPUT.  rptgpu_hit_surface's rays: ray i is origins[3i..], dirs[3i..] (f64, xyz interleaved), used as given.  And n_bindings
 * records that each tie one map to one object of the scene:
 *   object      the index of a TOP-LEVEL object whose shape is a mesh, plain or Transformed — the number rptgpu_closest_hit
 *               reports.  A mesh inside a group cannot be named.
 *   n_tris      that mesh's triangle count (checked).
 *   uvs         [n_tris][3][2] f64: uvs[j][k] is the (u, v) of vertex k of triangle j, j counted in the mesh's own triangle list in
 *               the caller's order — the order RPT_SURFACE_PRIMITIVE counts in and rptgpu_scene_set_mesh uses.
 *   map         [height][width][components] f64, components 1 or 3.  Row 0 is at v = 0, as the bake writes it: no flip.
 *   valid       [height][width] bytes, non-zero = the texel holds a value (the bake's owner >= 0, or what a dilation filled); NULL:
 *               every texel is valid.
 *
 * ARITHMETIC.  Everything below is plain f64 with no contraction, IEEE division, and every expression is evaluated in the
 * order written.  W = width, H = height of the ray's binding; fmin, fmax, floor are C's.
 *
 * THE HIT.  (t, obj) = what rptgpu_closest_hit returns for the ray; prim and (u, v, w) = rptgpu_hit_surface's PRIMITIVE and
 * BARYCENTRIC for it, bit for bit.  The ray is BOUND to binding b iff obj == bindings[b].object and prim >= 0.  A miss, a hit on
 * an object no binding names, on a mesh inside a group or on a shape that is no mesh is UNBOUND: a result, not an error.
 *
 * UV of a bound ray, with uvK = uvs[prim][K-1]:  U = (u * uv1[0] + v * uv2[0]) + w * uv3[0],  V = (u * uv1[1] + v * uv2[1]) +
 * w * uv3[1]  (rpt_amd.surface.interpolate's order).
 *
 * RPT_LOOKUP_NEAREST.  x = (int64_t)fmin(fmax(floor(U * (double)W), 0.0), (double)(W - 1)), y likewise from V and H.  The value is
 * map[y][x][c]; the texel counts iff valid[y][x] != 0.
 *
 * RPT_LOOKUP_BILINEAR.  Texel (x, y) has its centre at ((x + 0.5) / W, (y + 0.5) / H), the bake's.
 *   s = fmin(fmax(U * (double)W - 0.5, -1.0), (double)W),  x0f = floor(s),  fx = s - x0f,  x0 = (int64_t)x0f,  x1 = x0 + 1;
 *   t = fmin(fmax(V * (double)H - 0.5, -1.0), (double)H),  y0f = floor(t),  fy = t - y0f,  y0 = (int64_t)y0f,  y1 = y0 + 1;
 *   then — AFTER fx and fy are formed — x0, x1 are clamped to [0, W - 1] and y0, y1 to [0, H - 1]: clamp to edge.
 *   gx = 1.0 - fx,  gy = 1.0 - fy;   w00 = gx * gy,  w10 = fx * gy,  w01 = gx * fy,  w11 = fx * fy   (wXY: tap (xX, yY));
 *   the weight of a tap whose valid byte is 0 is replaced by +0.0;
 *   ws = ((w00 + w10) + w01) + w11;
 *   value[c] = (((w00 * m00[c] + w10 * m10[c]) + w01 * m01[c]) + w11 * m11[c]) / ws,   mXY = map[yY][xX].
 * A tap of weight +0.0 still enters the sum as written: 0.0 * m is +-0.0 for a finite texel and NaN for a NaN or an infinite
 * one.  So a NaN or infinite texel makes NaN of every value whose four taps include it, valid or not; keep the texels that are
 * not valid finite (the bake writes +0.0 there).  A NaN U or V takes the fmax's other argument: the taps stay inside the map.
 *
 * COVERED.  The ray is COVERED iff it is bound, U and V are finite, and ws > 0 (NEAREST: the texel is valid).  Otherwise
 * value[c] = q.fallback[c].  A map of one component writes its scalar to all three.
 *
 * CHANNELS.  One array each in RptLookupArrays.  A channel that `channels` does not name is not computed, its pointer is not
 * read and its array is not written.
 *   T, OBJECT   rptgpu_hit_surface's: t (+inf on a miss) and obj (-1), to join on                              f64, i32
 *   BINDING     the index b of the ray's binding in the caller's list; -1 if unbound                                i32
 *   COVERED     1 or 0                                                                                              u8
 *   UV          (U, V) as computed, covered or not; +0.0 twice if unbound                                      f64 x 2
 *   VALUE       value[0..3]                                                                                    f64 x 3
 *
 * INDEPENDENCE.  A ray's result depends on that ray, the bindings and the scene and on nothing else: not on the other rays, on
 * their order, on the pieces the library cuts the call into, on the traversal route (RPT_FLAG_GENERAL_TRAVERSAL).  Input and
 * output arrays must not overlap (not checked).  After a live update the results are those of a handle freshly created from
 * the updated scene.
 *
 * ROUTE AND STATS.  Per piece: rptgpu_first_hits' own query for T and OBJECT and rpt_hit_surface for PRIMITIVE and BARYCENTRIC,
 * both unchanged, into arrays the handle keeps (T and OBJECT into the caller's where named); then ONE kernel, rpt_lightmap_lookup,
 * with one lane per ray.  The object-to-binding table (one int32 per top-level object) and the binding records are made on the
 * host per call.  A host caller's uvs, maps and valid bytes are staged on the device whole, its rays and results a piece at a
 * time.  RptStats advance as for rptgpu_hit_surface.  RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured,
 * RPT_FLAG_PERSISTENT is refused.  There is no CPU fallback: RPTGPU_E_NO_DEVICE.  RPTGPU_LOOKUP_PIECE (environment, read per
 * call; tests): the rays per piece.
 *
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and every array untouched, in this
 * order.  The query: NULL, a wrong struct_size, channels == 0 or an unknown RPT_LOOKUP_* bit, an unknown filter, a
 * precision_mode other than RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT.  The arrays: a NULL RptLookupArrays, a wrong
 * struct_size, reserved != 0, a named channel whose pointer is NULL; NULL origins or dirs with n > 0.  The bindings: NULL with
 * n_bindings > 0, and per binding a wrong struct_size, reserved != 0, width or height of 0, components not 1 or 3, NULL uvs or
 * map, two bindings naming one object.  The handle: NULL — and then, against its scene, a binding whose object is out of range
 * or no top-level mesh, or whose n_tris is not that mesh's triangle count.  RPTGPU_E_COMM for an abandoned handle.  n == 0
 * returns RPTGPU_OK; n_bindings == 0 is legal (every ray is unbound).
 *
 * A host caller whose bindings' sizes no allocation could hold (more than 2^60 f64 words staged) is refused likewise, with
 * the bindings.
 *
 * NOT IN SCOPE.  Mip-maps or any minification filter; wrap modes other than clamp; meshes inside groups; f32 output; lookups
 * from inside the path tracer; multi-GPU (a caller shards the rays); the Rust binding. */
enum {
  RPT_LOOKUP_T = 1u, RPT_LOOKUP_OBJECT = 2u, RPT_LOOKUP_BINDING = 4u, RPT_LOOKUP_COVERED = 8u, RPT_LOOKUP_UV = 16u,
  RPT_LOOKUP_VALUE = 32u
};
enum { RPT_LOOKUP_NEAREST = 0u, RPT_LOOKUP_BILINEAR = 1u };
typedef struct RptLightmapBinding {
  uint32_t struct_size;       /* sizeof(RptLightmapBinding) */
  uint32_t object;            /* a top-level mesh object of the scene */
  uint32_t n_tris;            /* its triangle count */
  uint32_t width, height;     /* of the map, each >= 1 */
  uint32_t components;        /* 1 or 3 */
  uint32_t reserved;          /* 0 */
  const double* uvs;          /* [n_tris][3][2] */
  const double* map;          /* [height][width][components] */
  const uint8_t* valid;       /* [height][width], or NULL: every texel is valid */
} RptLightmapBinding;
typedef struct RptLookupQuery {
  uint32_t struct_size;       /* sizeof(RptLookupQuery) */
  uint32_t channels;          /* RPT_LOOKUP_* wanted, at least one */
  uint32_t filter;            /* RPT_LOOKUP_NEAREST or RPT_LOOKUP_BILINEAR */
  double fallback[3];         /* VALUE of a ray that is not covered */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused */
} RptLookupQuery;
typedef struct RptLookupArrays { /* one array per channel; a channel not named: pointer not read, array not written */
  uint32_t struct_size;       /* sizeof(RptLookupArrays) */
  uint32_t reserved;          /* 0 */
  double* t;                  /* [n] */
  int32_t* object;            /* [n] */
  int32_t* binding;           /* [n] */
  uint8_t* covered;           /* [n] */
  double* uv;                 /* [n][2] */
  double* value;              /* [n][3] */
} RptLookupArrays;
int rptgpu_lookup_lightmap(rptgpu_scene* h, uint64_t n, const double* origins /* [n][3] */, const double* dirs /* [n][3] */,
                           uint32_t n_bindings, const RptLightmapBinding* bindings, const RptLookupQuery* q,
                           const RptLookupArrays* out /* host arrays */);
/* The same with the rays, the output arrays and every binding's uvs, map and valid in device memory (the structs themselves
 * stay in host memory); `stream` and the synchronisation rule are rptgpu_trace_rays_device's (NULL means NO stream, not the
 * null stream). */
int rptgpu_lookup_lightmap_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, uint32_t n_bindings,
                                  const RptLightmapBinding* d_bindings /* host structs, device arrays */, const RptLookupQuery* q,
                                  const RptLookupArrays* d_out /* device arrays */, void* stream);

/* ---- VIEWS SHADED FROM A BAKE.  rptgpu_render_views_lightmapped: a batch of views whose first hits are shaded from the bound
 * maps, a diffuse surface under a baked irradiance, per SAMPLE — with jitter, albedo * irradiance has to be formed inside
 * the sample sum.
 *
 * RptView, RptViewQuery and the ray of (view v, pixel p, sample s) are EXACTLY rptgpu_render_views': all three projections, the
 * stream keyed by seed + v * seed_stride with counter (p, sample_index_base + s, .).  max_bounces is not read.
 * Per sample, with (t, obj) the ray's first hit:
 *   a miss:  L = the environment's colour for the ray's direction — what rptgpu_trace_rays returns for that ray at
 *            max_bounces = 0;
 *   a hit on an object with material m:  I = the lookup's VALUE under q.filter when the ray is COVERED (the rule above), else
 *            q.unbound_irradiance;   L[c] = m.emittance * m.color[c] + (m.color[c] / 3.141592653589793) * I[c]
 *            (the reference's emission, renderer.rs:153, plus its Lambert term, material.rs:170, under a baked irradiance).
 * out[v][p][c] = (the sum over s ascending, from +0.0, of L[c]) / (double)iterations * 2^exposure_value — rptgpu_render_views'
 * expressions.  Output: f64, [n_views][height][width][3].
 *
 * ROUTE.  In pieces of consecutive (view, pixel) indices (RPTGPU_VIEWS_PIECE, and RPTGPU_LOOKUP_PIECE caps them too: tests),
 * one sample per pass: rptgpu_render_views' own first step (rpt_raygen_views[_seeded], unchanged) makes the rays, rpt_views_rays_gather lays them out interleaved, the
 * ray form's three steps follow, and rpt_views_lightmapped_fold adds the sample to the sums it keeps in `out` between passes
 * (the last pass scales).  RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured.
 *
 * RPTGPU_E_INVALID_ARGUMENT, in this order: rptgpu_render_views' refusals of the RptViewQuery (RPT_FLAG_VIEWS_PERSISTENT too); a
 * NULL RptViewsLightmapQuery, a wrong struct_size, an unknown filter; NULL out, NULL views with n_views > 0, a frame count
 * that fits no memory; each view's refusals; the bindings' (above); a NULL handle; the bindings' against the scene.
 * n_views == 0 returns RPTGPU_OK. */
typedef struct RptViewsLightmapQuery {
  uint32_t struct_size;          /* sizeof(RptViewsLightmapQuery) */
  uint32_t filter;               /* RPT_LOOKUP_NEAREST or RPT_LOOKUP_BILINEAR */
  double unbound_irradiance[3];  /* I of a hit that is not covered */
} RptViewsLightmapQuery;
int rptgpu_render_views_lightmapped(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                    uint32_t n_bindings, const RptLightmapBinding* bindings, const RptViewsLightmapQuery* q,
                                    double* out /* host, [n_views][height][width][3] */);
/* The same with `out` and every binding's uvs, map and valid in device memory; `stream` as above. */
int rptgpu_render_views_lightmapped_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                           uint32_t n_bindings, const RptLightmapBinding* d_bindings,
                                           const RptViewsLightmapQuery* q, void* d_out, void* stream);

#endif /* RPT_GPU_LIGHTMAP_LOOKUP_H */
