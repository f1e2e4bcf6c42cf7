/*
 * rpt_gpu_lightmap.h — a lightmap baked on the device: rptgpu_bake_lightmap and its _device form.  Part of rpt_gpu.h, which
 * includes this file behind its own declarations (RptProbeQuery's and RptAoQuery's fields, RptHitArrays' pattern): include
 * rpt_gpu.h, not this file.  The two entry points are additions within ABI version 7 and OPTIONAL — a binding detects them by
 * symbol (dlsym "rptgpu_bake_lightmap") and a library without them is still ABI 7 —, which is why they stand in a file of
 * their own.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_LIGHTMAP_H
#define RPT_GPU_LIGHTMAP_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_lightmap.h behind the declarations this file needs"
#endif

/* ---- A LIGHTMAP.  rptgpu_bake_probes and rptgpu_bake_ao gather at points the caller supplies.  This call takes the mesh's UV
 * charts instead: it rasterises the triangles' uv coordinates into a width x height map, interpolates a position and a normal
 * at every covered texel's centre, gathers irradiance and / or ambient occlusion there with the two calls' own drivers, and
 * fills the charts' gutters — all on the device, and each step by a stated rule.
 *
 * INPUT.  n_tris triangles in WORLD space: positions[j][k][c] is coordinate c of vertex k of triangle j, normals[j][k][c] its
 * shading normal (NULL: flat, see NORMAL), uvs[j][k][0..2] its (u, v).
 *
 * ARITHMETIC.  Everything below is plain f64 with no contraction, IEEE division and square root, and every expression is
 * evaluated in the order written.  W = width, H = height.
 *
 * TEXEL SPACE.  Vertex k of triangle j is A_k = (uv[j][k][0] * (double)W, uv[j][k][1] * (double)H).  Texel (x, y) has its
 * centre at c = (x + 0.5, y + 0.5), which is exact.  Row 0 is v = 0: there is no flip.
 *
 * EDGE FUNCTION.  e(P, Q, c) = (Q.x - P.x) * (c.y - P.y) - (Q.y - P.y) * (c.x - P.x).
 *
 * COVERAGE.  area = e(A1, A2, A3).  A triangle with area == 0, a non-finite area or a non-finite texel-space vertex covers
 * nothing.  Otherwise e1 = e(A2, A3, c), e2 = e(A3, A1, c), e3 = e(A1, A2, c); for area > 0 the triangle covers the texel iff
 * e1 >= 0 && e2 >= 0 && e3 >= 0, for area < 0 iff all three are <= 0.  Edges are inclusive; mirrored charts work.
 *
 * OWNER.  The owner of a texel is the LOWEST triangle index that covers it; a texel nobody covers has owner -1.  UVs outside
 * [0, 1] are legal: the part of a chart that falls outside the map owns nothing.
 *
 * BARYCENTRICS of an owned texel: b = (e1 / area, e2 / area, e3 / area) — three divisions, not 1 - b1 - b2.
 *
 * POSITION.  P[c] = (b1 * p1[c] + b2 * p2[c]) + b3 * p3[c].
 *
 * NORMAL.  m[c] = (b1 * n1[c] + b2 * n2[c]) + b3 * n3[c]; n = m / sqrt((m.x*m.x + m.y*m.y) + m.z*m.z) (the project's
 * normalize).  With normals == NULL, m is instead the cross product of p2 - p1 and p3 - p1 in Triangle::from_vertices'
 * order (mesh.rs:27): with a = p2 - p1 and b = p3 - p1, m = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).  A zero
 * or non-finite m yields whatever that yields; it is not refused.
 *
 * GATHER POINT.  G[c] = P[c] + offset * n[c].  The POSITION channel reports G, the point the paths start from; the NORMAL
 * channel reports n.
 *
 * CHANNELS.  One array each in RptLightmapArrays, row-major [H][W]; a channel that `channels` does not name is not
 * computed, its pointer is not read and its array is not written.
 *   IRRADIANCE   of an owned texel: bit for bit what rptgpu_bake_probes returns for RPT_PROBE_IRRADIANCE, position G,
 *                normal n, streams[i] = stream_base + y*W + x and the query's seed, sample_index_base, samples and
 *                max_bounces                                                                                    f64 x 3
 *   AO           of an owned texel: what rptgpu_bake_ao returns for the same point, normal, stream id, seed,
 *                sample_index_base, samples and max_distance                                                        f64
 *   OWNER        the owner                                                                                          i32
 *   BARYCENTRIC  b                                                                                              f64 x 3
 *   POSITION     G                                                                                              f64 x 3
 *   NORMAL       n                                                                                              f64 x 3
 * UNOWNED TEXELS.  Before dilation every channel holds +0.0 (OWNER -1).
 *
 * DILATION applies to IRRADIANCE and AO only.  A texel is FILLED if it is owned.  In each of `dilate` rounds every unfilled
 * texel with at least one filled texel among its up-to-8 in-map neighbours takes, per component, acc / (double)count, where
 * acc starts at +0.0 and adds the filled neighbours in the order dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner) and count is
 * their number; that texel counts as filled from the next round on.  A round reads only the previous round's state
 * (ping-pong).  OWNER, BARYCENTRIC, POSITION and NORMAL are never dilated.  After max(W, H) rounds nothing is left to fill and
 * further rounds change no bit: the library runs min(dilate, max(W, H)) of them, so a large `dilate` means "fill everything".
 *
 * INDEPENDENCE.  An owned texel's undilated result depends on its owner triangle's nine positions, nine normals and six uv
 * values, on W and H, on seed, its stream id and the sample indices, on offset, max_bounces or max_distance, and on the
 * scene — not on the other triangles beyond the owner rule, not on the pieces or passes the library cuts the map into, not
 * on the route.  Input and output arrays must not overlap (not checked).  After a live update the results are those of a
 * handle freshly created from the updated scene.
 *
 * ROUTE.  rpt_lightmap_owners rasterises: every triangle's clamped bounding box of texels is tested with the rule above
 * and ownership is claimed with an integer atomicMin on the triangle index, which is order-independent.  The rule is the
 * rounded edge tests and nothing else: a SLIVER — vertices collinear up to rounding, an area that is tiny but not zero —
 * passes them at centres along its line beyond its vertices, and owns those texels too; the library tests the whole map for
 * such a triangle (|area| within 2^-46 of the magnitude of its terms), which costs a pass over the map each.  Then, per piece of
 * consecutive texels in row-major order (the probe call's pass target bounds a piece; RPTGPU_LIGHTMAP_PIECE — environment,
 * read per call; tests — overrides it): rpt_lightmap_texels recomputes e1..e3 / area from the owner, writes the raw
 * channels and appends (G, n, stream id) of the owned texels to compacted arrays in ascending texel order (52 B per owned
 * texel); rptgpu_bake_probes' and rptgpu_bake_ao's own drivers run over those; rpt_lightmap_scatter writes the results to
 * their texels and +0.0 elsewhere.  rpt_lightmap_dilate runs once per round over the whole map.  The owner map (4 B per
 * texel) is kept for the whole call; a host caller's triangles and named channels are staged on the device whole.
 *
 * FLAGS.  RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured.  RPT_FLAG_RAYS_PERSISTENT is passed to the
 * irradiance gather (a library that exports rptgpu_rays_persistent_supported) and masked out for the AO gather: the same
 * bits.  RPT_FLAG_PERSISTENT is refused by name.
 *
 * STATS.  RptStats advances as the inner probe and AO gathers advance it; total_ms advances once, by the call's time.  The
 * new kernels are counted under no RPT_K_* kind.  There is no CPU fallback: RPTGPU_E_NO_DEVICE.
 *
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and every array untouched —
 * the query first, then the arrays, then the handle: a NULL RptLightmapQuery or RptLightmapArrays, a wrong struct_size of
 * either, channels == 0 or an unknown RPT_LIGHTMAP_* bit, width == 0 or height == 0, width*height + stream_base > 2^32,
 * samples == 0 with IRRADIANCE or AO named, max_bounces > 254, a non-finite offset, a precision_mode other than
 * RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT (and RPT_FLAG_RAYS_PERSISTENT | RPT_FLAG_WAVEFRONT, as rptgpu_bake_probes);
 * reserved != 0 in the arrays, a named channel whose pointer is NULL; n_tris > 2^31 - 1, NULL positions or uvs with
 * n_tris > 0; a NULL handle.  RPTGPU_E_COMM for an abandoned handle.  n_tris == 0 is legal: every texel is unowned, the
 * arrays are written with the unowned values and the call returns RPTGPU_OK.
 *
 * NOT IN SCOPE.  Conservative or super-sampled rasterisation: the centre decides, dilation is the remedy.  Object
 * transforms: the caller passes world-space triangles.  Chart packing or unwrapping.  SH9 per texel.  Multi-GPU: a caller
 * splits the map by stream_base and rows.  The Rust binding.  Textures read by the renderer. */
enum {
  RPT_LIGHTMAP_IRRADIANCE = 1u, RPT_LIGHTMAP_AO = 2u, RPT_LIGHTMAP_OWNER = 4u, RPT_LIGHTMAP_BARYCENTRIC = 8u,
  RPT_LIGHTMAP_POSITION = 16u, RPT_LIGHTMAP_NORMAL = 32u
};
typedef struct RptLightmapQuery {
  uint32_t struct_size;       /* sizeof(RptLightmapQuery) */
  uint32_t channels;          /* RPT_LIGHTMAP_* wanted, at least one */
  uint32_t width, height;     /* texels, both > 0, width*height <= 2^32 - stream_base */
  uint32_t samples;           /* as RptProbeQuery / RptAoQuery; > 0 if IRRADIANCE or AO is named, else not read */
  uint32_t max_bounces;       /* IRRADIANCE: as RptProbeQuery, <= 254 */
  uint32_t dilate;            /* gutter-fill rounds, 0 = none */
  uint32_t stream_base;       /* texel (x, y) uses stream id stream_base + y*width + x */
  uint64_t seed, sample_index_base;
  double offset;              /* the gather point is lifted by offset * normal; finite */
  double max_distance;        /* AO only: RptAoQuery's */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* GENERAL_TRAVERSAL, PROFILE_KERNELS, RAYS_PERSISTENT honoured; PERSISTENT refused */
} RptLightmapQuery;
typedef struct RptLightmapArrays { /* one array per channel; a channel not named: pointer not read, array not written */
  uint32_t struct_size;       /* sizeof(RptLightmapArrays) */
  uint32_t reserved;          /* 0 */
  double* irradiance;         /* [H][W][3] */
  double* ao;                 /* [H][W] */
  int32_t* owner;             /* [H][W] */
  double* barycentric;        /* [H][W][3] */
  double* position;           /* [H][W][3] */
  double* normal;             /* [H][W][3] */
} RptLightmapArrays;
int rptgpu_bake_lightmap(rptgpu_scene* h, uint64_t n_tris, const double* positions /* [n][3][3] world space */,
                         const double* normals /* [n][3][3] or NULL */, const double* uvs /* [n][3][2] */,
                         const RptLightmapQuery* q, const RptLightmapArrays* out /* host arrays */);
/* The same with every array in device memory (the two structs stay in host memory); `stream` and the synchronisation rule
 * are rptgpu_trace_rays_device's (NULL means NO stream, not the null stream). */
int rptgpu_bake_lightmap_device(rptgpu_scene* h, uint64_t n_tris, const void* d_positions, const void* d_normals /* or NULL */,
                                const void* d_uvs, const RptLightmapQuery* q, const RptLightmapArrays* d_out /* device arrays */,
                                void* stream);

#endif /* RPT_GPU_LIGHTMAP_H */
