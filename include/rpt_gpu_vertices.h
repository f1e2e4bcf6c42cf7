/*
 * rpt_gpu_vertices.h — the vertices of the paths rptgpu_trace_rays runs: rptgpu_trace_vertices and its _device form.  Part of
 * rpt_gpu.h, which includes this file behind its own declarations (RptRayQuery's fields, RptHitArrays' pattern): include
 * rpt_gpu.h, not this file.  The two entry points are additions within ABI version 7 and OPTIONAL — a binding detects them
 * by symbol (dlsym "rptgpu_trace_vertices") and a library without them is still ABI 7 —, which is why they stand in a file
 * of their own.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_VERTICES_H
#define RPT_GPU_VERTICES_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_vertices.h behind the declarations this file needs"
#endif

/* ---- PATH VERTICES FOR THE CALLER'S RAYS.  rptgpu_first_hits, rptgpu_occluded and the AOV calls return the start of a path,
 * rptgpu_trace_rays its sum; this call returns what lies between: where every path bounced, what it picked up there, with
 * what BSDF value, pdf and cosine it went on, and where its Philox stream stood — training data for radiance caches and
 * path guiding, callers that shade or re-weight their own hits, finding the depth the firefly clamp cut, drawing light
 * paths, continuing a path later from one of its vertices.
 *
 * INPUT.  rptgpu_trace_rays': n rays (origins, dirs: [n][3] f64, used as given), optional stream ids, and a query with
 * RptRayQuery's fields and meanings plus `channels`, a set of RPT_VERTEX_* bits.
 *
 * INDEXING.  With B = max_bounces, path (i, s) — s = 0 .. iterations-1 — is sample sample_index_base + s of ray i: the SAME
 * stream (seed, stream id, sample index, from draw first_draw on), the same draws and the same path rptgpu_trace_rays runs
 * for that query.  Its vertices are d = 0 .. len-1 with 1 <= len <= B+1: vertex d is where the ray of depth d ended — on a
 * surface, or nowhere.  A per-vertex array `a` is [n][iterations][B+1] (x 3 where stated), a[i][s][d]; `length` is
 * [n][iterations]; `rgb` is [n][3].
 *
 * CHANNELS.  One array each in RptVertexArrays.  A channel that is not named is not computed: its pointer is not read and
 * its array is not written.
 *   LENGTH     length[i][s] = len                                                                            u32
 *   T, NORMAL, OBJECT, POSITION   what rptgpu_first_hits defines for the ray of depth d of that path, (origin_d, dir_d):
 *              t f64 (+inf on a miss), normal f64 x 3, object i32 (-1 on a miss), position f64 x 3 (+0.0 on a miss).
 *              origin_0 = origins[i]; origin_d = position_{d-1} EXACTLY — Ray::at, one multiply then one add, which is
 *              what the estimator respawns from.  A vertex with object == -1 is the escape vertex and is the path's last.
 *   DIRECTION  dir_d, f64 x 3; dir_0 = dirs[i], dir_d = the direction sample_f drew at vertex d-1
 *   DRAW       the draw index at which the path's stream stood when the ray of depth d was made, u32: DRAW[i][s][0] ==
 *              first_draw, and vertex d's shading (the lights' samples, then sample_f) draws from DRAW[i][s][d] on
 *   RADIANCE   A_d, f64 x 3: at a hit, emission plus sample_lights' sum (next-event estimation over every light); at the
 *              escape vertex the environment's colour along dir_d
 *   BSDF, INV_PDF, ABS_COS   the three factors the estimator multiplies when it folds vertex d+1 .. into vertex d: the BSDF
 *              value f_d (f64 x 3) for (wo = -dir_d normalised, wi = dir_{d+1}), 1 / pdf of that sample, |dir_{d+1} . normal_d|
 *              — kept separate so that the fold can be restated to the bit.  Defined for d < len-1; +0.0 at the last vertex.
 *   RGB        rgb[i][0..3] = rptgpu_trace_rays' output for the same query, bit for bit
 * FILLER.  Every entry with d >= len of a named per-vertex channel is written: +0.0, OBJECT -1, DRAW 0.
 *
 * THE FOLD.  L = A_{len-1}; for d = len-2 down to 0: ind = INV_PDF_d * (BSDF_d (.) L) * ABS_COS_d — per component, the
 * products in that order —, L = A_d + fmin(ind, 100) with C's fmin (the other operand for a NaN).  That L is
 * Renderer::trace_ray of the path; summed over s ascending from +0.0, then / iterations * 2^exposure_value, it is rgb[i].
 * The suffix value L_d of the same loop stopped at d is what rptgpu_trace_rays returns for the ray (origin_d, dir_d) with
 * the path's stream id, first_draw = DRAW_d, max_bounces = B - d, iterations = 1, sample_index_base = the path's sample index
 * and exposure_value = 0: a path can be continued from any of its vertices.
 *
 * INDEPENDENCE.  A path's records depend on its ray, seed, its stream id, its sample index, first_draw and the scene, and on
 * nothing else: not on the other rays of the call or their order, on pieces and passes, on a pass that starts over, on the
 * re-ordering of a depth's paths, on the traversal route (RPT_FLAG_GENERAL_TRAVERSAL).  After a live update (rptgpu_scene_set_
 * objects / _lights / _mesh / _group) they are those of a fresh handle on the updated scene.
 *
 * ROUTE AND STATS.  The call runs the wavefront pipeline, as rptgpu_trace_rays does; RPT_FLAG_GENERAL_TRAVERSAL and
 * RPT_FLAG_PROFILE_KERNELS are honoured, RPT_FLAG_WAVEFRONT changes nothing, RPT_FLAG_PERSISTENT is refused.  RptStats
 * advances exactly as for rptgpu_trace_rays (samples = n * iterations; the two kernels that carry the records out are not
 * counted under any RPT_K_* kind).  A library with rpt_gpu_vertices_persistent.h (included at the end of rpt_gpu.h) runs the
 * persistent kernel instead when it is asked to with RPT_FLAG_VERTICES_PERSISTENT: the same bytes in every array, the
 * stats of that kernel.  There is no CPU fallback.  RPTGPU_VERTICES_PIECE (environment, read per call; tests):
 * the rays per piece.
 *
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and every array untouched:
 * everything rptgpu_trace_rays refuses (a NULL query, a wrong struct_size, iterations == 0, max_bounces > 254, a
 * precision_mode other than RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT, NULL origins / dirs with n > 0, more than 2^32
 * rays without stream ids, a NULL handle); channels == 0 or an unknown bit; reserved != 0 in either struct; a NULL
 * RptVertexArrays or a wrong struct_size of it; a named channel whose pointer is NULL; n * iterations * (B+1) >= 2^56 (a
 * per-vertex array's size in bytes would not fit a uint64_t index).  RPTGPU_E_COMM for an abandoned handle.  n == 0
 * returns RPTGPU_OK.
 *
 * NOT IN SCOPE.  Views or camera pixels as the ray source (a caller makes those rays itself: tests/views_model.py shows
 * how); primitive ids or barycentrics per vertex (for a ray's first hit: rptgpu_hit_surface, rpt_gpu_hit_surface.h); the
 * shadow rays' own records (only their sum, inside RADIANCE); light probes; multi-GPU; the device Buffer.  (The persistent kernel: on request, rpt_gpu_vertices_persistent.h.) */
enum {
  RPT_VERTEX_LENGTH = 1u, RPT_VERTEX_T = 2u, RPT_VERTEX_NORMAL = 4u, RPT_VERTEX_OBJECT = 8u, RPT_VERTEX_POSITION = 16u,
  RPT_VERTEX_DIRECTION = 32u, RPT_VERTEX_DRAW = 64u, RPT_VERTEX_RADIANCE = 128u, RPT_VERTEX_BSDF = 256u,
  RPT_VERTEX_INV_PDF = 512u, RPT_VERTEX_ABS_COS = 1024u, RPT_VERTEX_RGB = 2048u
};
typedef struct RptVertexQuery {
  uint32_t struct_size;       /* sizeof(RptVertexQuery) */
  uint32_t max_bounces;       /* B <= 254 */
  uint32_t iterations;        /* samples per ray, > 0 */
  uint32_t first_draw;        /* draw index at which every ray's stream continues (0: a fresh stream) */
  double exposure_value;      /* RGB only */
  uint64_t seed;
  uint64_t sample_index_base; /* index of every ray's first sample */
  uint32_t precision_mode;    /* RPT_PRECISION_* */
  uint32_t flags;             /* as RptRayQuery: GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused; VERTICES_PERSISTENT */
  uint32_t channels;          /* RPT_VERTEX_* wanted, at least one */
  uint32_t reserved;          /* 0 */
} RptVertexQuery;
typedef struct RptVertexArrays { /* one array per channel; a channel not named: pointer not read, array not written */
  uint32_t struct_size;       /* sizeof(RptVertexArrays) */
  uint32_t reserved;          /* 0 */
  uint32_t* length;           /* [n][iterations] */
  double* t;                  /* [n][iterations][B+1] */
  double* normal;             /* [n][iterations][B+1][3] */
  int32_t* object;            /* [n][iterations][B+1] */
  double* position;           /* [n][iterations][B+1][3] */
  double* direction;          /* [n][iterations][B+1][3] */
  uint32_t* draw;             /* [n][iterations][B+1] */
  double* radiance;           /* [n][iterations][B+1][3] */
  double* bsdf;               /* [n][iterations][B+1][3] */
  double* inv_pdf;            /* [n][iterations][B+1] */
  double* abs_cos;            /* [n][iterations][B+1] */
  double* rgb;                /* [n][3] */
} RptVertexArrays;
int rptgpu_trace_vertices(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs,
                          const uint32_t* streams /* may be NULL */, const RptVertexQuery* q,
                          const RptVertexArrays* out /* host arrays */);
/* The same with every array in device memory, read and written where it lies; q and the arrays struct stay in host memory.
 * `stream` and the synchronisation rule are rptgpu_trace_rays_device's (NULL means NO stream, not the null stream). */
int rptgpu_trace_vertices_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs,
                                 const void* d_streams /* may be NULL */, const RptVertexQuery* q,
                                 const RptVertexArrays* d_out /* device arrays */, void* stream);

#endif /* RPT_GPU_VERTICES_H */
