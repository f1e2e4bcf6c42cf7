/*
 * rpt_gpu_hit_surface.h — the surface element behind a ray's first hit: rptgpu_hit_surface and its _device form.  Part of
 * rpt_gpu.h, which includes this file behind its own declarations (RptHitQuery's fields, RptHitArrays' pattern): include
 * rpt_gpu.h, not this file.  The two entry points are additions within ABI version 7 and OPTIONAL — a binding detects them
 * by symbol (dlsym "rptgpu_hit_surface") and a library without them is still ABI 7 —, which is why they stand in a file of
 * their own.  The conventions are rpt_gpu.h's.
 */
#ifndef RPT_GPU_HIT_SURFACE_H
#define RPT_GPU_HIT_SURFACE_H

#ifndef RPT_GPU_H
#error "include rpt_gpu.h: it includes rpt_gpu_hit_surface.h behind the declarations this file needs"
#endif

/* ---- THE SURFACE ELEMENT OF A FIRST HIT.  rptgpu_closest_hit, rptgpu_first_hits, the AOV calls and rptgpu_trace_vertices stop
 * at t, the shading normal and the top-level object.  This call says WHICH triangle of a mesh was hit, WHERE on it, and
 * which child of a group: what a caller needs to look up a texture or any per-vertex or per-triangle attribute at a hit, to
 * map a lightmap texel's hit back to its triangle, to pick a face or an instance, to paint on a mesh.
 *
 * INPUT.  rptgpu_first_hits': ray i is origins[3i..], dirs[3i..] (f64, xyz interleaved), used as given: no normalisation,
 * t_min = 1e-12, no origin offset.  precision_mode and flags as RptHitQuery's.
 *
 * CHANNELS.  One array each in RptSurfaceArrays.  A channel that `channels` does not name is not computed, its pointer is
 * not read and its array is not written.  With (t_i, n_i, obj_i) = what rptgpu_closest_hit returns for ray i:
 *   T            t[i] = t_i, bit for bit (+inf on a miss; a NaN record stays NaN)                                   f64
 *   OBJECT       object[i] = obj_i (-1 on a miss).  A caller joins on T and OBJECT without a second call           i32
 *   CHILD        if object obj_i is a group (KdTree<Box<dyn Bounded>>): the index of its DIRECT child whose intersect
 *                call wrote the record that stands, counted in the group's children list in the caller's order — the
 *                order rptgpu_scene_set_group uses.  Otherwise -1                                                  i32
 *   PRIMITIVE    if the record that stands was written by a Triangle::intersect (mesh.rs:49-82): the index of that
 *                triangle in its own mesh's triangle list in the caller's order — the order rptgpu_scene_set_mesh uses.
 *                The mesh may be the top-level object or a mesh anywhere inside a group.  Otherwise -1             i32
 *   BARYCENTRIC  barycentric[i][0..3] = the (u, v, w) of mesh.rs:71-73 as that call computed them: the weights of v1, v2,
 *                v3, for the ray in the mesh's own space, from the same operations in the same order, so that
 *                normalize(u*n1 + v*n2 + w*n3) is the mesh-space shading normal.  +0.0 three times when
 *                primitive[i] == -1                                                                            f64 x 3
 * A miss: t = +inf, object = child = primitive = -1, barycentrics +0.0.
 * LIMIT.  A hit whose t is NaN (the extended build's MonomialSurface reports one for a vertical ray over a corner of its
 * box) has child = primitive = -1 and barycentrics +0.0, whatever the object: no walk can be cut at a NaN.
 *
 * "THE CALL THAT WROTE THE RECORD THAT STANDS" is the reference's order: of all candidates that would be accepted with the
 * final t, the first one tested wins — mesh.rs:58 rejects `time >= record.time`, so a later equal one loses.  (The one shape
 * whose guard differs, MonomialSurface with `r > record.time`, lets a later equal one win; it has no triangle and is no
 * group, and inside a group the walk keeps that rule: the child named is the last one that wrote.)
 *
 * INDEPENDENCE.  A ray's result depends on that ray and the scene and on nothing else: not on the other rays of the call,
 * on their order, on the pieces the library cuts the call into, on the traversal route (RPT_FLAG_GENERAL_TRAVERSAL).  Input
 * and output arrays must not overlap (not checked).  After a live update (rptgpu_scene_set_objects, _set_mesh, _set_group)
 * the results are those of a handle freshly created from the updated scene.
 *
 * ROUTE AND STATS.  Per piece: rptgpu_first_hits' own query for T and OBJECT, unchanged (rpt_first_hits, or rpt_raygen_rays,
 * the per-tree query and rpt_hits_store) — into the caller's arrays where named, else into a pair the handle keeps —, then
 * ONE kernel, rpt_hit_surface, with one lane per ray: it walks object obj_i alone, in the reference's order, with the record
 * starting at the next double above t_i, and remembers the leaf entry, the (u, v, w) and the top-level child of every accept
 * (DESIGN.md §21 has the argument why the cut walk names the original's winner).  A host caller's piece is staged on the
 * device.  RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured, RPT_FLAG_WAVEFRONT changes nothing,
 * RPT_FLAG_PERSISTENT is refused.  RptStats: kernel_launches[RPT_K_EXTEND] (kernel_ms under RPT_FLAG_PROFILE_KERNELS) and
 * total_ms advance as for rptgpu_first_hits; rpt_hit_surface is counted under no RPT_K_* kind; samples, extend_rays and
 * shadow_rays do not advance.  There is no CPU fallback: RPTGPU_E_NO_DEVICE.  RPTGPU_SURFACE_PIECE (environment, read per
 * call; tests): the rays per piece.
 *
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and every array untouched: a
 * NULL RptSurfaceQuery or RptSurfaceArrays, a wrong struct_size of either, channels == 0 or an unknown RPT_SURFACE_* bit,
 * reserved != 0 in the arrays, a named channel whose pointer is NULL, a precision_mode other than RPT_PRECISION_F64_STRICT,
 * RPT_FLAG_PERSISTENT, NULL origins or dirs with n > 0, a NULL handle.  RPTGPU_E_COMM for an abandoned handle.  n == 0
 * returns RPTGPU_OK.
 *
 * NOT IN SCOPE.  The chain of children between a top-level group and a mesh nested more than one level down: CHILD names
 * the top-level group's child and PRIMITIVE the innermost triangle.  Geometric normals.  These channels in
 * rptgpu_trace_vertices, the AOV calls or the device Buffer.  Multi-hit; multi-GPU (a caller shards the rays: a result
 * depends on nothing else).  The Rust binding. */
enum {
  RPT_SURFACE_T = 1u, RPT_SURFACE_OBJECT = 2u, RPT_SURFACE_CHILD = 4u, RPT_SURFACE_PRIMITIVE = 8u, RPT_SURFACE_BARYCENTRIC = 16u
};
typedef struct RptSurfaceQuery {
  uint32_t struct_size;       /* sizeof(RptSurfaceQuery) */
  uint32_t channels;          /* RPT_SURFACE_* wanted, at least one */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused */
} RptSurfaceQuery;
typedef struct RptSurfaceArrays { /* one array per channel; a channel not named: pointer not read, array not written */
  uint32_t struct_size;       /* sizeof(RptSurfaceArrays) */
  uint32_t reserved;          /* 0 */
  double* t;                  /* [n] */
  int32_t* object;            /* [n] */
  int32_t* child;             /* [n] */
  int32_t* primitive;         /* [n] */
  double* barycentric;        /* [n][3] */
} RptSurfaceArrays;
int rptgpu_hit_surface(rptgpu_scene* h, uint64_t n, const double* origins /* [n][3] */, const double* dirs /* [n][3] */,
                       const RptSurfaceQuery* q, const RptSurfaceArrays* out /* host arrays */);
/* The same with every array in device memory (the two structs stay in host memory); `stream` and the synchronisation rule
 * are rptgpu_trace_rays_device's (NULL means NO stream, not the null stream). */
int rptgpu_hit_surface_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, const RptSurfaceQuery* q,
                              const RptSurfaceArrays* d_out /* device arrays */, void* stream);

#endif /* RPT_GPU_HIT_SURFACE_H */
