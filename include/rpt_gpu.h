/*
 * rpt_gpu.h — C ABI of the MI355X (gfx950) path-tracing back-end for the `rpt` renderer.
 *
 * This is the drop-in boundary for rpt's one hot path: the body of
 * `Renderer::sample(&self, iterations, &mut Buffer)` (reference src/renderer.rs:117-129),
 * which both public entry points call (`render` renderer.rs:96-100, `iterative_render`
 * renderer.rs:103-115).  The reference has no FFI of its own (`#![forbid(unsafe_code)]`,
 * src/lib.rs:3); the entry points below are what an `rpt-gpu-sys` style binding would bind
 * (see INTEGRATION.md for the Rust / ctypes / C++ stubs).
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no C++/torch types;
 *   - every POD struct mirrors a reference struct field by field (cited per struct);
 *   - matrices are column-major, exactly as nalgebra/glm stores them
 *     (element (row r, col c) of a 4x4 is m[c*4+r], of a 3x3 is m[c*3+r]);
 *   - every function returns 0 (RPTGPU_OK) or a negative RPTGPU_E_* code, never throws,
 *     never aborts; rptgpu_strerror() / rptgpu_last_error_detail() explain;
 *   - the caller owns every input pointer and every output buffer for the duration of the
 *     call only; the library copies what it needs to device memory in rptgpu_scene_create;
 *   - a handle is NOT re-entrant (one render in flight per handle); distinct handles may be
 *     used from distinct threads.  All calls are synchronous unless they take a stream.
 */
#ifndef RPT_GPU_H
#define RPT_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPTGPU_ABI_VERSION 7

/* ---- error codes (replace the reference's panics: buffer.rs:26,33,89, plane.rs:35) ---- */
enum {
  RPTGPU_OK = 0,
  RPTGPU_E_INVALID_ARGUMENT = -1,
  RPTGPU_E_UNSUPPORTED_SHAPE = -2, /* shape outside the closed device set          */
  RPTGPU_E_NO_DEVICE = -3,         /* no HIP device / HIP runtime failure at init              */
  RPTGPU_E_HIP = -4,               /* a HIP call failed; see rptgpu_last_error_detail          */
  RPTGPU_E_OUT_OF_MEMORY = -5,
  RPTGPU_E_TREE_TOO_DEEP = -6,     /* (not returned for any input since ABI v5; internal check)  */
  RPTGPU_E_UNIMPLEMENTED_SAMPLE = -7, /* Light::Object over a Plane: plane.rs:34-36 panics     */
  RPTGPU_E_COMM = -8               /* RCCL is not available or a collective failed             */
};

/* ---- Material: src/material.rs:8-26 ---- */
typedef struct RptMaterial {
  double color[3];
  double index;
  double roughness;
  double metallic;
  double emittance;
  int32_t transparent; /* bool */
  int32_t _pad;
} RptMaterial;

/* ---- Triangle: src/shape/mesh.rs:8-22 (three vertices, three normals) ---- */
typedef struct RptTriangle {
  double v1[3], v2[3], v3[3];
  double n1[3], n2[3], n3[3];
} RptTriangle;

/* ---- Transformed<T>: src/shape.rs:101-108, the five precomputed fields ---- */
typedef struct RptTransform {
  double transform[16];         /* M                                 shape.rs:103 */
  double linear[9];             /* mat4_to_mat3(M)                   shape.rs:104 */
  double inverse_transform[16]; /* glm::inverse(M)                   shape.rs:105 */
  double normal_transform[9];   /* glm::inverse_transpose(linear)    shape.rs:106 */
  double scale;                 /* linear.determinant()              shape.rs:107 */
} RptTransform;

/* The closed set of shapes the device understands (the reference's `dyn Shape` is open). */
enum {
  RPT_SHAPE_SPHERE = 0, /* src/shape/sphere.rs:9    unit sphere at the origin                 */
  RPT_SHAPE_PLANE = 1,  /* src/shape/plane.rs:7-13  x . normal = value                        */
  RPT_SHAPE_CUBE = 2,   /* src/shape/cube.rs:8      unit cube [-0.5,0.5]^3                    */
  RPT_SHAPE_MESH = 3,   /* src/shape/mesh.rs:102    Mesh = KdTree<Triangle>                   */
  RPT_SHAPE_GROUP = 4,  /* KdTree<Box<dyn Bounded>> (examples/fractal_spheres.rs:45,
                           fractal_teapots.rs:69).  Children: anything Bounded — SPHERE, CUBE, MESH,
                           MONOMIAL, or another GROUP — each optionally Transformed (a PLANE is not
                           Bounded, kdtree.rs:9-12, and is refused).  MESH children that share one
                           triangle array (Arc<Mesh>) share one tree on the device.  NESTING: GROUPs may
                           contain GROUPs to any depth, as in the reference (kdtree.rs:14-24 forwards
                           Bounded through Box).  A group with tree children is walked by the per-tree
                           kernels of the wavefront pipeline (two regular levels in one loop, anything else
                           by the generic walker); RPT_FLAG_PERSISTENT is ignored for such a scene.  Only a
                           Light::Object's shape keeps a limit: eight group levels (Shape::sample) */
  RPT_SHAPE_MONOMIAL = 5 /* src/shape/monomial_surface.rs:12-18  y = height*(x^2+z^2)^(exp/2),
                            x^2+z^2 <= 1; like the reference, intersection and normals are
                            only valid for exp = 4 (monomial_surface.rs:10): any other exp is
                            refused.  As a top-level object, a Light::Object, or a GROUP child  */
};

typedef struct RptShape {
  int32_t kind;        /* RPT_SHAPE_*                                                          */
  int32_t transformed; /* 1 = wrapped in Transformed<T> (shape.rs:101), xf is valid            */
  RptTransform xf;
  double plane_normal[3]; /* PLANE: plane.rs:9  */
  double plane_value;     /* PLANE: plane.rs:12 */
  double monomial_height; /* MONOMIAL: monomial_surface.rs:15 */
  double monomial_exp;    /* MONOMIAL: monomial_surface.rs:17 (must be 4) */
  const RptTriangle* triangles; /* MESH: KdTree<Triangle>::objects (kdtree.rs:102)             */
  uint64_t num_triangles;
  const struct RptShape* children; /* GROUP: KdTree<Box<dyn Bounded>>::objects                 */
  uint64_t num_children;
} RptShape;

/* ---- Object: src/object.rs:10-16 (one shape, one material) ---- */
typedef struct RptObject {
  RptShape shape;
  RptMaterial material;
} RptObject;

/* ---- Light: src/light.rs:7-19 ---- */
enum {
  RPT_LIGHT_POINT = 0,       /* Point(color, location)        */
  RPT_LIGHT_AMBIENT = 1,     /* Ambient(color)                */
  RPT_LIGHT_DIRECTIONAL = 2, /* Directional(color, direction) */
  RPT_LIGHT_OBJECT = 3       /* Object(Object)                */
};

typedef struct RptLight {
  int32_t kind;
  int32_t _pad;
  double color[3];
  double vec[3];    /* POINT: location; DIRECTIONAL: direction (not normalised by the caller) */
  RptObject object; /* OBJECT */
} RptLight;

/* ---- Environment: src/environment.rs:56-62, Hdri: environment.rs:5-15 ---- */
enum { RPT_ENV_COLOR = 0, RPT_ENV_HDRI = 1 };

typedef struct RptEnvironment {
  int32_t kind;
  int32_t _pad;
  double color[3];      /* COLOR */
  uint32_t width;       /* HDRI  */
  uint32_t height;      /* HDRI  */
  const double* texels; /* HDRI: width*height*3 doubles, row-major, row 0 = polar angle 0
                           (environment.rs:14 `buf: Vec<Color>`)                              */
} RptEnvironment;

/* ---- Scene: src/scene.rs:7-16 ---- */
typedef struct RptScene {
  const RptObject* objects;
  uint64_t num_objects;
  const RptLight* lights;
  uint64_t num_lights;
  RptEnvironment environment;
} RptScene;

/* ---- Camera: src/camera.rs:8-26 ---- */
typedef struct RptCamera {
  double eye[3];
  double direction[3];
  double up[3];
  double fov;
  double aperture;
  double focal_distance;
} RptCamera;

/* Arithmetic modes.  STRICT is the parity mode and the only one: IEEE f64, no FMA contraction, true
 * divisions — the arithmetic of the reference (Rust never contracts).  ABI versions <= 3 also had
 * F64_FAST = 1 (the same kernels with contraction allowed): it measured SLOWER than STRICT and was not
 * bit-exact, so it was removed; the value 1 is now refused with RPTGPU_E_INVALID_ARGUMENT.  */
enum {
  RPT_PRECISION_F64_STRICT = 0
};

enum {
  RPT_FLAG_PROFILE_KERNELS = 1u, /* bracket every kernel with HIP events (rptgpu_get_stats) */
  RPT_FLAG_GENERAL_TRAVERSAL = 4u, /* tests: always use the general (box-carrying, scratch-stack)
                                      kd traversal instead of the compact LDS-stack one */
  RPT_FLAG_WAVEFRONT = 2u,       /* force the multi-kernel wavefront pipeline (raygen / extend / shade /
                                    shadow / resolve; path state in HBM, lean 4-waves/SIMD traversal
                                    kernels with LDS stacks) */
  RPT_FLAG_PERSISTENT = 8u,      /* force the persistent path kernel (whole path in registers).
                                    With neither flag the library picks: wavefront when the scene has
                                    real kd-trees (depth >= 3: traversal latency dominates and wants
                                    occupancy), persistent otherwise.  Both give the same bits. */
  RPT_FLAG_VIEWS_PERSISTENT = 16u, /* RptViewQuery::flags of rptgpu_render_views[_seeded][_device] only: the batch of views
                                    in the persistent path kernel — an OPTIONAL addition within ABI 7, read only by a
                                    library that exports rptgpu_views_persistent_supported (rpt_gpu_views_persistent.h,
                                    included at the end of this file; a library without it ignores the bit) */
  RPT_FLAG_RAYS_PERSISTENT = 32u, /* RptRayQuery::flags of rptgpu_trace_rays[_device] and RptProbeQuery::flags of
                                     rptgpu_bake_probes[_device] only: the call's paths in the persistent path kernel — an
                                     OPTIONAL addition within ABI 7, read only by a library that exports
                                     rptgpu_rays_persistent_supported (rpt_gpu_rays_persistent.h, included at the end of this
                                     file; a library without it ignores the bit) */
  RPT_FLAG_VERTICES_PERSISTENT = 64u /* RptVertexQuery::flags of rptgpu_trace_vertices[_device] only: the call's paths in the
                                    persistent path kernel, which then writes each vertex where it makes it — an OPTIONAL
                                    addition within ABI 7, read only by a library that exports
                                    rptgpu_vertices_persistent_supported (rpt_gpu_vertices_persistent.h, included at the end
                                    of this file; a library without it ignores the bit) */
};

/* ---- what Renderer carries into sample(): src/renderer.rs:18-42 + the call argument ----
 * seed / sample_index_base are ADDITIONS: the reference seeds every row from OS entropy
 * (renderer.rs:121) and is not reproducible.  Random numbers are Philox4x32-10 keyed by
 * `seed`, counter (pixel index, sample index, draw block): the image does not depend on how
 * pixels are partitioned over devices. */
typedef struct RptRenderParams {
  uint32_t width;       /* renderer.rs:26 */
  uint32_t height;      /* renderer.rs:29 */
  uint32_t max_bounces; /* renderer.rs:38 */
  uint32_t iterations;  /* argument of sample(): paths per pixel in this batch (renderer.rs:117) */
  double exposure_value; /* renderer.rs:32 */
  uint64_t seed;
  uint64_t sample_index_base; /* global index of this batch's first sample                    */
  /* pixel partition for multi-GPU: the image is cut into tile_width x tile_height tiles,
     numbered row-major; this call renders tiles with (tile_id % part_count) == part_index and
     writes 0.0 to every other pixel, so the sum over parts is the full frame.
     part_count = 0 or 1 renders everything. */
  uint32_t tile_width;
  uint32_t tile_height;
  uint32_t part_index;
  uint32_t part_count;
  uint32_t precision_mode; /* RPT_PRECISION_* */
  uint32_t flags;          /* RPT_FLAG_*      */
  /* ABI v6 — how rptgpu_render_batch_reduce brings the ranks' pixels to the root (ignored by every other call):
     RPT_COLLECTIVE_GATHER (also 0): each rank sends only the pixels it owns (ncclSend / ncclRecv), RPT_COLLECTIVE_REDUCE:
     ncclReduce(sum) of full frames that are zero outside the rank's tiles.  Same frame either way.  Every rank of a
     batch must pass the same value.  Until v5: the environment variable RPTGPU_COLLECTIVE, which still overrides. */
  uint32_t collective;
  uint32_t _reserved0;     /* 0 */
} RptRenderParams;
enum { RPT_COLLECTIVE_DEFAULT = 0, RPT_COLLECTIVE_GATHER = 1, RPT_COLLECTIVE_REDUCE = 2 };

/* Per-kernel accounting since the last rptgpu_reset_stats (filled when
 * RPT_FLAG_PROFILE_KERNELS is set; counts are always maintained). */
enum {
  RPT_K_RAYGEN = 0,
  RPT_K_EXTEND = 1, /* closest-hit traversal + intersection      */
  RPT_K_SHADE = 2,  /* emission, NEE generation, BSDF sampling   */
  RPT_K_SHADOW = 3, /* shadow-ray traversal                      */
  RPT_K_RESOLVE = 4,/* nested firefly-clamp fold + accumulation  */
  RPT_K_PATHS = 5,  /* persistent path kernel: all of the above in registers */
  RPT_K_TREE_TRACE = 6, /* per-tree persistent kd traversal (closest-hit and shadow queries of deep trees);
                           its time is also part of RPT_K_EXTEND / RPT_K_SHADOW, which bracket whole queries */
  RPT_K_TREE_SORT = 7,  /* root slab test + queue append (rpt_tree_enter) and the ray sort in front of a traversal;
                           likewise contained in RPT_K_EXTEND / RPT_K_SHADOW */
  RPT_K_COUNT = 8
};

typedef struct RptStats {
  double kernel_ms[RPT_K_COUNT];        /* summed HIP-event time per kernel kind             */
  uint64_t kernel_launches[RPT_K_COUNT];
  uint64_t extend_rays;  /* closest-hit rays traced  (get_closest_hit, renderer.rs:146)      */
  uint64_t shadow_rays;  /* shadow rays the REFERENCE casts for these samples: one per hit and non-ambient
                            light (renderer.rs:191-196)                                       */
  uint64_t shadow_rays_traced; /* of those, the ones actually traversed: a light that can only add exactly zero
                            (bsdf = 0 below an opaque surface, a light sample facing away) needs no ray  */
  uint64_t samples;      /* camera paths started                                             */
  double total_ms;       /* wall time inside rptgpu_render_batch* (host clock)                */
  /* rptgpu_render_batch_reduce since the last reset (ABI v5), HIP events on the library's stream: */
  uint64_t reduce_calls;
  double reduce_render_ms;     /* this rank's own tiles                                         */
  double reduce_collective_ms; /* the gather (or reduce) over the ranks: includes waiting for the slowest one */
  double reduce_copy_ms;       /* root: assembling the frame and its copy to host memory        */
} RptStats;

typedef struct rptgpu_scene rptgpu_scene; /* opaque */

/* ---- library ---- */
int rptgpu_abi_version(void);
const char* rptgpu_strerror(int code);
/* Detail of the last error on this handle (or of the last failed create when h == NULL);
 * the pointer stays valid until the next call on the same handle / thread. */
const char* rptgpu_last_error_detail(const rptgpu_scene* h);
int rptgpu_device_count(int* out_count);

/* ---- scene hand-off: replaces `&Scene` (scene.rs:7-16) behind Renderer::new
 * (renderer.rs:46).  Builds the kd-trees by the reference rule (kdtree.rs:235-345), flattens
 * everything into the device layout and uploads it to `device`.  Unsupported shapes are
 * rejected here, not at render time. */
int rptgpu_scene_create(const RptScene* scene, int device, rptgpu_scene** out);
void rptgpu_scene_destroy(rptgpu_scene* h);

/* ---- the knobs of a scene handle as a struct (ABI v6; SURVEY 5: "kernel tunables via a params struct, not env vars").
 * None of them changes a result — they route work between kernels that compute the same bits (tests: every route
 * against the same fixtures) and bound memory.  rptgpu_scene_options_default() fills in the defaults;
 * rptgpu_scene_create(scene, device, out) is rptgpu_scene_create_opts with them.  The environment variables named
 * beside the fields — the only interface until v5 — remain as OVERRIDES for experiments: read once, inside
 * rptgpu_scene_create[_opts], never afterwards (a handle's behaviour is fixed when it is made).  What is left in the
 * environment only: diagnostics (RPTGPU_PRINT_CREATE / _LAUNCH / _PHASES), the A/B switches RPTGPU_FLAT_TRIS_GLOBAL,
 * RPTGPU_NO_PLANE_TABLE, RPTGPU_PATH_REORDER (the per-depth re-order of the paths in scenes whose trees are walked
 * in-kernel) and RPTGPU_WS_FREE_FRACTION (percent of the free memory a pass may take: 85), the tests' hooks
 * RPTGPU_FAIL_COMM, RPTGPU_PATH_REORDER_MIN and RPTGPU_REC_RATIO, and the launcher's RPTGPU_LOCAL_RANKS /
 * LOCAL_WORLD_SIZE (how many ranks share the host's cores). */
typedef struct RptSceneOptions {
  uint32_t struct_size;           /* sizeof(RptSceneOptions) of the caller's header: lets the struct grow            */
  uint32_t _reserved0;            /* 0                                                                               */
  /* routing */
  uint32_t deep_depth;            /* RPTGPU_DEEP_DEPTH (8): a kd-tree at least this deep gets its own ray queue, sort
                                     and persistent traversal kernel; shallower ones are walked inside the path kernels */
  uint32_t fast_max_depth;        /* RPTGPU_FAST_MAX_DEPTH (32): deeper trees never use the in-kernel traversals        */
  int32_t sort_rays;              /* RPTGPU_SORT_RAYS (-1): 0 never, 1 every deep tree, -1 by the tree's footprint      */
  int32_t rays_in_kernel;         /* RPTGPU_RAYS_IN_KERNEL (0): rptgpu_closest_hit keeps to one kernel for any scene    */
  uint64_t sort_min_bytes;        /* RPTGPU_SORT_MIN_BYTES (8 MiB): nodes + leaf records of a tree whose rays are sorted */
  uint64_t sort_shadow_min_bytes; /* RPTGPU_SORT_SHADOW_MIN_BYTES (8 MiB): ... whose SHADOW rays are sorted too          */
  uint32_t sort_min_rays;         /* RPTGPU_SORT_MIN_RAYS (2^19): queries of fewer rays are not sorted                   */
  int32_t nest_trace;             /* RPTGPU_NEST_TRACE (1): kd-trees of kd-trees in rpt_nest_trace (else rpt_tree_generic) */
  int32_t leaf_boxes;             /* RPTGPU_LEAF_BOXES (1): the conservative f32 box in front of every exact leaf test    */
  int32_t object_filter_min;      /* RPTGPU_OBJECT_FILTER_MIN (5): flat scenes of at least this many objects filter them; 0 = never */
  uint64_t device_build_min;      /* RPTGPU_DEVICE_BUILD_MIN (32768; 4096 when ranks share the host): kd-trees of at least
                                     this many primitives are built on the device; 0 = never                              */
  uint32_t build_threads;         /* RPTGPU_BUILD_THREADS (0 = the usable cores): host threads of the flattening / kd build */
  uint32_t paths_chunk;           /* RPTGPU_PATHS_CHUNK (0 = per launch: 16, 2 for filtered flat scenes at 4+ bounces, fewer
                                     when a lane would get under 24 items): samples per work item of the persistent path kernel       */
  /* memory */
  uint64_t workspace_bytes;       /* RPTGPU_WS_BYTES (240 GiB; and never more than 85 % of the free memory): cap of the
                                     wavefront pipeline's path state                                                          */
  uint64_t lbuf_bytes;            /* RPTGPU_LBUF_BYTES (32 GiB): cap of the per-sample radiance buffer of rpt_paths        */
  uint64_t target_paths;          /* RPTGPU_TARGET_PATHS (0 = what the workspace cap holds, at most 512 Mi): paths per pass */
  /* multi-GPU */
  double comm_timeout_s;          /* RPTGPU_COMM_TIMEOUT_S (300): a batch's exchange is given up after this long           */
  /* routing, added after the first v6 header (struct_size 104): a caller built against that one gets the default */
  int32_t env_park;               /* RPTGPU_ENV_PARK (1): rpt_paths parks the texture lookups of escaped rays per lane and runs
                                     them for the wave together; 0 = each on the spot                                       */
  uint32_t paths_batch;           /* RPTGPU_PATHS_BATCH (0 = per launch: 1/32 of a wave's share of the launch's work items, within
                                     [16, 256]; at most 1024): work items a wave of rpt_paths claims with one atomic on the
                                     work counter                                                                            */
} RptSceneOptions;
/* Fills *out (sizeof(RptSceneOptions) of THIS header, 112 bytes) with the defaults. */
void rptgpu_scene_options_default(RptSceneOptions* out);
/* ABI v7 — the same for a caller whose header may be older: writes exactly struct_size bytes.  struct_size must be a size
 * the struct has had (104: the first v6 header, before env_park; 112); RPTGPU_E_INVALID_ARGUMENT otherwise. */
int rptgpu_scene_options_default_sized(RptSceneOptions* out, uint32_t struct_size);
/* opts == NULL: the defaults.  opts->struct_size must be one of those sizes (the fields a smaller struct lacks take their
 * defaults); RPTGPU_E_INVALID_ARGUMENT otherwise, also when a field — or an RPTGPU_* override of one — is out of range. */
int rptgpu_scene_create_opts(const RptScene* scene, int device, const RptSceneOptions* opts, rptgpu_scene** out);
/* The options a handle runs with, environment overrides applied.  ABI v7: the caller sets out->struct_size to the size of
 * ITS struct before the call (rptgpu_scene_options_default[_sized] leaves it set); exactly that many bytes are written. */
int rptgpu_scene_get_options(const rptgpu_scene* h, RptSceneOptions* out);

/* ---- live updates of a handle's scene: the objects' and lights' placements and materials, for animation (a frame loop
 * keeps one handle instead of creating one per frame).  Additions within ABI version 7, detected by symbol (dlsym
 * "rptgpu_scene_set_objects").  After an update every result — frames, rptgpu_closest_hit, rptgpu_buffer_* — is
 * bit-identical to what a handle freshly created from the updated scene gives.  The kd-trees, triangles, environment
 * texels, routing and workspace (with what it has learned) stay; device buffers (rptgpu_buffer) and the communicator
 * of the handle stay valid.  The object, light and environment counts and all geometry are fixed at creation: for new
 * geometry create a new handle.
 * Both calls are all or nothing: every entry is checked before anything changes, and a refused call leaves the handle
 * rendering what it rendered before.  RPTGPU_E_INVALID_ARGUMENT, with a detail naming the entry and the reason: an
 * index out of range, an index named twice in one call, a shape or light kind or a `transformed` flag that differs
 * from the one at creation (an untransformed mesh lives in the flat kernel's plane table), a material whose specular
 * lobe probability lies outside [0, 1] (as rptgpu_scene_create refuses it), a NULL array with n > 0, an abandoned
 * handle.  A call returns after its uploads on the handle's stream have completed.  Do not call them concurrently
 * with a render, a buffer sample or another call on the same handle.  n == 0 is a no-op. */
/* Replace top-level object index[i] with objects[i] (its shape's Transformed fields and its material).
 * The shape's geometry (triangles, children, plane, monomial parameters) is NOT read: it stays what the handle
 * was created with.  objects[i].shape.kind and .transformed must equal the object's at creation. */
int rptgpu_scene_set_objects(rptgpu_scene* h, uint64_t n, const uint32_t* index, const RptObject* objects);
/* Same for scene.lights: colour / vector of Point, Directional, Ambient; xf + material of Light::Object.
 * kind must be unchanged; a Light::Object's shape geometry is not read. */
int rptgpu_scene_set_lights(rptgpu_scene* h, uint64_t n, const uint32_t* index, const RptLight* lights);

/* ---- a deforming mesh on a live handle (cloth, a character, a surface driven by the particle systems): new triangles
 * for one mesh, the count unchanged.  Additions within ABI version 7, detected by symbol (dlsym "rptgpu_scene_set_mesh").
 * `object` is a top-level object whose shape is a Mesh; n must equal its triangle count at creation (deformation, not
 * re-topology).  The triangles' records are made on the device, the mesh's kd-tree is rebuilt by the builder creation
 * would use, and everything creation derives from the tree follows, so that afterwards every result — frames under
 * every flag, rptgpu_closest_hit, rptgpu_render_aov, rptgpu_trace_rays, rptgpu_bake_probes, rptgpu_buffer_* — is
 * bit-identical to that of a handle freshly created from the scene in which that mesh has the new triangles.  Objects
 * that share the mesh (one tree) all follow.  Workspace, learned ratios, device buffers and the communicator stay valid.
 * All or nothing: the new scene is built in a second set of arrays that replaces the first only at the end; a refused or
 * failed call leaves the handle rendering what it rendered before.  RPTGPU_E_INVALID_ARGUMENT, the detail naming the
 * reason: a null or abandoned handle, an index out of range, an object that is not a mesh, n different from the count at
 * creation, a NULL array with n > 0 — and, "needs a new handle": a mesh that is also a Light::Object's shape or a group's
 * child, a handle whose trees are all single leaves (the flat path kernel's LDS layout and plane table are derived from
 * the coordinates at creation), and a
 * deformation that makes the tree of an object walked inside the path kernels deeper than their stacks (fast_max_depth).
 * The call returns when the handle is ready to render.  Not concurrent with another call on the same handle. */
int rptgpu_scene_set_mesh(rptgpu_scene* h, uint32_t object, uint64_t n, const RptTriangle* tris);
/* The same with the triangles on the handle's device ([n][18] f64: v1 v2 v3 n1 n2 n3, as RptTriangle); no triangle goes
 * through the host.  stream: the producer's, waited for before d_tris is read (as rptgpu_trace_rays_device; NULL: none).
 * d_tris is only read. */
int rptgpu_scene_set_mesh_device(rptgpu_scene* h, uint32_t object, uint64_t n, const void* d_tris, void* stream);

/* ---- a group whose children move on a live handle (instanced bodies: the spheres of a particle system, a swarm): new
 * placements for the children of one KdTree<Box<dyn Bounded>>.  Additions within ABI version 7, detected by symbol (dlsym
 * "rptgpu_scene_set_group").  `object` is a top-level object whose shape is a GROUP; n must equal its child count at
 * creation.  Child i keeps its kind and its `transformed` flag; only the five RptTransform fields change, and they are
 * taken as given, exactly as creation takes them.  The record of a child that is not transformed is ignored; of each
 * child the call reads kind, transformed and xf and nothing else.  The children's records and boxes are made on the device, the group's
 * kd-tree is rebuilt by the builder creation would use, and everything creation derives from the tree follows, so that
 * afterwards every result — frames under every flag, rptgpu_closest_hit, rptgpu_render_aov, rptgpu_trace_rays,
 * rptgpu_bake_probes, rptgpu_buffer_* — is bit-identical to that of a handle freshly created from the scene in which the
 * group has the new children.  Workspace, learned ratios, device buffers and the communicator stay valid.
 * All or nothing, as rptgpu_scene_set_mesh: a refused or failed call leaves the handle rendering what it rendered
 * before.  RPTGPU_E_INVALID_ARGUMENT, the detail naming the reason: a null or abandoned handle, an index out of range,
 * an object that is not a group, n different from the count at creation, a NULL array with n > 0, a child whose kind or
 * `transformed` flag differs from the creation's — and, "needs a new handle": a group with a MESH, MONOMIAL or GROUP
 * child (accepted: children that are all SPHERE or CUBE), a handle whose trees are all single leaves (the flat path
 * kernel), a rebuilt tree deeper than fast_max_depth for a group that is walked inside the path kernels, 32-bit node or
 * entry index overflow.  n == 0 returns RPTGPU_OK.  The call returns when the handle is ready to render.  Not concurrent
 * with another call on the same handle. */
int rptgpu_scene_set_group(rptgpu_scene* h, uint32_t object, uint64_t n, const RptShape* children);
/* The same with the placements on the handle's device: [n] RptTransform, 51 f64 each (transform[16], linear[9],
 * inverse_transform[16], normal_transform[9], scale); the kinds and `transformed` flags are the creation's.  stream: the
 * producer's, waited for before d_transforms is read (as rptgpu_scene_set_mesh_device; NULL: none).  d_transforms is only
 * read. */
int rptgpu_scene_set_group_device(rptgpu_scene* h, uint32_t object, uint64_t n,
                                  const void* d_transforms /* [n] RptTransform, 51 f64 each */, void* stream);

/* ---- the hot path: replaces the body of Renderer::sample (renderer.rs:117-129).
 * Writes out_rgb[(y*width+x)*3+c] = mean over `iterations` paths of pixel (x,y), times
 * 2^exposure_value (renderer.rs:141); y = 0 is the top row (renderer.rs:134).  The host then
 * calls Buffer::add_samples(&colors) unchanged (buffer.rs:32-40). */
int rptgpu_render_batch(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* params,
                        double* out_rgb /* width*height*3, host */);

/* Same, but the result stays in device memory (for an RCCL reduce of the framebuffer by the
 * caller).  `d_out` is a device pointer to width*height*3 elements, f64 if out_is_f32 == 0
 * else f32.  `stream` is a hipStream_t (NULL = the library's own stream); the call returns
 * after the work has been enqueued AND completed on that stream (synchronous). */
int rptgpu_render_batch_device(rptgpu_scene* h, const RptCamera* camera,
                               const RptRenderParams* params, void* d_out, int out_is_f32,
                               void* stream);

/* ---- multi-GPU: one process per GPU, pixel tiles shard across the ranks, ONE collective per batch.
 * The reference's rows are independent (renderer.rs:118-127); rank r renders the 32x8 tiles with
 * tile_id % world == r and the full frame is the SUM of the ranks' frames (every pixel is non-zero on
 * exactly one rank; random numbers are keyed by pixel and sample, so the frame does not depend on the
 * partition).  The library owns the communicator: one RCCL communicator per handle on the handle's
 * device and stream (librccl is opened on first use; without it these calls return RPTGPU_E_COMM).
 *   rank 0:      rptgpu_comm_unique_id(id);  hand the 128 bytes to every rank (any side channel)
 *   every rank:  rptgpu_comm_init(h, rank, world, id);
 *   per batch:   rptgpu_render_batch_reduce(h, camera, params, root, out_rgb32_on_root)
 * rptgpu_render_batch_reduce replaces the body of Renderer::sample on every rank: it renders this
 * rank's tiles (params->tile_*, part_* are overridden: 32x8 tiles, part = rank of world), brings the f32
 * means to `root` over xGMI on the library's stream, and on `root` writes the width*height*3 f32 means to
 * host memory (out_rgb32 may be NULL on other ranks).  Synchronous.  The exchange is a GATHER: every rank
 * sends only the pixels it owns (width*height*3*4 / world bytes, ncclSend / ncclRecv in one group), the
 * root puts them in place — the tiles are disjoint, so nothing is added and the frame is the one a single
 * GPU renders, bit for bit.  RPTGPU_COLLECTIVE=reduce selects ncclReduce(sum) of zero-filled full frames
 * instead (8x the bytes at 8 ranks; the same frame, since every pixel is non-zero on one rank only).
 * With no communicator attached (world = 1) it is a plain single-GPU render into out_rgb32.
 * Failure: the call waits for the stream by polling it together with ncclCommGetAsyncError, at most
 * RPTGPU_COMM_TIMEOUT_S seconds (default 300) per batch.  A rank that fails locally (HIP error, out of
 * memory), sees an asynchronous RCCL error or times out aborts its communicator (ncclCommAbort) and
 * returns RPTGPU_E_COMM / its own error; its peers then run into their time-out or an RCCL error and do
 * the same.  After that every further rptgpu_render_batch_reduce on the handle returns RPTGPU_E_COMM until
 * rptgpu_comm_destroy + rptgpu_comm_init.  The library's stream is drained before the error is returned (nothing is
 * written into out_rgb32 afterwards); should the device not finish within the time-out again, the handle is ABANDONED
 * (ABI v7): its workspace may still be in use by that work, so every later call that would enqueue work on it returns
 * RPTGPU_E_COMM — destroy it.  Argument errors that every rank makes alike (bad params) are
 * returned before anything is enqueued and leave the communicator alone. */
#define RPTGPU_UNIQUE_ID_BYTES 128
int rptgpu_comm_unique_id(uint8_t out_id[RPTGPU_UNIQUE_ID_BYTES]);
int rptgpu_comm_init(rptgpu_scene* h, int rank, int world, const uint8_t id[RPTGPU_UNIQUE_ID_BYTES]);
int rptgpu_comm_destroy(rptgpu_scene* h);
int rptgpu_render_batch_reduce(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* params,
                               int root, float* out_rgb32 /* width*height*3 f32, host, on root */);
/* Diagnostics: the frame as `world` ranks would produce it, on this one GPU and without a communicator — every
 * rank's part rendered in turn into the root's receive buffer (packed, as ncclSend would deliver it) and placed by
 * the root's pixel lists: the gather of rptgpu_render_batch_reduce minus the wire.  Must equal the frame of a plain
 * render bit for bit (tests; a box with one GPU cannot run RCCL across two ranks). */
int rptgpu_render_batch_emulate_ranks(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* params,
                                      int world, float* out_rgb32 /* width*height*3 f32, host */);

/* ---- the closest-hit kernel on its own: replaces Renderer::get_closest_hit
 * (renderer.rs:211-220) for a batch of rays (host arrays, n rays, xyz interleaved).
 * out_t = +inf and out_object = -1 on a miss.  A scene with deep trees sends the rays the way a
 * render does (object by object, per-tree queues, sort, persistent traversal); otherwise, or with
 * RPTGPU_RAYS_IN_KERNEL=1, one kernel walks every object per ray.  Same results either way. */
int rptgpu_closest_hit(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs,
                       uint32_t precision_mode, double* out_t, double* out_normal,
                       int32_t* out_object);

/* ---- path-traced radiance along rays the CALLER supplies: light probes, lightmap texels, other projections, rays made
 * by another program.  Additions within ABI version 7, detected by symbol (dlsym "rptgpu_trace_rays").
 * Ray i is origins[3i..], dirs[3i..] (f64, xyz interleaved); the direction is used as given, as rptgpu_closest_hit uses
 * it (normalise it yourself: the estimator, like the reference's trace_ray, expects a unit vector).  out_rgb[3i..] =
 * (sum over s = 0 .. iterations-1, in that order, of L(i, s)) / iterations * 2^exposure_value, where L(i, s) is
 * Renderer::trace_ray (renderer.rs:143-175: next-event estimation over every light, the sampled BSDF, the nested
 * firefly clamp) of ray i with max_bounces bounces — every sample of a ray starts from the same ray.
 * THE STREAM CONTRACT.  The random numbers of L(i, s) are the Philox4x32-10 stream keyed by `seed` with the counter
 * (stream id, sample_index_base + s, draw block) — the keying of pixels, with the stream id where the pixel index is —
 * read from draw `first_draw` on.  The stream id of ray i is streams[i], or i (its index in this call's arrays) when
 * streams is NULL.  So a ray's result depends on (its origin and direction, seed, its stream id, its sample indices,
 * first_draw) and on nothing else: not on which other rays share the call, on their order, on how the library cuts the
 * call into pieces and passes, or on how a caller splits a batch over calls, handles or GPUs.  With the rays a camera
 * makes (pixel p's ray of sample s, streams[i] = p, first_draw = the draws the camera took: 2, more under a lens) the
 * result is the frame of rptgpu_render_batch, bit for bit.
 * The call runs the wavefront pipeline (flat scenes are walked in-kernel, deep trees through the per-tree queries), sized
 * and restarted like a render's passes; RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured,
 * RPT_FLAG_WAVEFRONT changes nothing, and RptStats advances as for a render (samples = n * iterations).  The one exception:
 * a library with rpt_gpu_rays_persistent.h (included at the end of this file) runs the persistent kernel instead when it is
 * asked to with RPT_FLAG_RAYS_PERSISTENT.
 * RPTGPU_RAYS_PIECE (environment, read per call; tests): the rays per piece.
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work and with a detail naming the reason: a NULL RptRayQuery, a
 * wrong struct_size, iterations == 0, max_bounces > 254, a precision_mode other than RPT_PRECISION_F64_STRICT,
 * RPT_FLAG_PERSISTENT (the persistent kernel makes its rays from a camera), NULL origins / dirs / out with n > 0, more
 * than 2^32 rays without stream ids, a NULL handle; RPTGPU_E_COMM for an abandoned handle.  n == 0 returns RPTGPU_OK. */
typedef struct RptRayQuery {
  uint32_t struct_size;       /* sizeof(RptRayQuery) */
  uint32_t max_bounces;       /* <= 254 */
  uint32_t iterations;        /* samples per ray, > 0 */
  uint32_t first_draw;        /* draw index at which every ray's stream continues (0: a fresh stream) */
  double exposure_value;
  uint64_t seed;
  uint64_t sample_index_base; /* index of every ray's first sample */
  uint32_t precision_mode;    /* RPT_PRECISION_* */
  uint32_t flags;             /* RPT_FLAG_* */
} RptRayQuery;
int rptgpu_trace_rays(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs,
                      const uint32_t* streams /* may be NULL */, const RptRayQuery* q, double* out_rgb /* [n][3], host */);
/* The same with every array in device memory ([n][3] f64 rays and results, [n] u32 stream ids or NULL), read and written
 * where it lies.  `stream` is the hipStream_t the arrays' producer ran on: the call synchronises it, runs on the handle's
 * own stream and returns when the results are complete (rptgpu_render_batch_device's rule).  NULL means NO stream, not
 * the null stream: nothing is waited for.  The handle's stream is non-blocking (it is not ordered with the null stream),
 * so a caller whose producer ran on the null stream — the default stream of most frameworks — synchronises it itself
 * before the call (hipStreamSynchronize(0)); GpuScene.trace_rays does. */
int rptgpu_trace_rays_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs,
                             const void* d_streams /* may be NULL */, const RptRayQuery* q, void* d_out_rgb, void* stream);

/* ---- light probes baked on the device: per probe, `samples` directions made from the Philox stream, one path along each
 * (Renderer::trace_ray, as rptgpu_trace_rays runs it), projected as the directions come back.  Additions within ABI
 * version 7, detected by symbol (dlsym "rptgpu_bake_probes").  Probe i stands at positions[3i..]; out is [n][9][3] f64 for
 * RPT_PROBE_SH9 (radiance in the real spherical harmonics of bands 0-2) and [n][3] for RPT_PROBE_IRRADIANCE (the
 * irradiance of a surface with normal normals[3i..]).  24 B (48 B) in and 216 B (24 B) out per probe, whatever S is.
 * THE STREAM CONTRACT.  Direction k of probe i is sample sample_index_base + k of the Philox4x32-10 stream keyed by `seed`
 * (rptgpu_trace_rays' keying); its stream id is streams[i], or i (the probe's index in this call's arrays) when streams is
 * NULL.  The direction is made from draw 0 on, and the path that leaves along it continues the SAME stream at the draw
 * where the direction stopped — what a render's first kernel does behind the camera's draws.  So a probe's result depends
 * on (its position, its normal, seed, its stream id, the sample indices, max_bounces) and on nothing else: not on the other
 * probes of the call, on their order, on the pieces and passes the library cuts the call into, or on how a caller splits
 * the PROBES over calls, handles or GPUs.
 * DIRECTIONS, in plain f64, no contraction, the expressions in the order written:
 *   RPT_PROBE_SH9         uniform on the sphere without transcendentals: (x1, x2) = UnitDisc (rand_distr 0.4: pairs of
 *                         gen_range(-1, 1) until x1*x1 + x2*x2 <= 1);  s = x1*x1 + x2*x2;  r = 2.0*sqrt(1.0 - s);
 *                         d = (x1*r, x2*r, 1.0 - 2.0*s)
 *   RPT_PROBE_IRRADIANCE  d = Sphere::sample(normal).v (sphere.rs:52-64): cosine-weighted about normalize(normal).  A zero
 *                         or non-finite normal yields whatever that function yields; it is not refused
 * The ray is (position, d), used as given.
 * RESULT.  L_k = Renderer::trace_ray of ray k: what rptgpu_trace_rays returns for it with iterations = 1, exposure_value =
 * 0 and first_draw = the draws its direction took.  With S = samples and k ascending from sums that start at +0.0:
 *   RPT_PROBE_SH9         acc[j][c] = acc[j][c] + L_k[c] * Y_j(d_k);  out[j][c] = acc[j][c] * (12.566370614359172 / (double)S)
 *   RPT_PROBE_IRRADIANCE  acc[c] = acc[c] + L_k[c];                   out[c] = acc[c] * (3.141592653589793 / (double)S)
 * The basis, in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), at d = (x, y, z):
 *   Y0 = 0.28209479177387814                  Y1 = 0.4886025119029199*y            Y2 = 0.4886025119029199*z
 *   Y3 = 0.4886025119029199*x                 Y4 = 1.0925484305920792*(x*y)        Y5 = 1.0925484305920792*(y*z)
 *   Y6 = 0.31539156525252005*(3.0*(z*z) - 1.0)  Y7 = 1.0925484305920792*(x*z)      Y8 = 0.5462742152960396*(x*x - y*y)
 * The call runs the wavefront pipeline as rptgpu_trace_rays does, in pieces of whole probes; RPT_FLAG_GENERAL_TRAVERSAL and
 * RPT_FLAG_PROFILE_KERNELS are honoured, and RptStats advances as for a render (samples = n * S).  RPTGPU_PROBES_PIECE
 * (environment, read per call; tests): the probes per piece.
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work and with a detail naming the reason: a NULL RptProbeQuery, a
 * wrong struct_size, an unknown kind, samples == 0, max_bounces > 254, a precision_mode other than
 * RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT, NULL positions or out with n > 0, NULL normals with
 * RPT_PROBE_IRRADIANCE, more than 2^32 probes without stream ids, a NULL handle; RPTGPU_E_COMM for an abandoned handle.
 * n == 0 returns RPTGPU_OK. */
enum { RPT_PROBE_SH9 = 0, RPT_PROBE_IRRADIANCE = 1 };
typedef struct RptProbeQuery {
  uint32_t struct_size;       /* sizeof(RptProbeQuery) */
  uint32_t kind;              /* RPT_PROBE_* */
  uint32_t samples;           /* S: directions per probe, one path each, > 0 */
  uint32_t max_bounces;       /* <= 254 */
  uint64_t seed;
  uint64_t sample_index_base; /* sample index of every probe's first direction */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* as RptRayQuery: GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused */
} RptProbeQuery;
int rptgpu_bake_probes(rptgpu_scene* h, uint64_t n, const double* positions /* [n][3] */,
                       const double* normals /* [n][3]; RPT_PROBE_IRRADIANCE only, else NULL */,
                       const uint32_t* streams /* [n] or NULL */, const RptProbeQuery* q, double* out /* host */);
/* The same with every array in device memory; `stream` and the synchronisation rule are rptgpu_trace_rays_device's. */
int rptgpu_bake_probes_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals,
                              const void* d_streams /* may be NULL */, const RptProbeQuery* q, void* d_out, void* stream);

/* ---- visibility on its own: "is anything between A and B?" for rays the caller supplies, and ambient occlusion baked from
 * directions the library draws itself.  Additions within ABI version 7, detected by symbol (dlsym "rptgpu_occluded").  Both
 * run the query a render's shadow rays run — it stops at the first blocker and makes no normal — and both are DEFINED by
 * rptgpu_closest_hit, so that a caller may replace "closest hit, then compare t" by them and keep every bit.
 * OCCLUDED.  Ray i is origins[3i..], dirs[3i..] (f64, xyz interleaved), used as given: no normalisation, t_min = 1e-12, no
 * origin offset — rptgpu_closest_hit's rules.  max_t[i] is in units of the ray parameter (a distance only for a unit
 * direction); max_t == NULL means +inf for every ray.  With t_i = what rptgpu_closest_hit returns for ray i (+inf on a
 * miss; a NaN record — MonomialSurface reports one for a vertical ray over a corner of its box — stays NaN) and
 *   stop_i = fmin(max_t[i], 1.7976931348623157e308)
 *   out[i] = (t_i > stop_i) ? 0 : 1                       (sample_lights' test, renderer.rs:191-197, negated)
 * So a NaN max_t behaves as +inf, a negative max_t (and 0.0) is never occluded, a NaN hit is occluded, a hit exactly at
 * max_t is occluded; none of these is refused.  A ray's result depends on that ray, its max_t and the scene and on nothing
 * else: not on the other rays of the call, on their order, or on the pieces the library cuts the call into.
 * 56 B in (48 B without max_t) and 1 B out per ray.
 * AMBIENT OCCLUSION.  Point i stands at positions[3i..] with normal normals[3i..]; S = samples.  Direction k of point i is
 * d_k = Sphere::sample(normals[i]).v (sphere.rs:52-64: cosine-weighted about normalize(normal) — exactly
 * RPT_PROBE_IRRADIANCE's direction, in its expressions), made from draw 0 of the Philox4x32-10 stream keyed by `seed` with
 * the counter (stream id, sample_index_base + k, draw block); the stream id is streams[i], or i (the point's index in this
 * call's arrays) when streams is NULL.  A zero or non-finite normal yields whatever that function yields; it is not refused.
 * The ray is (positions[i], d_k), used as given: NO origin offset.  A point that lies ON a surface sees that surface only
 * through the 1e-12 guard on t; a caller whom that does not suit lifts the points off their surface before the call.
 *   v_k = (t_k > fmin(max_distance, 1.7976931348623157e308)) ? 1 : 0     (t_k as above; NaN max_distance = +inf)
 *   out_ao[i]      = (double)(v_0 + .. + v_{S-1}) / (double)S            (an integer count: no order dependence)
 *   out_bent[i][c] = acc[c] / (double)S,  acc[c] = acc[c] + d_k[c] over the visible k, ascending, from +0.0
 * out_ao is the unoccluded fraction (1.0: open sky); out_bent (may be NULL) is the unnormalised bent normal.  A point's
 * result depends on (its position, its normal, seed, its stream id, the sample indices, max_distance) and on nothing else:
 * not on the other points, their order, the pieces and passes, or on how a caller splits the POINTS over calls or GPUs.
 * 48 B in (52 B with stream ids) and 8 B or 32 B out per point, whatever S is.
 * ROUTE.  The rays are laid where a depth's shadow rays lie and go through the visibility query of a render: one kernel
 * that walks the whole scene per ray, or — scenes with deep trees — the per-tree queries (queues, ray sort, persistent
 * traversal, the generic walker for trees of trees); RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured.
 * RptStats: shadow_rays and shadow_rays_traced advance by the rays traced (n, or n * S), kernel_launches[RPT_K_SHADOW] by the
 * queries; samples does not advance.  There is no CPU fallback: RPTGPU_E_NO_DEVICE.  RPTGPU_OCCLUSION_PIECE (environment,
 * read per call; tests): the rays (rptgpu_occluded) or the points (rptgpu_bake_ao) per piece.
 * NOT IN SCOPE: multi-GPU sharding (a caller shards the rays or the points: a result depends on nothing else; the device
 * form of rptgpu_closest_hit is rptgpu_first_hits_device, below); ambient occlusion as a feature buffer of a render or in the device Buffer; distance-weighted
 * ambient occlusion.
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and with the output arrays
 * untouched: a NULL query, a wrong struct_size, samples == 0, reserved != 0, a precision_mode other than
 * RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT (the persistent kernel makes its rays from a camera), NULL origins / dirs /
 * out or positions / normals / out_ao with n > 0, more than 2^32 points without stream ids, a NULL handle; RPTGPU_E_COMM
 * for an abandoned handle.  n == 0 returns RPTGPU_OK. */
typedef struct RptVisibilityQuery {
  uint32_t struct_size;       /* sizeof(RptVisibilityQuery) */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused */
  uint32_t reserved;          /* 0 */
} RptVisibilityQuery;
int rptgpu_occluded(rptgpu_scene* h, uint64_t n, const double* origins /* [n][3] */, const double* dirs /* [n][3] */,
                    const double* max_t /* [n], or NULL: +inf for every ray */, const RptVisibilityQuery* q,
                    uint8_t* out /* [n], host */);
/* The same with every array in device memory; `stream` and the synchronisation rule are rptgpu_trace_rays_device's (NULL
 * means NO stream, not the null stream). */
int rptgpu_occluded_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs,
                           const void* d_max_t /* may be NULL */, const RptVisibilityQuery* q, void* d_out, void* stream);
typedef struct RptAoQuery {
  uint32_t struct_size;       /* sizeof(RptAoQuery) */
  uint32_t samples;           /* S: directions per point, > 0 */
  uint64_t seed;
  uint64_t sample_index_base; /* sample index of every point's first direction */
  double max_distance;        /* in units of the ray parameter = world units (d_k is a unit vector); +inf allowed, NaN = +inf */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* as RptVisibilityQuery */
} RptAoQuery;
int rptgpu_bake_ao(rptgpu_scene* h, uint64_t n, const double* positions /* [n][3] */, const double* normals /* [n][3] */,
                   const uint32_t* streams /* [n] or NULL */, const RptAoQuery* q, double* out_ao /* [n], host */,
                   double* out_bent /* [n][3], host; may be NULL */);
/* The same with every array in device memory; `stream` as for rptgpu_occluded_device. */
int rptgpu_bake_ao_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals,
                          const void* d_streams /* may be NULL */, const RptAoQuery* q, void* d_out_ao,
                          void* d_out_bent /* may be NULL */, void* stream);

/* ---- batches of views: n_views frames of one size in ONE call, each from a camera of its own under one of three
 * projections — cube-map faces, stereo pairs, turntables, light fields, data sets; orthographic views; and 360-degree
 * panoramas in exactly Hdri::get_color's convention (environment.rs:25-52), so that a rendered panorama is a valid
 * RptEnvironment texel array: one scene captured as the environment of another.  Additions within ABI version 7, detected
 * by symbol (dlsym "rptgpu_render_views").  The rays are made on the device from each pixel's own Philox stream (96 + 16 B
 * per VIEW in, 24 B per pixel out, whatever the sample count).  The views of a call share the launches and the host waits
 * of the wavefront pipeline's depth loop, which a small frame on its own cannot fill — whatever their seeds: where the
 * views' seeds differ (seed_stride != 0, or the _seeded entry points of rpt_gpu_views_seeded.h) the seed travels with the path.
 * out[v][y][x][c], row-major, top row first, v in the order of `views`.
 * THE STREAM CONTRACT.  Sample s of pixel p = y*width + x of view v draws from the Philox4x32-10 stream keyed by
 * seed + v*seed_stride (wrapping in 64 bits) with the counter (p, sample_index_base + s, draw block), from draw 0 on; its
 * path continues the SAME stream behind the camera's draws, as a render's does.  out[v][p] = (sum over s = 0 ..
 * iterations-1, ascending, from +0.0, of L(v, p, s)) / iterations * 2^exposure_value, where L is Renderer::trace_ray
 * (renderer.rs:143-175) of the ray below — rptgpu_render_batch's expressions.  A view's pixels depend on that view, the
 * query and the scene and on nothing else: not on the other views of the call, on their order, or on the pieces and passes
 * the library cuts the call into.
 * THE RAY of (v, p, s), in plain f64, no contraction, the expressions in the order written; gen_range(a, b) is the
 * reference's (rand 0.8 UniformFloat: one draw), normalize(a) = a / sqrt((a.x*a.x + a.y*a.y) + a.z*a.z) component by
 * component, `right` = normalize(direction x up) (camera.rs:67), a sum of three terms is added left to right:
 *   RPT_VIEW_PERSPECTIVE   exactly rptgpu_render_batch's ray (renderer.rs:132-139, camera.rs:64-81, the lens included; the
 *                          camera's constants are made by the host function a render uses): view v is rptgpu_render_batch
 *                          of its camera with seed + v*seed_stride, bit for bit.
 *   RPT_VIEW_ORTHOGRAPHIC  px, py and their two gen_range draws as in the perspective case (renderer.rs:132-138; the
 *                          integers 2*x + 1 and 2*(height - y) - 1 are formed in uint32_t as a render forms them, which
 *                          is exact for width, height < 2^31);
 *                          origin = eye + (px*right + py*up) * ortho_scale (the form of camera.rs:74);
 *                          dir = normalize(direction).  px and py span [-1, 1] over the LONGER image side, so ortho_scale
 *                          is the half-extent of that side in world units.  fov, aperture, focal_distance: not read.
 *   RPT_VIEW_PANORAMA      world-aligned at eye: column <-> atan2(z, x) + pi over width-1, row <-> acos(y) over height-1.
 *                          jx = gen_range(-0.5, 0.5); jy = gen_range(-0.5, 0.5);
 *                          cx = (double)x + jx; if (cx < 0.0) cx = cx + (double)(width-1); else if (cx > (double)(width-1))
 *                          cx = cx - (double)(width-1);          (columns 0 and width-1 are the same meridian)
 *                          cy = fmin(fmax((double)y + jy, 0.0), (double)(height-1));
 *                          psi = cx / (double)(width-1) - 0.5;   (the azimuth atan2(z, x) in turns)
 *                          fabs(psi) <= 0.25:  (s, c) = rpt_sincos_pio2(6.283185307179586 * psi)
 *                          otherwise:          (s, c) = -rpt_sincos_pio2(6.283185307179586 * (psi - copysign(0.5, psi)))
 *                          (se, ce) = rpt_sincos_pio2((0.5 - cy / (double)(height-1)) * 3.141592653589793);
 *                          dir = (ce*c, se, ce*s); origin = eye.  Every argument stays within rpt_sincos_pio2's
 *                          |x| < 3 pi / 4 (include/rpt_math.h).  direction, up, fov, aperture, focal_distance: not read.
 * The call runs the wavefront pipeline (always, unless a library with rpt_gpu_views_persistent.h is asked for the persistent
 * kernel with RPT_FLAG_VIEWS_PERSISTENT: that file, included at the end of this one), as rptgpu_trace_rays does, sized and restarted like a render's passes, over
 * pieces of consecutive (view, pixel) indices (a piece begins and ends wherever the piece size says, inside a view or at
 * its border, whatever the views' seeds: with seeds that differ, rpt_raygen_views_seeded and rpt_shade_seeded run in
 * rpt_raygen_views' and rpt_shade's places and read the seed of each index of the piece, 8 B per index more, and the
 * first of them is launched once for every view a pass's piece holds — RptStats counts at least one RPT_K_RAYGEN launch per
 * view rendered under a seed of its own, while the depth loop behind it is the piece's and shared);
 * RPT_FLAG_GENERAL_TRAVERSAL and RPT_FLAG_PROFILE_KERNELS are honoured, RPT_FLAG_WAVEFRONT changes nothing, and RptStats
 * advances as for a render (samples = n_views * width * height * iterations).  RPTGPU_VIEWS_PIECE (environment, read per
 * call; tests): the indices per piece.
 * NOT IN SCOPE: the tile partition and multi-GPU (a caller shards the VIEWS over handles: a view's pixels depend on nothing
 * else), the device-resident Buffer for views, and the persistent path kernel as the default route (the views' feature buffers:
 * rptgpu_render_views_aov, below; a denoised frame per view — batches, features and the filter of rptgpu_buffer_denoise over
 * the whole batch of views —: rpt_gpu_views_denoised.h, which this file includes at its end).
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work and with a detail naming the reason: a NULL RptViewQuery, a
 * wrong struct_size, width, height or iterations == 0, max_bounces > 254, a precision_mode other than
 * RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT, width * height > 2^32, NULL views or out with n_views > 0, frames whose
 * size does not fit 64 bits, an unknown projection, RPT_VIEW_ORTHOGRAPHIC with an ortho_scale that is not finite or <= 0,
 * RPT_VIEW_ORTHOGRAPHIC or RPT_VIEW_PANORAMA with aperture > 0, RPT_VIEW_PANORAMA with width < 2 or height < 2, a NULL
 * handle; RPTGPU_E_COMM for an abandoned handle.  n_views == 0 returns RPTGPU_OK. */
enum { RPT_VIEW_PERSPECTIVE = 0, RPT_VIEW_ORTHOGRAPHIC = 1, RPT_VIEW_PANORAMA = 2 };
typedef struct RptView {
  RptCamera camera;
  uint32_t projection;        /* RPT_VIEW_* */
  uint32_t _pad;              /* reserved: write 0; not read */
  double ortho_scale;         /* RPT_VIEW_ORTHOGRAPHIC: half-extent of the longer image side, world units; else not read */
} RptView;
typedef struct RptViewQuery {
  uint32_t struct_size;       /* sizeof(RptViewQuery) */
  uint32_t width;             /* of every view, > 0 */
  uint32_t height;
  uint32_t max_bounces;       /* <= 254 */
  uint32_t iterations;        /* samples per pixel, > 0 */
  uint32_t _pad;              /* reserved: write 0; not read */
  double exposure_value;
  uint64_t seed;
  uint64_t seed_stride;       /* view v renders with seed + v*seed_stride (0: every view with `seed`) */
  uint64_t sample_index_base; /* index of every pixel's first sample */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* as RptRayQuery: GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused */
} RptViewQuery;
int rptgpu_render_views(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                        double* out /* [n_views][height][width][3], host */);
/* The same into device memory, f64 or (out_is_f32 != 0) f32 of the same layout; `views` stays in host memory.  `stream`
 * and the synchronisation rule are rptgpu_trace_rays_device's. */
int rptgpu_render_views_device(rptgpu_scene* h, uint64_t n_views, const RptView* views /* host */, const RptViewQuery* q,
                               void* d_out, int out_is_f32, void* stream);
/* A SEED PER VIEW (seeds[v] in place of seed + v*seed_stride: resuming a data set, rendering one view of an earlier job
 * again, seeds from the caller's own generator): rptgpu_render_views_seeded and rptgpu_render_views_seeded_device, optional
 * additions within ABI version 7 that are detected by symbol — declared and defined in rpt_gpu_views_seeded.h, which this
 * file includes at its end. */

/* ---- the first hit itself, for rays the caller supplies and for batches of views: distance, normal, object, position and
 * albedo on host or device memory — depth sensors and lidar, picking, collision against the scene, callers that shade their
 * own hits, the points and normals rptgpu_bake_ao and rptgpu_bake_probes consume; depth, normal, albedo and object maps of
 * cube maps, light fields, orthographic and panoramic views.  Additions within ABI version 7, detected by symbol (dlsym
 * "rptgpu_first_hits", "rptgpu_render_views_aov").  Both are DEFINED by rptgpu_closest_hit and run the closest-hit query of
 * a render — rpt_extend's closest_hit, or the per-tree query for scenes with deep trees —, so a caller may replace
 * rptgpu_closest_hit plus host arithmetic by them and keep every bit.
 * FIRST HITS.  Ray i is origins[3i..], dirs[3i..] (f64, xyz interleaved), used as given: no normalisation, t_min = 1e-12, no
 * origin offset — rptgpu_closest_hit's rules.  With (t_i, n_i, obj_i) = what rptgpu_closest_hit returns for ray i:
 *   t[i]           = t_i                  (+inf on a miss; a NaN record — MonomialSurface reports one — stays NaN)
 *   normal[i][c]   = n_i[c]
 *   object[i]      = obj_i                (-1 on a miss)
 *   position[i][c] = origins[i][c] + t_i * dirs[i][c] on a hit (obj_i >= 0): one multiply, then one add, never contracted
 *                    (Ray::at, shape.rs:59-61 — rptgpu_render_aov's expression); +0.0 on a miss
 *   albedo[i][c]   = objects[obj_i].material.color[c] on a hit; +0.0 on a miss
 * A channel that `channels` does not name is not computed, its pointer is not read and its array is not written.  A ray's
 * result depends on that ray and the scene and on nothing else: not on the other rays of the call, on their order, or on
 * the pieces the library cuts the call into.  Input and output arrays must not overlap (not checked).  After a live update
 * (rptgpu_scene_set_objects, _set_mesh, _set_group) the results are those of a handle freshly created from the updated
 * scene.  48 B in and 8 / 24 / 4 / 24 / 24 B out per ray and channel (100 B with all five).
 * ROUTE.  Scenes walked in-kernel: ONE kernel (rpt_first_hits) reads the caller's ray, finds its hit and writes the named
 * channels straight into the caller's arrays; nothing goes through the path state.  Scenes with deep trees: rpt_raygen_rays
 * lays a piece of the rays into the path state, the per-tree closest-hit query of a render runs over them (queues, ray sort,
 * persistent traversal, the generic walker for trees of trees), rpt_hits_store writes the named channels.  A host caller's
 * piece is staged on the device and runs the same kernels: no transpose on the CPU.  RPT_FLAG_GENERAL_TRAVERSAL and
 * RPT_FLAG_PROFILE_KERNELS are honoured, RPT_FLAG_WAVEFRONT changes nothing.  RptStats: kernel_launches[RPT_K_EXTEND] advances
 * by the queries (one per piece; kernel_ms[RPT_K_EXTEND] under RPT_FLAG_PROFILE_KERNELS) and total_ms by the call's wall time;
 * extend_rays, shadow_rays and samples do not advance, as rptgpu_closest_hit advances none of them.  There is no CPU
 * fallback: RPTGPU_E_NO_DEVICE.  RPTGPU_HITS_PIECE (environment, read per call; tests): the rays per piece.
 * VIEWS.  rptgpu_render_views_aov is rptgpu_render_aov's sums for every view of a batch: every array of RptAovBuffers is
 * [n_views][height][width] (x 3 where that struct says so), v in the order of `views`, and every element is written (a
 * pixel without a hit: 0 everywhere, object = -1).  For view v, pixel p and s = 0 .. iterations-1 ascending, the ray is
 * EXACTLY the ray rptgpu_render_views makes for (v, p, s) — the expressions of its block above, drawn from the stream keyed
 * by seed + v*seed_stride with the counter (p, sample_index_base + s, draw block) —, and steps 2 to 4 of rptgpu_render_aov's
 * contract follow: the sums are f64, start at +0.0 and add in ascending sample order; object is that of the call's first
 * sample.  max_bounces and exposure_value are not read.  So view v under RPT_VIEW_PERSPECTIVE is rptgpu_render_aov of its
 * camera over the full frame with seed + v*seed_stride, bit for bit; under the two other projections it is the header's
 * rays through rptgpu_closest_hit, folded in that order.  A view's buffers depend on that view, the query and the scene and
 * on nothing else.  The call always runs the wavefront kernels over rptgpu_render_views' pieces of consecutive (view, pixel)
 * indices (RPTGPU_VIEWS_PIECE; whatever the views' seeds), each piece's samples in passes of
 * rpt_raygen_views (views with seeds that differ: rpt_raygen_views_seeded), the closest-hit query (rpt_extend, or the per-tree query) and rpt_views_aov_fold, which keeps index j's
 * sums in the output arrays at j between passes.  RPT_FLAG_GENERAL_TRAVERSAL is honoured and changes no bit; RptStats:
 * total_ms only.
 * NOT IN SCOPE: a max_t cut or an early-out in the closest-hit query; multi-hit (primitive ids, barycentrics and a group's
 * child are a call of their own that joins on T and OBJECT: rptgpu_hit_surface, rpt_gpu_hit_surface.h); the tile partition and multi-GPU (a caller shards the rays or the views: a result
 * depends on nothing else); the device-resident Buffer and the denoiser for views; the persistent kernel; rptgpu_closest_hit
 * itself, which stays as it is and is not routed through this code.
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work, with a detail naming the reason and with the output arrays
 * untouched.  rptgpu_first_hits: a NULL RptHitQuery or RptHitArrays, a wrong struct_size of either, channels == 0 or an
 * unknown RPT_HIT_* bit, reserved != 0, a named channel whose pointer is NULL, a precision_mode other than
 * RPT_PRECISION_F64_STRICT, RPT_FLAG_PERSISTENT (the persistent kernel makes its rays from a camera), NULL origins or dirs
 * with n > 0, a NULL handle.  rptgpu_render_views_aov: rptgpu_render_views' refusals for the query and the views,
 * rptgpu_render_aov's for the buffers.  RPTGPU_E_COMM for an abandoned handle.  n == 0 / n_views == 0 returns RPTGPU_OK. */
enum { RPT_HIT_T = 1u, RPT_HIT_NORMAL = 2u, RPT_HIT_OBJECT = 4u, RPT_HIT_POSITION = 8u, RPT_HIT_ALBEDO = 16u };
typedef struct RptHitQuery {
  uint32_t struct_size;       /* sizeof(RptHitQuery) */
  uint32_t channels;          /* RPT_HIT_* wanted, at least one */
  uint32_t precision_mode;    /* RPT_PRECISION_F64_STRICT */
  uint32_t flags;             /* GENERAL_TRAVERSAL, PROFILE_KERNELS honoured; PERSISTENT refused */
} RptHitQuery;
typedef struct RptHitArrays {   /* one array per channel; a channel not named: pointer not read, array not written */
  uint32_t struct_size;       /* sizeof(RptHitArrays) */
  uint32_t reserved;          /* 0 */
  double* t;                  /* [n] */
  double* normal;             /* [n][3] */
  int32_t* object;            /* [n] */
  double* position;           /* [n][3] */
  double* albedo;             /* [n][3] */
} RptHitArrays;
int rptgpu_first_hits(rptgpu_scene* h, uint64_t n, const double* origins /* [n][3] */, const double* dirs /* [n][3] */,
                      const RptHitQuery* q, const RptHitArrays* out /* host arrays */);
/* The same with every array in device memory (the two structs stay in host memory); `stream` and the synchronisation rule
 * are rptgpu_trace_rays_device's (NULL means NO stream, not the null stream). */
int rptgpu_first_hits_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, const RptHitQuery* q,
                             const RptHitArrays* d_out /* device arrays */, void* stream);
/* (rptgpu_render_views_aov[_device] are declared behind RptAovBuffers, below) */

/* ---- host utility: KdTree::new (kdtree.rs:108-119, construct kdtree.rs:235-345) over n
 * axis-aligned boxes (p_min xyz, p_max xyz interleaved: 6 doubles per box).  Returns the
 * flattened tree through malloc'ed arrays the caller releases with rptgpu_free.
 * Node i: split[i], info[i] = axis (0..2) for inner nodes or 3 for a leaf, a[i] = index of
 * the left child (right = a[i]+1) for inner nodes or first entry in refs for a leaf,
 * b[i] = number of refs for a leaf (0 for inner nodes).  Children are visited left first,
 * nodes are numbered in the order they are created by a depth-first construction. */
typedef struct RptKdTree {
  uint64_t num_nodes;
  uint64_t num_refs;
  uint32_t max_depth;
  uint32_t regular; /* 1 if every split plane lies inside its node's cell (rptgpu_kdtree_build only;
                       the device's compact traversal requires it, otherwise the general one runs) */
  double* split;
  uint32_t* info;
  uint32_t* a;
  uint32_t* b;
  uint32_t* refs;
} RptKdTree;
int rptgpu_kdtree_build(const double* boxes, uint64_t n, RptKdTree* out);
/* The same tree — node for node, entry for entry — built on HIP device `device` (events sorted once per axis, one
 * round of scans and stable scatters per tree level).  rptgpu_scene_create uses it by itself for trees of at least
 * RPTGPU_DEVICE_BUILD_MIN primitives (default 32768).  RPTGPU_E_INVALID_ARGUMENT for inputs it does not take (fewer
 * than 16 boxes, non-finite coordinates): build those with rptgpu_kdtree_build. */
int rptgpu_kdtree_build_device(const double* boxes, uint64_t n, int device, RptKdTree* out);
void rptgpu_kdtree_free(RptKdTree* tree);

/* ---- diagnostics: evaluate one function of include/rpt_math.h on the DEVICE for n arguments
 * (host arrays).  fn: 0 exp, 1 log, 2 atan, 3 sin, 4 cos (|x| < 3pi/4), 5 acos, 6 atan2(y, x),
 * 7 y / x computed through the kernels' shared-reciprocal division (must equal IEEE y / x).
 * 8-11 y / x computed in the kernels' batches of 2, 3, 4 and 6 interleaved divisions (must equal IEEE y / x).
 * 12, 13 the draws of a hit in the persistent kernel's draw-first shading (illuminate's triangle index and (u, v) pair,
 * then gen_bool(f), u_theta and the +-1 pair of sample_f): 12 as the kernels take them, 13 the same sequence drawn one
 * next_u64 at a time (must be equal).  x and out hold raw 64-bit words, nine per element, n = 9 * elements (y is not
 * read; words behind the last whole element come back 0).  In, x[9e + k]: 0 seed, 1 pixel (< 2^32), 2 sample, 3 the
 * stream's draw counter at the hit (< 2^31; the cached half of an odd counter is derived on the device), 4 the light's
 * triangle count (1 .. 2^32 - 1), 5 its sampling zone (>= 2^62), 6 f as an f64 in [0, 1], 7 flags: bit 0 sample_f
 * runs (the path goes on), bit 1 gen_bool's threshold comes from a table of the material's constants, as the kernels
 * that hold one have it, 8 unused.  Out, out[9e + k]: 0 the triangle's index, 1-2 the (u, v) pair kept, 3 u_theta's
 * draw (2^63 when none is taken), 4-5 the +-1 pair kept, 6 gen_bool's answer (0 / 1), 7 the counter behind the hit,
 * 8 the half cached there (0 when the counter is even).  Elements outside these ranges: RPTGPU_E_INVALID_ARGUMENT.
 * Lets the parity tests show that the kernels' transcendental functions are bit-identical to
 * the host's. */
int rptgpu_eval_math(rptgpu_scene* h, int fn, uint64_t n, const double* x, const double* y,
                     double* out);

/* ---- device-resident Buffer (reference src/buffer.rs): SURVEY §8f rank 1.
 * Keeps every batch of Renderer::sample on the GPU so that iterative_render (renderer.rs:103-115)
 * needs no host round trip per batch; image() and variance() follow buffer.rs:43-93 exactly:
 * per-pixel batch means summed in insertion order, box filter over (2r+1)^2 neighbours visited
 * x-outer / y-inner, gamma 2.2 + clamp + truncation to u8 (color.rs:18-24). */
typedef struct rptgpu_buffer rptgpu_buffer; /* opaque; belongs to the scene handle it was made from */
int rptgpu_buffer_create(rptgpu_scene* h, uint32_t width, uint32_t height, uint32_t filter_radius,
                         rptgpu_buffer** out);
void rptgpu_buffer_destroy(rptgpu_buffer* b);
/* Renderer::sample(iterations, &mut buffer): render one batch (params->width/height must match the
 * buffer) and Buffer::add_samples it (buffer.rs:32-40), all on the device. */
int rptgpu_buffer_sample(rptgpu_buffer* b, const RptCamera* camera, const RptRenderParams* params);
/* Buffer::image (buffer.rs:43-56): out_rgb8 = height*width*3 bytes (host). */
int rptgpu_buffer_image(rptgpu_buffer* b, uint8_t* out_rgb8);
/* Buffer::variance (buffer.rs:59-73): mean over pixels of the per-pixel sample variance of the batch means. */
int rptgpu_buffer_variance(rptgpu_buffer* b, double* out_variance);
/* number of add_samples calls so far */
int rptgpu_buffer_num_batches(const rptgpu_buffer* b, uint32_t* out);

/* ---- adaptive sampling on the device-resident Buffer.  Additions within ABI version 7, detected by
 * symbol (dlsym "rptgpu_buffer_sample_adaptive").  Per pixel p the buffer keeps n_p, the batches p holds, and a Welford
 * state over their values x (accum / iterations * 2^EV, f64): n += 1, d = x - m, m += d / n, M2 += dot(d, x - m).
 * After an adaptive round each pixel sampled in it RETIRES when n >= min_batches and (M2 / (n - 1)) / n <= t * t,
 * t = abs_tol + rel_tol * ((m.x + m.y) + m.z) (a NaN never retires).  A retired pixel is never sampled again, so pixel
 * p holds exactly batches 0 .. n_p - 1 of the buffer, and image() / variance() are buffer.rs:59-93 with per-pixel
 * lengths (Buffer::add_sample, buffer.rs:25-30).  Random numbers are keyed by (pixel, sample index), so p's batches are
 * bit for bit those of full-frame renders at the same sample_index_base. */
typedef struct RptAdaptive {
  uint32_t struct_size;    /* sizeof(RptAdaptive) */
  uint32_t min_batches;    /* >= 2 */
  double abs_tol, rel_tol; /* finite, >= 0 */
} RptAdaptive;
/* One batch of params->iterations samples for the pixels still active (all pixels at first), recorded as one more
 * batch, then the stopping rule; *out_active = the pixels active afterwards.  No pixel active: nothing is rendered or
 * recorded, *out_active = 0.  RPTGPU_E_INVALID_ARGUMENT for a bad RptAdaptive (struct_size, min_batches < 2, a
 * negative or non-finite tolerance — checked first, so also without a buffer), part_count > 1 or a size mismatch.
 * rptgpu_buffer_sample may be mixed in while every pixel is active and is refused once one has retired. */
int rptgpu_buffer_sample_adaptive(rptgpu_buffer* b, const RptCamera* camera, const RptRenderParams* params,
                                  const RptAdaptive* a, uint32_t* out_active);
/* n_p per pixel: height*width uint32 (host), row-major */
int rptgpu_buffer_sample_counts(const rptgpu_buffer* b, uint32_t* out_counts);
/* the sum of each pixel's batch values (samples[index].iter().sum(), buffer.rs:84): height*width*3 doubles (host); the
 * linear mean of pixel p is its sum / n_p */
int rptgpu_buffer_totals(const rptgpu_buffer* b, double* out_totals);

/* ---- first-hit feature buffers ("AOVs"): what a denoiser, a compositor or a picking tool asks of a frame
 * besides its colour.  Additions within ABI version 7, detected by symbol (dlsym "rptgpu_render_aov").
 * One stateless call.  For each pixel p the call owns (the tile partition of RptRenderParams, as in rptgpu_render_batch)
 * and each sample index s = sample_index_base .. sample_index_base + iterations - 1, in ascending order:
 *   1. ray = the camera ray of (p, s): renderer.rs:132-139 + Camera::cast_ray (camera.rs:64-81) with the draws of the
 *      Philox stream (seed, p, s) — the very ray the colour sample (p, s) of rptgpu_render_batch starts with (jitter, then
 *      the lens disc when aperture > 0);
 *   2. (t, n, obj) = get_closest_hit(ray) (renderer.rs:211-220): what rptgpu_closest_hit returns for that ray;
 *   3. if it hit (obj >= 0): hits += 1, depth += t, normal += n, albedo += objects[obj].material.color,
 *      position += ray.at(t), ray.at(t) = origin + t * dir per component (shape.rs:59-61: one multiply, then one add, never
 *      contracted).  A miss adds nothing;
 *   4. object = obj of the call's FIRST sample (s = sample_index_base), -1 on a miss.
 * All sums are f64, start at +0.0 and add in ascending sample order, so a result is defined to the bit (a lone -0.0
 * comes out as +0.0 + -0.0 = +0.0).  The outputs are SUMS plus the hit count: the caller divides (mean = sum / hits) and
 * may add the sums of consecutive calls.  max_bounces, exposure_value and collective are ignored.  Pixels outside the
 * caller's part get 0 everywhere and object = -1.  After a live update (rptgpu_scene_set_objects) the buffers are those
 * of a handle freshly created from the updated scene.
 * RPT_FLAG_WAVEFRONT, RPT_FLAG_PERSISTENT and RPT_FLAG_GENERAL_TRAVERSAL choose the route as they do for a render (one
 * fused kernel, rpt_aov, or rpt_raygen + the per-tree closest-hit query + rpt_aov_fold in passes) and never change a bit.
 * RPTGPU_E_INVALID_ARGUMENT, checked before any device work and with a detail naming the reason: a NULL handle / camera /
 * params / out, a wrong struct_size, an unknown channel bit, hits == NULL, a named channel whose pointer is NULL,
 * iterations == 0, width * height == 0, a precision_mode other than RPT_PRECISION_F64_STRICT, an abandoned handle. */
enum { RPT_AOV_DEPTH = 1u, RPT_AOV_NORMAL = 2u, RPT_AOV_ALBEDO = 4u, RPT_AOV_POSITION = 8u, RPT_AOV_OBJECT = 16u };
typedef struct RptAovBuffers {        /* host arrays, row-major, top row first                                  */
  uint32_t struct_size;               /* sizeof(RptAovBuffers)                                                  */
  uint32_t channels;                  /* RPT_AOV_* wanted; a channel not named is not computed, its pointer not */
                                      /* read, its array not written                                            */
  uint32_t* hits;                     /* width*height, ALWAYS written, must not be NULL                         */
  double* depth;                      /* width*height                                                           */
  double* normal;                     /* width*height*3                                                         */
  double* albedo;                     /* width*height*3                                                         */
  double* position;                   /* width*height*3                                                         */
  int32_t* object;                    /* width*height                                                           */
} RptAovBuffers;
int rptgpu_render_aov(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* params, const RptAovBuffers* out);
/* rptgpu_render_aov's sums for every view of a batch: the contract stands with rptgpu_first_hits, above */
int rptgpu_render_views_aov(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                            const RptAovBuffers* out /* host arrays, [n_views][height][width](x 3) */);
/* The same into device arrays; `views`, q and the struct stay in host memory.  `stream` as for rptgpu_trace_rays_device. */
int rptgpu_render_views_aov_device(rptgpu_scene* h, uint64_t n_views, const RptView* views /* host */, const RptViewQuery* q,
                                   const RptAovBuffers* d_out /* device arrays */, void* stream);
/* A SEED PER VIEW: rptgpu_render_views_aov_seeded and rptgpu_render_views_aov_seeded_device, in rpt_gpu_views_seeded.h. */

/* ---- feature-guided denoising of the device-resident Buffer: an edge-avoiding a-trous wavelet filter
 * (Dammertz et al. 2010) with the variance guidance of SVGF (Schied et al. 2017), run wholly on the device on what the
 * buffer already holds.  Additions within ABI version 7, detected by symbol (dlsym "rptgpu_buffer_denoise").
 *
 * FEATURES.  rptgpu_buffer_features computes what rptgpu_render_aov computes for (camera, params) with the channels
 * DEPTH | NORMAL | ALBEDO | POSITION — the same sums and hits, by the same two routes, bit for bit — and leaves them in
 * device arrays the buffer owns; nothing of them travels to the host.  A later call replaces them (a failed one leaves
 * the buffer without features).  params->width / height must be the buffer's and part_count <= 1; the other refusals are
 * rptgpu_render_aov's.  The sample range is the caller's: sample_index_base = 0 with a few iterations gives the first
 * hits of the rays the buffer's first colour samples started with.  rptgpu_buffer_feature_sums copies the held sums out
 * through an RptAovBuffers (tests, tools); `object` is not held: naming RPT_AOV_OBJECT is refused.
 *
 * THE FILTER, defined to the bit.  All arithmetic is IEEE f64, never contracted; exp is rpt_exp of include/rpt_math.h;
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; |a|^2 = dot(a, a); every sum starts at +0.0 and a vector sum adds per
 * component; taps are visited x-outer / y-inner, both ascending (the box filter's order, buffer.rs:80-81); a tap outside
 * the frame is skipped (it adds nothing to any sum).
 *   Inputs of pixel p, with n = (double)n_p and h = the held hit count of p:
 *     c_p = total_p / n per component;  u_p = (M2_p / (n - 1.0)) / n  (the variance of that mean; M2 sums the channels);
 *     hit_p = h > 0, and where hit_p, each per component: N_p = normal_p / (double)h, P_p = position_p / (double)h,
 *     Z_p = depth_p / (double)h, A_p = albedo_p / (double)h.
 *   Variance prefilter, g(-1) = g(1) = 0.25, g(0) = 0.5, over q = p + (dx, dy), dx, dy in -1..1:
 *     a = a + (g(dx) * g(dy)) * u_q;  s = s + g(dx) * g(dy);  then v_p = a / s.
 *   Level l = 0 .. levels - 1, step = 2^l, k(0) = 0.375, k(-1) = k(1) = 0.25, k(-2) = k(2) = 0.0625, over
 *   q = p + step * (dx, dy), dx, dy in -2..2, with w0 = k(dx) * k(dy):
 *     the centre tap (dx = dy = 0):  w = w0, no exponent is evaluated;
 *     any other tap is skipped when hit_q != hit_p; otherwise, with d = c_q - c_p,
 *       e = |d|^2 / (sigma_color * sigma_color * (v_p + v_q) + 1e-12)      [(sc * sc) * (v_p + v_q), then + 1e-12]
 *       and where both are hits, with t = 1.0 - dot(N_p, N_q) and D = A_q - A_p:
 *         en = (t > 0.0 ? t : 0.0) / sigma_normal
 *         ez = fabs(dot(N_p, P_q - P_p)) / (sigma_depth * Z_p + 1e-12)
 *         ea = |D|^2 / (sigma_albedo * sigma_albedo)
 *         e  = e + ((en + ez) + ea);
 *       the tap is skipped unless e >= 0.0 and e < +inf (a NaN fails both: a NaN or infinite pixel keeps its own value
 *       and never spreads); else w = w0 * exp(-e);
 *     a tap that is not skipped adds  C = C + w * c_q,  W = W + w,  V = V + (w * w) * v_q;
 *     then c'_p = C / W per component and v'_p = V / (W * W); (c', v') are the next level's (c, v); the features stay.
 *   out_linear = the last level's c', out_linear[(y*width+x)*3+ch]; out_rgb8 = color_bytes of it (color.rs:18-24, through
 *   the thresholds rptgpu_buffer_image uses).  Either may be NULL, not both.
 * The buffer's own state (totals, counts, Welford state, batches, features) is not modified: image(), variance() and
 * totals() give the same bits before and after.  A buffer with retired pixels (uneven n_p) is filtered like any other.
 * RPTGPU_E_INVALID_ARGUMENT before any device work, with a detail naming the reason: a NULL RptDenoise, a wrong
 * struct_size, levels outside 1..8, a sigma that is not finite or not > 0 (these first, so also without a buffer); a
 * NULL buffer; both outputs NULL; no features held; fewer than two batches (every pixel holds min(batches, the count
 * it retired with >= 2) of them, and one batch has no variance); an abandoned handle (RPTGPU_E_COMM). */
typedef struct RptDenoise {
  uint32_t struct_size; /* sizeof(RptDenoise) */
  uint32_t levels;      /* 1 .. 8: a-trous passes, tap spacing 1, 2, 4, ... */
  double sigma_color, sigma_normal, sigma_depth, sigma_albedo; /* finite, > 0 */
} RptDenoise;
int rptgpu_buffer_features(rptgpu_buffer* b, const RptCamera* camera, const RptRenderParams* params);
int rptgpu_buffer_feature_sums(const rptgpu_buffer* b, const RptAovBuffers* out);
int rptgpu_buffer_denoise(rptgpu_buffer* b, const RptDenoise* d, double* out_linear, uint8_t* out_rgb8);

/* ---- particle systems: the reference's `rpt::ode` (src/ode.rs, src/ode/particle_system.rs) on the device.
 * Additions within ABI version 7: no earlier struct or signature changed, so a caller detects them by symbol
 * (dlsym "rptgpu_particles_integrate"), not by version.
 * A state is n particles: pos and vel are n*3 doubles (x, y, z per particle), as ParticleState's two Vec<DVec3>.
 * Every result is bit-identical to the reference's f64 arithmetic in its order of operations.
 * RPTGPU_E_INVALID_ARGUMENT: a NULL pointer with n > 0, n > RPT_PARTICLES_MAX_N, an unknown kind or flag, both
 * schedule flags, a forced single-workgroup schedule with n > RPT_PARTICLES_SINGLE_MAX, a time that is not finite, a
 * step that is not finite and > 0, or a (time, step) whose schedule never ends or has more than
 * RPT_PARTICLES_MAX_STEPS steps — the reference loops for ever on step <= 0 and on any step for which
 * `time - step == time` (time = 1, step = 1e-17); the library counts the steps with the reference's own f64
 * decrements before anything runs.  n == 0 returns RPTGPU_OK (after the checks of time and step).  There is no CPU
 * fallback: without a device the entry points return RPTGPU_E_NO_DEVICE. */
enum {
  RPT_PARTICLES_SOLID_GRAVITY = 0, /* SolidGravitySystem (particle_system.rs:42-62)                        */
  RPT_PARTICLES_MARBLES = 1,       /* MarblesSystem { radius } (particle_system.rs:64-127)                 */
  RPT_PARTICLES_CIRCLE = 2         /* SimpleCircleSystem, the reference's test system (:27-40)             */
};
enum {
  RPT_PARTICLES_FLAG_SINGLE_GROUP = 1u, /* force one workgroup for the whole call (state in LDS and registers) */
  RPT_PARTICLES_FLAG_GRID = 2u,         /* force one launch per RK4 stage over a grid of workgroups            */
  RPT_PARTICLES_SINGLE_MAX = 2048,      /* the most particles the single-workgroup schedule takes; by default it
                                           runs for n <= 256 and the grid schedule above that                  */
  RPT_PARTICLES_MAX_N = 715827882,      /* the most particles (points, arguments) of any call: INT_MAX / 3      */
  RPT_PARTICLES_MAX_STEPS = 67108864    /* the most RK4 steps one rk4_integrate call may take (2^26)           */
};
typedef struct RptParticleSystem {
  uint32_t kind;  /* RPT_PARTICLES_* */
  uint32_t flags; /* RPT_PARTICLES_FLAG_*, 0 = choose by n */
  double radius;  /* MarblesSystem::radius; ignored by the other kinds */
} RptParticleSystem;
/* ParticleSystem::time_derivative: out_dpos = vel, out_dvel = the accelerations (n*3 doubles each). */
int rptgpu_particles_time_derivative(int device, const RptParticleSystem* sys, uint64_t n, const double* pos,
                                     const double* vel, double* out_dpos, double* out_dvel);
/* ParticleSystem::rk4_integrate(&mut state, time, step) (particle_system.rs:10-24) — named without the digit so that
 * it reads as one identifier to every symbol scanner of the header: pos and vel are updated in
 * place.  The state is copied to the device once and back once, whatever the number of steps. */
int rptgpu_particles_integrate(int device, const RptParticleSystem* sys, uint64_t n, double* pos, double* vel,
                                   double time, double step);
/* MonomialSurface { height, exp: 4 }::closest_point (monomial_surface.rs:126-152) with the grid x = i / steps,
 * i = -steps..=steps (steps = 100 is closest_point, 10000 closest_point_precise): out = n*3 doubles. */
int rptgpu_monomial_closest_point(int device, double height, uint32_t steps, uint64_t n, const double* points,
                                  double* out);
/* diagnostics: the device's restatement of the platform libm's hypot (glibc 2.35, dbl-64), which closest_point uses for
 * x.hypot(z), evaluated for n argument pairs (host arrays) so that tests can compare it with the host's. */
int rptgpu_particles_eval_hypot(int device, uint64_t n, const double* x, const double* y, double* out);

/* ---- accounting ---- */
int rptgpu_get_stats(const rptgpu_scene* h, RptStats* out);
int rptgpu_reset_stats(rptgpu_scene* h);
/* name of kernel kind k as it appears in a rocprofv3 kernel trace */
const char* rptgpu_kernel_name(int k);

/* ---- optional additions within ABI version 7, detected by symbol: a seed per view for the batches of views ---- */
#include "rpt_gpu_views_seeded.h"
/* ---- ... and a denoised frame per view of a batch ---- */
#include "rpt_gpu_views_denoised.h"
/* ---- ... and the vertices of the paths rptgpu_trace_rays runs ---- */
#include "rpt_gpu_vertices.h"
/* ---- ... and a batch of views in the persistent path kernel, on request ---- */
#include "rpt_gpu_views_persistent.h"
/* ---- ... and caller-supplied rays and light probes in the persistent path kernel, on request ---- */
#include "rpt_gpu_rays_persistent.h"
/* ---- ... and the vertices of those rays' paths from the persistent path kernel, on request ---- */
#include "rpt_gpu_vertices_persistent.h"
/* ---- ... and the triangle, group child and barycentrics behind a ray's first hit ---- */
#include "rpt_gpu_hit_surface.h"
/* ---- ... and a lightmap baked from a mesh's UV charts: irradiance and ambient occlusion per texel ---- */
#include "rpt_gpu_lightmap.h"
/* ---- ... and such a map denoised with a filter guided by its own owner, position and normal channels ---- */
#include "rpt_gpu_lightmap_filter.h"
/* ---- ... and direct lighting (next-event estimation) at caller points and lightmap texels ---- */
#include "rpt_gpu_direct.h"
/* ---- ... and a baked lightmap read back at the first hits of the caller's rays ---- */
#include "rpt_gpu_lightmap_lookup.h"
/* ---- ... and a grid of baked SH9 probes read at points, at first hits and in views shaded from both ---- */
#include "rpt_gpu_probe_volume.h"

#ifdef __cplusplus
}
#endif
#endif /* RPT_GPU_H */
