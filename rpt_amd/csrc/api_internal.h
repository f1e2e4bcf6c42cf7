// api_internal.h — what the files behind the C ABI of include/rpt_gpu.h share: the handle, device buffers, the error
// convention and the entry points' frames (guarded; device_call around a call's kernels), the steps the calls over pieces
// share, the RCCL binding.  The ABI's implementation is split by concern
// (round 6; it was one 1 900-line api.cpp):
//   api_common.cpp   errors, the RCCL loader, kernel tables, version / strerror / stats
//   api_scene.cpp    RptSceneOptions, rptgpu_scene_create[_opts] (flatten, open the device, plan, apply, upload), the live
//                    updates of placements and materials, the kd-tree entry points
//   scene_plan.h     the plan: every object's route (obj_deep / obj_tris, their bits named in launch_limits.h), the scene's
//                    flags, the re-route after a live rebuild, and the flat path kernel's LDS layout (flat_layout.h) — pure
//                    host functions, read by creation and by every live update (tests/cpp/scene_plan_check.cpp)
//   api_render.cpp   workspace, the wavefront loop and the persistent launch (render_impl), render_batch[_device],
//                    rptgpu_closest_hit, rptgpu_eval_math; their launch and pass sizes come from render_plan.h.  Also the
//                    steps every driver of the wavefront kernels shares: the route (use_wavefront), a pass's size with
//                    its out-of-memory shrink (size_pass), the per-tree queries (reset_tree_counters, query_closest,
//                    query_visibility), the profiling event pairs, the end of a call (drain_call)
//   api_comm.cpp     communicator, rptgpu_render_batch_reduce (the library-owned exchange and its failure paths),
//                    rptgpu_render_batch_emulate_ranks
//   api_buffer.cpp   the device-resident Buffer
//   api_rays.cpp     rptgpu_trace_rays[_device]: the path drivers over rays the caller supplies, in pieces — and that piece
//                    loop itself (trace_ray_pieces), which the next file and api_vertices.cpp run too
//   api_probes.cpp   rptgpu_bake_probes[_device]: light probes (SH9 radiance, irradiance) through the same loop
//   api_views.cpp    rptgpu_render_views[_seeded][_device]: batches of perspective, orthographic and panoramic views through the
//                    same driver, in pieces of consecutive (view, pixel) indices, with one seed or a seed per view
//   api_views_denoise.cpp rptgpu_render_views_denoised[_device]: per batch the views driver into a device frame and one
//                    rpt_buffer_accumulate over all views, then the views' feature sums and the filter, one launch per step
//   api_occlusion.cpp rptgpu_occluded[_device], rptgpu_bake_ao[_device]: the caller's rays, or points x directions made on the
//                    device, through ONE visibility query of a render per pass (no depth loop), in pieces
//   api_direct.cpp   rptgpu_bake_direct[_device], rptgpu_bake_lightmap_direct[_device]: next-event estimation at the caller's
//                    points — every light's sample per (sample, point) slot made on the device, the visibility queries of a
//                    depth over the lights' queues, the fold — in the AO call's pieces and passes
//   api_hits.cpp     rptgpu_first_hits[_device], rptgpu_render_views_aov[_seeded][_device]: the first hit's record for the caller's rays
//                    (one fused kernel, or the per-tree closest-hit query, in pieces) and rptgpu_render_aov's sums for
//                    every view of a batch (raygen, closest-hit query and fold in passes over render_views' pieces)
//   api_vertices.cpp rptgpu_trace_vertices[_device]: api_rays.cpp's loop with a vertex sink in each piece's RaySource — the
//                    drivers then also carry every path's vertices into the caller's arrays
//   api_surface.cpp  rptgpu_hit_surface[_device]: api_hits.cpp's first-hit query per piece (plan_hit_pieces, hit_piece), then
//                    rpt_hit_surface, the resolve walk that names the triangle, the barycentrics and the group's child
//   api_lightmap.cpp rptgpu_bake_lightmap[_device]: the triangles' uv charts rasterised into an owner map, then per piece of
//                    texels the interpolation and compaction, the probe and AO calls' own device work over the compacted
//                    points (enqueue_probes, enqueue_ao), the scatter; the dilation over the whole map (the kernels:
//                    kernels_lightmap.hip; the sizes: lightmap_plan.h)
//   api_lightmap_filter.cpp rptgpu_filter_lightmap[_device]: a baked map through the geometry-guided a-trous filter — the
//                    guides as columns, one launch per level, the columns written back, then api_lightmap.cpp's dilation
//                    rounds (the kernels: kernels_lightmap_filter.hip; the sizes: lightmap_filter_plan.h)
//   api_lightmap_lookup.cpp rptgpu_lookup_lightmap[_device]: a baked map read back at the caller's rays' first hits — per piece
//                    api_hits.cpp's first-hit query and api_surface.cpp's resolve walk into arrays the handle keeps, then
//                    rpt_lightmap_lookup, one lane per ray (the kernel: kernels_lightmap_lookup.hip; the sizes:
//                    lightmap_lookup_plan.h)
//   api_probe_volume.cpp rptgpu_sample_probe_volume[_device], rptgpu_lookup_probe_volume[_device]: a grid of SH9 probes read at the
//                    caller's points (one kernel per piece) and at the first hits of its rays (api_hits.cpp's query, then one
//                    kernel), and rptgpu_render_views_probe_lit[_device] through api_lightmap_lookup.cpp's views driver with
//                    the volume's step (the kernels: kernels_probe_volume.hip, kernels_probe_volume_views.hip; the sizes:
//                    probe_volume_plan.h)
//   api_mesh.cpp     rptgpu_scene_set_mesh[_device]: a deformed mesh's records and tree into the second set of the geometry
//                    arrays, then the swap (the kernels: mesh_update.hip)
//   api_group.cpp    rptgpu_scene_set_group[_device]: a group's moved children — their records, the group's tree — the same
//                    way (the kernels: group_update.hip); tree_splice.h holds what both files share: the first refusals,
//                    the lap timer, the tree's rebuild, the spare-set storage, the swap and the re-route
//   api_aov.cpp      rptgpu_render_aov: first-hit feature buffers (argument checks, pass loop, copy_aov_out); its device
//                    half also fills the features a Buffer holds for rptgpu_buffer_denoise
//   channel_plan.h   what the calls that return named channels into the caller's arrays share (hits, AOVs, vertices, hit
//                    surfaces, lightmaps, lookups, probe volumes): one table per output struct beside its planner, and the
//                    null check, the staging layout, the piece offsets and the copy out that walk it
// No compute happens on the host; if there is no HIP device every compute entry point returns RPTGPU_E_NO_DEVICE (there is
// no CPU fallback by design).
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rpt_gpu.h"
#include "device_types.h"
#include "host_scene.h"
#include "kernels.h"
#include "render_plan.h"
#include "surface_plan.h"
#include "lightmap_plan.h"
#include "lightmap.h"
#include "lightmap_filter_plan.h"
#include "lightmap_filter.h"
#include "lightmap_lookup_plan.h"
#include "lightmap_lookup.h"
#include "lightmap_views.h"
#include "probe_volume_plan.h"
#include "probe_volume.h"

namespace rptapi {

extern thread_local std::string g_create_error;

struct HipError {
  hipError_t e;
  const char* what;
  int line;
  const char* file = "";
};
// the file's name without its directories, for error messages
constexpr const char* rpt_basename(const char* path) {
  const char* b = path;
  for (const char* p = path; *p; p++)
    if (*p == '/') b = p + 1;
  return b;
}
#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t _e = (expr);                             \
    if (_e != hipSuccess) throw HipError{_e, #expr, __LINE__, rptapi::rpt_basename(__FILE__)}; \
  } while (0)

// owning device allocation: released by the destructor, moved but never copied
template <class T> struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p; n = o.n;
      o.p = nullptr; o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void alloc(size_t count) {
    if (count <= n && p) return;
    release();
    HIP_TRY(hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)));
    n = count;
  }
  void upload(const std::vector<T>& v, hipStream_t st) {
    alloc(v.size());
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

constexpr int MAX_EVENT_PAIRS = 4096;
// ---- RCCL, opened on first use (the library has no link-time dependency on it) -----------------------------
// the handful of declarations of <rccl/rccl.h> that are used here
struct RcclUniqueId { char internal[128]; };
typedef void* RcclComm;
struct Rccl {
  void* so = nullptr;
  int (*GetUniqueId)(RcclUniqueId*) = nullptr;
  int (*CommInitRank)(RcclComm*, int, RcclUniqueId, int) = nullptr;
  int (*CommDestroy)(RcclComm) = nullptr;
  int (*CommAbort)(RcclComm) = nullptr;
  int (*Reduce)(const void*, void*, size_t, int /*ncclDataType_t*/, int /*ncclRedOp_t*/, int, RcclComm, hipStream_t) = nullptr;
  // the gather (optional: without them rptgpu_render_batch_reduce falls back to the reduce)
  int (*Send)(const void*, size_t, int, int /*peer*/, RcclComm, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int /*peer*/, RcclComm, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommGetAsyncError)(RcclComm, int*) = nullptr; // optional: polled while a batch's collective is in flight
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
  std::string why;
};
constexpr int RCCL_FLOAT32 = 7, RCCL_SUM = 0, RCCL_IN_PROGRESS = 7; // ncclFloat32, ncclSum, ncclInProgress (rccl.h)
Rccl& rccl(); // opened on first use (api_common.cpp)

} // namespace rptapi
using namespace rptapi;

struct rptgpu_scene {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string error;
  // flattened scene on the device
  DevBuf<rptdev::Inst> insts;
  DevBuf<rptdev::Tree> trees;
  DevBuf<rptdev::KdNode> nodes;
  DevBuf<uint32_t> refs;
  DevBuf<rptdev::Tri> tris;
  DevBuf<rptdev::TriX> trix;
  DevBuf<rptdev::LeafBox> lbox;
  DevBuf<rptdev::LeafBox> obj_box; // flat scenes' object filter (FlatLayout::obj_box / obj_grid)
  DevBuf<double> obj_grid;
  DevBuf<rptdev::Material> materials;
  DevBuf<rptdev::Light> lights;
  DevBuf<double> env_texels;
  rptdev::Scene dscene{};
  // workspace
  DevBuf<double> ray, hit, rec, shadow, accum, out_full;
  DevBuf<int32_t> hit_obj;
  DevBuf<uint32_t> draw, counters, pixels;
  uint64_t ws_cap = 0;
  uint64_t ws_rec_cols = 0;            // columns of the depth-record pool (PathState::rec)
  bool ws_stale = false;               // rptgpu_scene_set_mesh made a tree deeper than the traversal columns were sized for:
                                       // the next ensure_workspace makes them again (api_mesh.cpp)
  DevBuf<uint32_t> rec_parent, last_col;
  DevBuf<double> ray_next;             // dense path state of the NEXT depth (PathState: rpt_shade writes, the host swaps)
  DevBuf<uint32_t> draw_next, pid, pid_next, col, col_next;
  // in-kernel-traversal scenes: the paths of a depth are re-ordered by ray key (kernels/wf_sort_key.inc ray_sort_key)
  bool path_reorder = false;
  uint32_t path_reorder_min = RPT_PATH_REORDER_MIN; // ... when a depth has at least this many (RPTGPU_PATH_REORDER_MIN: tests)
  double scene_bounds[6] = {0, 0, 0, 1, 1, 1};
  DevBuf<uint32_t> path_order;
  DevBuf<double> next_rows;           // [cap][8]: the survivors' next state as rows (PathState::next_rows)
  double rec_ratio = 0.0;              // record columns a path of this scene needs on average, as measured by the passes so
  uint32_t rec_ratio_bounces = 0xffffffffu; // far at this max_bounces (0 = not measured yet: the next pass measures)
  uint64_t ws_fail_paths = 0;          // the smallest pass (paths) whose workspace did not fit on this device so far; 0 = none
  DevBuf<double> prec;                 // persistent kernel: depth records [threads][bounces][8]
  DevBuf<double> lbuf;                 // persistent kernel: radiance of every sample of a launch [spp][3][npix]; opt.lbuf_bytes caps
                                       // it, larger batches run as several launches
  DevBuf<unsigned long long> pcounters; // [0] closest-hit rays [1] shadow rays
  DevBuf<double> rays_o, rays_d, rays_out; // rptgpu_trace_rays: a piece of the host caller's rays and of their results (api_rays.cpp)
  DevBuf<uint32_t> ray_ids;            // ... and the piece's stream ids (the caller's, or the rays' indices); rptgpu_bake_probes
                                       // stages a piece of probes in the same four (api_probes.cpp)
  DevBuf<uint8_t> occ_out;             // rptgpu_occluded: a piece of a host caller's answers (api_occlusion.cpp)
  DevBuf<double> hits_out;             // rptgpu_first_hits: a piece of a host caller's records, the named channels back to back (api_hits.cpp)
  DevBuf<double> surface_out;          // rptgpu_hit_surface: the handle's pair of T and OBJECT and a piece of a host caller's records (api_surface.cpp, surface_plan.h layout)
  DevBuf<double> surf_defer, surf_frame; // ... and rpt_hit_surface's columns (surface_plan.h columns), as high as gen_levels / gen_frames
  rptsurface::Columns surf_cols{};
  // rptgpu_bake_lightmap (api_lightmap.cpp): the owner map of the call, the list of triangles with large boxes, a piece's scan
  // with its scratch, its compacted arrays (lightmap_plan.h compact), the dilation's second copy and its filled flags, and
  // a host caller's triangles and named channels, staged whole
  DevBuf<uint32_t> lm_owner, lm_large, lm_scan;
  DevBuf<uint8_t> lm_scan_tmp, lm_filled;
  DevBuf<double> lm_compact, lm_pong, lm_tris, lm_stage;
  // rptgpu_filter_lightmap (api_lightmap_filter.cpp): the filter's columns with the dilation's second copy inside them
  // (lightmap_filter_plan.h workspace) and a host caller's arrays, staged whole (stage)
  DevBuf<double> lf_ws, lf_stage;
  // rptgpu_lookup_lightmap (api_lightmap_lookup.cpp): a piece's arrays (lightmap_lookup_plan.h layout), the call's binding
  // records and object-to-binding table, and a host caller's uvs, maps and valid bytes, staged whole (stage_binding)
  DevBuf<double> lk_piece, lk_stage;
  DevBuf<rptlookup::Binding> lk_bindings;
  DevBuf<int32_t> lk_table;
  // rptgpu_sample_probe_volume, rptgpu_lookup_probe_volume, rptgpu_render_views_probe_lit (api_probe_volume.cpp): a piece's
  // arrays (probe_volume_plan.h layout) and a host caller's coefficients and valid bytes, staged whole (stage_volume)
  DevBuf<double> pv_piece, pv_stage;
  DevBuf<double> vertices_out;         // rptgpu_trace_vertices: a piece of a host caller's records, the named channels back to back (api_vertices.cpp)
  DevBuf<rptdev::View> view_recs;     // rptgpu_render_views: the call's views (api_views.cpp)
  DevBuf<uint64_t> view_seeds;         // ... their seeds, when the views have seeds of their own,
  DevBuf<uint64_t> ray_seeds;          // ... and then the seed of each index of a piece, beside ray_ids
  DevBuf<uint32_t> view_of;            // ... in the persistent kernel: the view of each index of a piece (ViewRays::view_of)
  // rptgpu_render_views_denoised's working set over the batch's n_views * width * height indices (api_views_denoise.cpp;
  // the bytes: rptplan::views_denoise_plan), grown on demand: the Buffer's per-pixel state, one batch's frame, the feature
  // sums, the filter's columns and hit flags, color_bytes' thresholds, and a host caller's outputs before they are copied
  DevBuf<double> vd_total, vd_mean, vd_m2, vd_stage, vd_feat, vd_cols, vd_thr, vd_linear, vd_out_mean, vd_out_var;
  DevBuf<uint32_t> vd_counts;
  DevBuf<uint8_t> vd_hit, vd_rgb8;
  DevBuf<double> aov_out;              // rptgpu_render_aov: the requested channels' full-frame arrays, back to back (api_aov.cpp)
  int num_cus = 0;
  bool prefer_wavefront = false; // scene has real kd-trees: traversal-latency bound
  bool all_flat = false;         // every tree is a single leaf (and the scene fits the LDS tables): the path kernel
                                 // without any traversal code
  FlatLayout flat_layout{};        // the flat kernel's dynamic LDS
  DevBuf<double> plane_vals;       // distinct bounding-plane coordinates of the untransformed meshes [3][4]
  uint32_t flat_lds_bytes = 0;
  bool ext_shapes = false;       // scene has a shape only the *_ext kernel builds implement
  // deep-tree scenes: per top-level object the route bytes (launch_limits.h; made by scene_plan.h) and the buffers of the
  // object-by-object query
  std::vector<uint8_t> obj_deep, obj_tris, light_casts;
  // every per-tree object of the scene is one only by the kd-trees-of-kd-trees rule (shallow group, mesh children): for
  // (fractal_teapots at 8 bounces, 3.8 M paths per pass: 60.7 against 56.9 Msamples/s; 7.7 M: 70.6 against 86.7)
  bool tree_kids = false;   // some object is a group with tree children, or a tree too deep for the in-kernel
                            // traversals: only the per-tree pipeline walks those
  uint32_t max_tree_depth = 0;
  uint32_t gen_levels = 0, gen_frames = 0; // rpt_tree_generic's column heights for this scene (host_scene.cpp)
  bool gen_all = false;     // some object sends EVERY ray through rpt_tree_generic (irregular tree, generic_only)
  DevBuf<double> gen_defer, gen_frame;
  DevBuf<uint32_t> gen_overflow;
  uint32_t gen_threads = 0;
  std::vector<rptdev::Light> host_lights; // (what launch decisions need of the lights)
  // what rptgpu_scene_set_objects / _lights recompute from (api_scene.cpp): host copies of what they change, and what
  // creation knew of each object's geometry
  std::vector<rptdev::Inst> top_insts;    // insts[0, num_objects + Light::Object shapes) as on the device
  std::vector<rptdev::Material> host_materials;
  std::vector<rpthost::ObjectGeom> obj_geom;
  // what rptgpu_scene_set_mesh rebuilds a tree from (api_mesh.cpp): host copies of the tree records and depths, which
  // trees a Light::Object's shape or a group's child uses (those are not updated), the arrays' element counts (a DevBuf's n
  // is its capacity), and the SECOND set of the geometry arrays: an update builds the whole new scene there — the other
  // trees' records copied device to device, packed as a fresh handle packs them — and the two sets swap at the end
  std::vector<rptdev::Tree> host_trees;
  std::vector<uint32_t> tree_depth;
  std::vector<uint8_t> tree_shared;
  std::vector<uint8_t> inst_sig;     // per record of insts[]: kind | has_xf << 7 — what rptgpu_scene_set_group holds a group's
                                     // children to (api_group.cpp; the children's records themselves live on the device only)
  uint64_t n_insts = 0, n_nodes = 0, n_refs = 0, n_tris = 0;
  DevBuf<rptdev::Inst> alt_insts;
  DevBuf<rptdev::Tree> alt_trees;
  DevBuf<rptdev::KdNode> alt_nodes;
  DevBuf<uint32_t> alt_refs;
  DevBuf<rptdev::Tri> alt_tris;
  DevBuf<rptdev::TriX> alt_trix;
  DevBuf<rptdev::LeafBox> alt_lbox;
  DevBuf<double> mesh_src;           // the host entry point's triangles, uploaded (rptgpu_scene_set_group: its RptTransform records)
  DevBuf<rptdev::TriX> mesh_trix;    // the updated mesh's records by triangle index
  DevBuf<rpthost::Box> mesh_boxes;   // ... and its triangles' boxes (rptgpu_scene_set_group: the children's)
  DevBuf<uint32_t> mesh_flag;        // [0] some triangle is a sliver
  std::vector<uint32_t> cnt_host;  // the per-depth counters read back from the device
  bool has_deep = false;
  DevBuf<uint32_t> tq, tq_ctr;
  StackSpill spill{};              // the per-tree traversal kernels' stack beyond the LDS levels (kernels.h)
  DevBuf<uint32_t> spill_node;
  DevBuf<double> spill_ts, spill_bmax;
  DevBuf<double> tree_rays;        // [cap][8]: rpt_tree_enter's rows for the traversal kernels' refill
  // optional ray sort in front of the per-tree traversal (RPTGPU_SORT_RAYS)
  bool sort_rays = false;          // some deep tree is large enough for sorting to pay (RPT_DEEP_SORTED in its obj_deep)
  RptSceneOptions opt{};           // the handle's knobs: defaults, the caller's RptSceneOptions, environment overrides — fixed at creation,
                                   // and the one copy of each: every reader reads it here
  QueryTuning qtune{0u, 1u << 19};  // launch_query's counter-set toggle; opt.sort_min_rays
  DevBuf<uint32_t> sort_kin, sort_kout, sort_vin;
  DevBuf<uint8_t> sort_tmp;
  SortBufs sort_bufs{};
  DevBuf<double> srt;
  DevBuf<uint32_t> shadow_q;
  // cached pixel partition
  uint32_t part_key[6] = {0, 0, 0, 0, 0, 0};
  uint32_t npix = 0;
  // accounting
  RptStats stats{};
  std::vector<hipEvent_t> ev_pool;
  struct Pending { int kind; int e0, e1; };
  std::vector<Pending> pending;
  int ev_used = 0;
  // multi-GPU: the communicator of this handle (rptgpu_comm_init) and its frame buffers
  RcclComm comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  DevBuf<float> frame32, frame32_sum;
  // multi-GPU gather: this rank's packed pixels; on the root the peers' packed pixels and every rank's pixel list
  DevBuf<float> packed32, gather32;
  DevBuf<uint32_t> gather_pixels;          // [world] lists back to back, in rank order
  std::vector<uint64_t> gather_off;        // [world + 1] offsets (pixels) into gather_pixels
  uint32_t gather_key[5] = {0, 0, 0, 0, 0}; // width, height, world, root, 1
  bool comm_failed = false;                // a batch's collective failed: sticky until comm_destroy + comm_init
  bool abandoned = false;                  // an aborted batch's work did not drain: kernels of it may still run on the old stream
                                           // and touch the workspace — nothing more is enqueued on this handle, ever
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};

  ~rptgpu_scene() {
    (void)hipSetDevice(device);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (comm && rccl().ok) (void)rccl().CommDestroy(comm);
    if (stream) (void)hipStreamDestroy(stream);
    // every DevBuf member frees itself (its destructor runs after this body, on `device`)
  }
};

namespace rptapi {

// the error convention: every entry point returns an int; the detail goes to the handle (or, without one, to the thread)
int fail(rptgpu_scene* h, int code, const std::string& detail);
int hip_fail(rptgpu_scene* h, const HipError& e);
// The frame of an entry point that uses the device: select it, run the body (-> the call's code), and map what the body
// throws to a code and a detail in this one place.  h may be null (the detail then goes to the thread).  Argument checks
// that need no device stand in front of it.
// hipGetLastError() reports the thread's LAST failed runtime call, whoever made it (another library in the process, an
// unchecked clean-up call): the body starts from a clean slate, so that its checks speak about this call's launches.
template <class Body> int guarded(rptgpu_scene* h, int device, Body&& body) {
  try {
    HIP_TRY(hipSetDevice(device));
    (void)hipGetLastError();
    return body();
  } catch (const HipError& e) {
    return hip_fail(h, e);
  } catch (const std::bad_alloc&) {
    return fail(h, RPTGPU_E_OUT_OF_MEMORY, "host allocation failed");
  } catch (...) {
    return fail(h, RPTGPU_E_HIP, "unexpected exception");
  }
}
// ext: the scene contains a shape of the extended set (RPT_SHAPE_MONOMIAL), which only the *_ext builds
// of the kernels know; everything else runs the base builds
const KernelTable* table_for(uint32_t mode, bool ext = false);
extern const char* const BAD_MODE;

// ---- the entry points that return named channels into the caller's arrays (channel_plan.h: one table per output struct,
// beside the struct's planner).  What every such call refuses in its query and its arrays, as string literals made from the
// struct's name and its channels' prefix: a null struct, a wrong struct_size, no channel, an unknown bit; reserved != 0, and
// the lowest named channel whose array is NULL.  A driver's own checks stand between and behind these, in its own order
struct QueryTexts { const char *null, *size, *none, *unknown; };
#define RPT_QUERY_TEXTS(Struct, PREFIX)                                                                                         \
  rptapi::QueryTexts { "null " #Struct, #Struct ": struct_size is not sizeof(" #Struct ")",                                     \
                       #Struct ": channels == 0 (name at least one " #PREFIX "_* channel)", #Struct ": channels names an unknown " #PREFIX "_* bit" }
template <class Q> const char* bad_query_struct(const Q* q, const QueryTexts& t) {
  return !q ? t.null : q->struct_size != sizeof(Q) ? t.size : nullptr;
}
template <class Q> const char* bad_query_channels(const Q& q, const QueryTexts& t, uint32_t all) {
  return !q.channels ? t.none : (q.channels & ~all) ? t.unknown : nullptr;
}
template <class Q> const char* bad_channel_query(const Q* q, const QueryTexts& t, uint32_t all) {
  const char* why = bad_query_struct(q, t);
  return why ? why : bad_query_channels(*q, t, all);
}
struct ArraysTexts { const char *null, *size, *reserved; };
#define RPT_ARRAYS_TEXTS(Struct) \
  rptapi::ArraysTexts { "null " #Struct, #Struct ": struct_size is not sizeof(" #Struct ")", #Struct ": reserved != 0" }
template <class A> const char* bad_channel_arrays(const A* o, const ArraysTexts& t, rptchan::Table rows, uint32_t channels) {
  if (!o) return t.null;
  if (o->struct_size != sizeof(A)) return t.size;
  if (o->reserved) return t.reserved;
  const rptchan::Row* r = rptchan::first_null(rows, channels, o);
  return r ? r->null_text : nullptr;
}
// a table's arrays by row (nullptr: not there): the caller's, from `base` items on — only the named channels' members are
// read —; those of layout l inside an allocation of the handle; and the copy of `channels` from the device to the host, c
// items each, in ascending bit order (api_common.cpp)
struct ChannelPtrs {
  char* p[rptchan::MAX_ROWS];
  template <class T> T* at(int k) const { return (T*)p[k]; }
};
ChannelPtrs ptrs_at(rptchan::Table t, const void* arrays, uint32_t channels, const rptchan::Counts& base);
ChannelPtrs ptrs_in(double* base, const rptchan::Layout& l);
void copy_out(rptchan::Table t, const ChannelPtrs& src, const ChannelPtrs& dst, uint32_t channels, const rptchan::Counts& c, hipStream_t st);
// a piece of a host caller's m rays (or points and their directions) into the handle's rays_o / rays_d -> where it lies
void stage_rays(rptgpu_scene* h, const double*& a, const double*& b, uint32_t m);

// api_render.cpp
// StackSpill::zeros_common of a scene with these lights (scheduling: which kernel takes rays with a zero component)
uint32_t zeros_common(const std::vector<rptdev::Light>& lights);
void ensure_partition(rptgpu_scene* h, const RptRenderParams& p);
std::vector<uint32_t> pixel_list(uint32_t width, uint32_t height, uint32_t tw, uint32_t th, uint32_t pi, uint32_t pc);
const char* bad_params(const RptRenderParams* p);
// the workspace and its views, shared with rptgpu_render_aov's pass loop (api_aov.cpp)
void ensure_workspace(rptgpu_scene* h, uint64_t cap, uint64_t rec_cols);
void release_workspace(rptgpu_scene* h);
void ensure_generic(rptgpu_scene* h, bool all);
rptdev::PathState path_state(rptgpu_scene* h);
rptdev::Camera make_camera(const RptCamera& c);
int64_t free_memory();
// the route of a call: a group with tree children is only walked by the per-tree kernels of the wavefront pipeline
// (RPT_FLAG_PERSISTENT is a request such a scene cannot honour, not an error); without a flag, `fallback`
inline bool use_wavefront(const rptgpu_scene* h, uint32_t flags, bool fallback) {
  return (flags & RPT_FLAG_WAVEFRONT) || h->tree_kids ? true : (flags & RPT_FLAG_PERSISTENT) ? false : fallback;
}
// the next pass of `in` (everything filled) with its workspace made: rptplan::plan_pass, shrunk while the device is out
// of memory (a pass of one sample per pixel that does not fit rethrows, as does every other error)
rptplan::PassPlan size_pass(rptgpu_scene* h, const rptplan::PassInput& in, uint32_t npix, bool generic_all);
// The per-tree pipeline's queries over the workspace (KernelTable::query with what every call takes from the handle):
// the closest hits of the n rays of `ps`; the visibility of light l's shadow queue (n rays; d_n: its length on the
// device).  reset_tree_counters: both sets of a tree's counters cleared, before the first query of a pass.
void reset_tree_counters(rptgpu_scene* h);
void query_closest(rptgpu_scene* h, const KernelTable* kt, const rptdev::PathState& ps, uint32_t n, const QueryHook* hook);
void query_visibility(rptgpu_scene* h, const KernelTable* kt, const rptdev::PathState& ps, int l, uint32_t n,
                      const uint32_t* d_n, const QueryHook* hook);
// profiling: a launch of `kind` is counted and, when `on` and the pool has room (MAX_EVENT_PAIRS), bracketed with two
// events of the handle's pool.  begin -> the pair (-1: none); drain_events resolves the pairs once the stream is idle
int event_pair_begin(rptgpu_scene* h, int kind, bool on);
void event_pair_end(rptgpu_scene* h, int kind, int pair);
// The end of a call that ran the wavefront kernels: its last synchronisation.  rpt_tree_generic raises a flag when a
// traversal outgrows its columns (they are sized from the scene, so that is a bug, not an input): with read_overflow the
// flag rides with the synchronisation and is cleared, so that the flag of one call never surfaces in the next.
int drain_call(rptgpu_scene* h, bool read_overflow);
// The frame of an entry point that runs kernels on the handle's stream, behind its argument checks (h is not null): guarded
// around the call's clock, the wait for the caller's stream (user_stream: the one the call's device inputs were
// produced on; nullptr: none, or the body waits itself, where it has to do something first), the body, drain_call.  The
// body enqueues the call's work and returns drain_call's read_overflow — whether this call ran rpt_tree_generic.  A call that
// fails leaves RptStats::total_ms as it was.
template <class Body> int device_call(rptgpu_scene* h, hipStream_t user_stream, Body&& body) {
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = guarded(h, h->device, [&]() -> int {
    // a call leaves no event pair behind, however it ends (one that ends well has resolved them: drain_call)
    struct EventPairs {
      rptgpu_scene* h;
      ~EventPairs() { h->pending.clear(); h->ev_used = 0; }
    } event_pairs{h};
    if (user_stream) HIP_TRY(hipStreamSynchronize(user_stream));
    const bool read_overflow = body();
    return drain_call(h, read_overflow);
  });
  if (rc != RPTGPU_OK) return rc;
  h->stats.total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return RPTGPU_OK;
}
// Where the paths of a driver's batch start: a camera's pixels, or a piece of one of three kinds, told apart by which
// pointers are set.  Both drivers read it; each line names the fields its form reads, and every other field keeps its default.
//   a camera (render_impl)       cam.  Wavefront: rpt_raygen.  Persistent: rpt_paths.
//   the caller's rays (api_rays.cpp)  origins, dirs ([fr.npix][3] f64 on the device), first_draw (where every stream continues).
//                                Wavefront: rpt_raygen_rays, which also writes the piece's stream ids id_base + i to ids_out
//                                (nullptr: the caller named them, and they lie in Frame::pixels).  Persistent: rpt_paths_rays;
//                                Frame::pixels holds the ids already (the caller's, or rpt_rays_ids'), ids_out and id_base are
//                                not read.
//   ... with vertices (api_vertices.cpp)  the same, and vertices: where the vertices of the piece's paths go — the caller's arrays
//                                or their staging, offset to the piece; s_first is filled in per pass or launch.
//                                Wavefront: rpt_vertices_store and rpt_vertices_fold beside the ray call's kernels.
//                                Persistent: rpt_paths_vertices, which writes them itself.
//   light probes (api_probes.cpp)  probe (the RPT_PROBE_* kind), origins = the positions, dirs = the normals (nullptr for
//                                RPT_PROBE_SH9), probe_scale (4 pi / S or pi / S), ids_out and id_base as for rays.
//                                Wavefront: rpt_raygen_probes, rpt_resolve_probes into sums of probe_width(kind) words per
//                                probe, rpt_finish_probes.  Persistent: rpt_paths_rays, rpt_project_probes, rpt_finish_probes.
//   a batch of views (api_views.cpp)  views (the call's records on the device), view_width, view_height, view_base: the piece
//                                is the fr.npix consecutive indices from view_base on, index j = view * (view_width *
//                                view_height) + pixel.  view_seeds (nullptr: every view's seed is the Frame's): the call's
//                                seeds on the device, one per view; Frame::seed is not read then.
//                                Wavefront: rpt_raygen_views writes the pixels to ids_out; with view_seeds
//                                rpt_raygen_views_seeded also writes each index's seed to seeds_out, where rpt_shade_seeded
//                                reads it.  Persistent: rpt_paths_views; view_seeds always, view_of the view of each index
//                                counted from the piece's first (rpt_views_ids wrote it, and the pixels into Frame::pixels).
struct RaySource {
  const rptdev::Camera* cam;
  const double *origins, *dirs;
  uint32_t first_draw, id_base;
  uint32_t* ids_out;
  int probe = -1;           // < 0: not probes
  double probe_scale = 0.0;
  const rptdev::View* views = nullptr;
  uint32_t view_width = 0, view_height = 0;
  uint64_t view_base = 0;
  const uint64_t* view_seeds = nullptr;
  uint64_t* seeds_out = nullptr;
  const uint32_t* view_of = nullptr;
  const rptdev::VertexOut* vertices = nullptr;
};
// api_views.cpp: what is wrong with an RptViewQuery / with one view of a call with query q (nullptr: nothing); shared with
// rptgpu_render_views_aov (api_hits.cpp)
// views_persistent_ok: the call takes RPT_FLAG_VIEWS_PERSISTENT (rptgpu_render_views and its forms); the others refuse it by name
const char* bad_view_query(const RptViewQuery* q, bool views_persistent_ok = false);
const char* bad_view(const RptView& v, const RptViewQuery& q);
// the seeds of a call's views as the drivers take them: the caller's (the _seeded entry points), or seed + v * seed_stride in
// wrapping u64 arithmetic; empty: every view has the query's seed (seed_stride == 0), the one-seed route
constexpr const char* NULL_SEEDS = "null seeds: the _seeded entry points take one seed per view";
std::vector<uint64_t> view_seed_list(uint64_t n_views, const RptViewQuery& q, const uint64_t* seeds);
// the drivers behind rptgpu_render_views[_seeded][_device] (api_views.cpp) and rptgpu_render_views_aov[_seeded][_device]
// (api_hits.cpp), argument checks included; rptgpu_render_views_denoised (api_views_denoise.cpp) runs both into device arrays
// of its own.  out / out's arrays: host memory, or — on_device — device memory; seeded: view v's seed is seeds[v] (host)
int render_views(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q, bool seeded, const uint64_t* seeds,
                 void* out, bool on_device, bool out_f32, hipStream_t user_stream);
int render_views_aov(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q, bool seeded,
                     const uint64_t* seeds, const RptAovBuffers* out, bool on_device, hipStream_t user_stream);
// api_hits.cpp: rptgpu_first_hits' query, piece by piece, as rptgpu_hit_surface runs it too (api_surface.cpp).  plan_hit_pieces:
// the call's route (flags: its RPT_FLAG_GENERAL_TRAVERSAL into the scene record), the rays per piece (piece_env: the
// environment variable that overrides it, read per call) and, for the per-tree query, the workspace and its path state.
// hit_piece: the query over m rays at d_o / d_d on the device and the channels of `ho` — rpt_first_hits, or rpt_raygen_rays,
// the per-tree query and rpt_hits_store; one RPT_K_EXTEND launch is counted (timed when prof)
struct HitPieces {
  bool by_object;
  uint64_t piece;
  rptdev::PathState ps;
};
HitPieces plan_hit_pieces(rptgpu_scene* h, uint64_t n, uint32_t flags, const char* piece_env);
void hit_piece(rptgpu_scene* h, const KernelTable* kt, const HitPieces& hp, const double* d_o, const double* d_d, uint32_t m,
               const rptdev::HitOut& ho, bool prof);
// api_surface.cpp: rptgpu_hit_surface's resolve walk, piece by piece, as rptgpu_lookup_lightmap runs it too
// (api_lightmap_lookup.cpp).  ensure_surface_columns: rpt_hit_surface's columns for pieces of `piece` rays (and the overflow
// flag); group_holds_monomial: the walk's groups_from_inf; surface_walk_piece: the walk over m rays at d_o / d_d whose T and
// OBJECT stand in `so`, into so's named channels
GenericStack ensure_surface_columns(rptgpu_scene* h, uint64_t piece);
bool group_holds_monomial(const rptgpu_scene* h);
void surface_walk_piece(rptgpu_scene* h, const double* d_o, const double* d_d, uint32_t m, const rptdev::SurfaceOut& so,
                        const GenericStack& gs, bool from_inf);
// api_lightmap_lookup.cpp: what rptgpu_render_views_probe_lit (api_probe_volume.cpp) shares with
// rptgpu_render_views_lightmapped.  bad_bindings / bad_bindings_for: what is wrong with the bindings by themselves / against
// the handle's scene (empty: nothing); stage_bindings: a host caller's bindings' arrays inside one allocation -> the words, or
// ~0 when no allocation holds them (BINDINGS_TOO_LARGE); upload_bindings: the call's binding records and object-to-binding
// table on the device, into `rays` (table and recs are the caller's: the uploads read them until the call's last
// synchronisation)
std::string bad_bindings(uint32_t n_bindings, const RptLightmapBinding* b);
std::string bad_bindings_for(const rptgpu_scene* h, uint32_t n_bindings, const RptLightmapBinding* b);
uint64_t stage_bindings(uint32_t n_bindings, const RptLightmapBinding* bindings, bool on_device, std::vector<rptlookup::Staged>& staged);
constexpr const char* BINDINGS_TOO_LARGE = "the bindings' maps do not fit: no allocation holds them";
void upload_bindings(rptgpu_scene* h, uint32_t n_bindings, const RptLightmapBinding* bindings, bool on_device,
                     const std::vector<rptlookup::Staged>& staged, uint64_t stage_words, std::vector<int32_t>& table,
                     std::vector<rptlookup::Binding>& recs, rptlookup::Rays& rays);
// ... and the driver the two calls share (api_lightmap_lookup.cpp): rptgpu_render_views' refusals of qv, then bad_own_query — what
// is wrong with the call's own query (nullptr: nothing) —, then out, the views, the bindings, the handle; `lit` is read only
// when bad_own_query is nullptr.  volume == nullptr: rptgpu_render_views_lightmapped
struct ViewsLit {
  uint32_t filter;                // RPT_LOOKUP_NEAREST / _BILINEAR
  const double* unbound;          // [3] I of a hit nothing covers
  const RptProbeVolume* volume;   // checked by the caller (api_probe_volume.cpp bad_volume), or nullptr
  double normal_bias;             // the volume rule's
};
int render_views_lit(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* qv, uint32_t n_bindings,
                     const RptLightmapBinding* bindings, const char* bad_own_query, const ViewsLit& lit, double* out, bool on_device,
                     hipStream_t user_stream);
// api_probe_volume.cpp: the volume as the kernels read it — a device caller's arrays as they are, a host caller's staged
// whole on the handle's stream —, and RPTGPU_VOLUME_PIECE's value (0: not set)
rptvolume::Volume upload_volume(rptgpu_scene* h, const RptProbeVolume& v, double normal_bias, bool on_device);
uint64_t asked_volume_piece();
// f64 words of a probe's result and of its running sums: [9][3] SH coefficients, or an RGB irradiance
inline uint32_t probe_width(uint32_t kind) { return kind == RPT_PROBE_SH9 ? 27u : 3u; }
const char* bad_probe_query(const RptProbeQuery* q);
// the device work of rptgpu_bake_probes (api_probes.cpp) and rptgpu_bake_ao (api_occlusion.cpp) behind their checks, n > 0:
// the bodies of their device_calls -> drain_call's read_overflow.  rptgpu_bake_lightmap runs both inside its own device_call
// over its compacted texels (on_device, with stream ids and outputs given: they then stage nothing)
bool enqueue_probes(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                    const RptProbeQuery* q, double* out, bool on_device);
bool enqueue_ao(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                const RptAoQuery* q, double* out_ao, double* out_bent, bool on_device);
// the pass planner's input for a call over npix pixels or rays: what its passes share, and the device's state right now
rptplan::PassInput pass_input(rptgpu_scene* h, uint32_t npix, uint32_t iterations);
void pass_input_now(rptgpu_scene* h, rptplan::PassInput& in);
// rptgpu_bake_direct's device work in the same way (api_direct.cpp): its device_call's body, which
// rptgpu_bake_lightmap_direct runs over its compacted texels
bool enqueue_direct(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                    const RptDirectQuery* q, double* out, bool on_device);
// the lightmap pipeline (api_lightmap.cpp) with enqueue_direct as its one gather, into `direct` ([H][W][3]): the driver
// behind rptgpu_bake_lightmap_direct[_device] (api_direct.cpp), argument checks included
int bake_lightmap_direct(rptgpu_scene* h, uint64_t n_tris, const double* positions, const double* normals, const double* uvs,
                         const RptLightmapQuery* q, double* direct, bool on_device, hipStream_t user_stream);

// what the drivers of rptgpu_occluded, rptgpu_bake_ao (api_occlusion.cpp) and rptgpu_bake_direct (api_direct.cpp) share: the
// route, the pass bound, the workspace, and the query itself
struct Occlusion {
  rptgpu_scene* h;
  const KernelTable* kt;
  bool prof, by_object;
  uint64_t pass_target; // rays a pass may hold
  uint64_t asked;       // piece_env's value (0: not set)

  Occlusion(rptgpu_scene* h_, uint32_t precision_mode, uint32_t flags, const char* piece_env)
      : h(h_), kt(table_for(precision_mode, h_->ext_shapes)), prof((flags & RPT_FLAG_PROFILE_KERNELS) != 0) {
    h->dscene.force_general = (flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
    // (run_pass's decision: per-tree queries for scenes with deep trees — under RPT_FLAG_GENERAL_TRAVERSAL only where a
    // group with tree children leaves no other walker)
    by_object = h->has_deep && (!(flags & RPT_FLAG_GENERAL_TRAVERSAL) || h->tree_kids);
    rptplan::PassInput in = pass_input(h, 1, 1);
    in.remaining = 1;
    in.ratio = 1.0; // no depth follows the rays: one record column is all ensure_workspace is asked for
    pass_input_now(h, in);
    pass_target = rptplan::plan_pass(in).target;
    asked = 0;
    if (const char* e = std::getenv(piece_env)) asked = std::strtoull(e, nullptr, 10);
  }
  // slots for `cap` rays.  ensure_workspace sizes the shadow state, the queues and srt for max(1, lights) columns, so a
  // scene without lights has the column 0 the visibility calls use
  rptdev::PathState workspace(uint64_t cap) {
    ensure_workspace(h, cap, 1);
    if (h->has_deep && (h->gen_all || h->dscene.force_general)) ensure_generic(h, true); // (as render_wavefront's size_pass)
    return path_state(h);
  }
  uint32_t* queue_length() const { return h->counters.p + 2; } // where rpt_shade counts light 0's shadow rays
  // the visibility of the n rays laid into light 0's shadow state: srt's column 0
  void query(const rptdev::PathState& ps, uint32_t n) {
    const int pair = event_pair_begin(h, RPT_K_SHADOW, prof);
    if (by_object) {
      reset_tree_counters(h);
      query_visibility(h, kt, ps, 0, n, queue_length(), nullptr);
    } else {
      kt->shadow_rays(h->stream, h->dscene, ps, h->shadow_q.p, queue_length(), n, 1, h->srt.p);
    }
    event_pair_end(h, RPT_K_SHADOW, pair);
    h->stats.shadow_rays += n;
    h->stats.shadow_rays_traced += n;
  }
  // the visibility of every light's queued rays, as a depth of run_pass asks for it: cnt[l] rays stand in light l's queue
  // (queue_length() + l on the device); srt's column l receives the queued slots' answers.  -> the rays traced
  uint64_t query_lights(const rptdev::PathState& ps, const uint32_t* cnt) {
    const int nlights = h->dscene.num_lights;
    uint64_t traced = 0;
    uint32_t n_max = 0;
    for (int l = 0; l < nlights; l++) {
      traced += cnt[l];
      n_max = std::max(n_max, cnt[l]);
    }
    if (!n_max) return 0;
    const int pair = event_pair_begin(h, RPT_K_SHADOW, prof);
    if (by_object) {
      reset_tree_counters(h);
      for (int l = 0; l < nlights; l++)
        if (cnt[l]) query_visibility(h, kt, ps, l, cnt[l], queue_length() + l, nullptr);
    } else { // one launch for all lights (the grid's y is the light; an empty queue costs its blocks one load)
      kt->shadow_rays(h->stream, h->dscene, ps, h->shadow_q.p, queue_length(), n_max, nlights, h->srt.p);
    }
    event_pair_end(h, RPT_K_SHADOW, pair);
    return traced;
  }
};

// ---- what the calls that run a path driver over PIECES share (api_rays.cpp, api_probes.cpp, api_vertices.cpp, api_views.cpp):
// a piece of rays, probes or (view, pixel) indices is the "frame" of its own passes or launches
// the RptRenderParams of such a call, from its query q: what render_wavefront reads of it, and render_persistent
template <class Query> RptRenderParams piece_params(const Query& q, uint32_t iterations, double exposure_value) {
  RptRenderParams p{};
  p.max_bounces = q.max_bounces; p.iterations = iterations; p.exposure_value = exposure_value;
  p.seed = q.seed; p.sample_index_base = q.sample_index_base; p.precision_mode = q.precision_mode; p.flags = q.flags;
  return p;
}
// the paths one pass may hold with every level of every path: what bounds a piece (rptplan::rays_piece and its kin take it)
inline uint64_t piece_pass_target(rptgpu_scene* h, uint32_t iterations, uint32_t max_bounces) {
  rptplan::PassInput in = pass_input(h, 1, iterations);
  in.remaining = iterations;
  in.ratio = (double)max_bounces + 1.0;
  pass_input_now(h, in);
  return rptplan::plan_pass(in).target;
}
// the persistent kernel on request (`flag`: the call's RPT_FLAG_*_PERSISTENT) — unless the scene has a group with tree
// children, which only the wavefront pipeline walks (use_wavefront: such a scene cannot honour the request, as for a render)
inline bool piece_persistent(const rptgpu_scene* h, uint32_t flags, uint32_t flag) {
  return (flags & flag) && !use_wavefront(h, 0, false);
}
// ... whose pieces are also at most what a launch's 32-bit work counter holds, at the most resident blocks any
// instantiation has: `piece` (the planner's), capped
inline uint64_t persistent_piece(const rptgpu_scene* h, uint64_t piece, uint32_t iterations) {
  return rptplan::rays_persistent_piece(piece, iterations, (uint32_t)std::max(1, h->num_cus) * RPT_PATHS_WAVES_PER_CU_MAX, RPT_PATHS_BATCH_MAX);
}
// the Frame of a piece of m items whose stream ids lie (or will lie) at `pixels`
inline rptdev::Frame piece_frame(rptgpu_scene* h, const RptRenderParams& p, const uint32_t* pixels, uint64_t m) {
  rptdev::Frame fr{};
  fr.width = (uint32_t)m; fr.height = 1; fr.npix = (uint32_t)m; fr.pixels = pixels;
  fr.max_bounces = p.max_bounces; fr.seed = p.seed; fr.accum = h->accum.p;
  return fr;
}
// the wavefront driver: the batch in passes from `src`, then rpt_finish into `out` (api_render.cpp)
void render_wavefront(rptgpu_scene* h, const KernelTable* kt, const RptRenderParams& p, rptdev::Frame fr, const RaySource& src,
                      void* out, bool out_f32, bool packed, bool prof);
// the persistent driver: the batch in launches of the form of the persistent kernel src asks for (KernelTable::paths),
// rpt_sum_samples behind each, then rpt_finish into `out` — probes: rpt_project_probes and rpt_finish_probes in their places
// (api_render.cpp)
void render_persistent(rptgpu_scene* h, const KernelTable* kt, const RptRenderParams& p, rptdev::Frame fr, const RaySource& src,
                       void* out, bool out_f32, bool packed, bool prof);
// a piece through the driver of its call's route, the results packed into `out` in the order of the piece's items
inline void render_piece(rptgpu_scene* h, const KernelTable* kt, const RptRenderParams& p, const rptdev::Frame& fr, const RaySource& src,
                         void* out, bool out_f32, bool persistent) {
  const bool prof = (p.flags & RPT_FLAG_PROFILE_KERNELS) != 0;
  if (persistent) render_persistent(h, kt, p, fr, src, out, out_f32, true, prof);
  else render_wavefront(h, kt, p, fr, src, out, out_f32, true, prof);
  HIP_TRY(hipGetLastError());
}
// A call over n rays or probes of the caller, and the loop that runs it in pieces (api_rays.cpp; rptgpu_trace_rays,
// rptgpu_bake_probes, rptgpu_trace_vertices and their _device forms).  on_device: a, b, streams and out are device pointers,
// read and written where they lie; else a piece at a time is staged in arrays the handle keeps.
struct RayPieces {
  uint64_t n;
  const double *a, *b;     // [n][3] each: origins and directions, or positions and normals; b may be null (it is not read then)
  const uint32_t* streams; // [n] stream ids; nullptr: item i has id i
  bool on_device;
  uint64_t piece;          // items per piece
  bool persistent;         // the route (piece_persistent); the piece is then persistent_piece's
  RptRenderParams p;       // piece_params
  uint32_t first_draw;
  uint32_t width;          // f64 words of an item's result: 3, or probe_width(kind)
  double* out;             // [n][width]; nullptr: the call does not return them (they stay in the handle's array)
  int probe = -1;          // light probes: the RPT_PROBE_* kind and its RaySource::probe_scale
  double probe_scale = 0.0;
};
// before(base, m, src): the piece's RaySource is complete but for what the call adds, its inputs are on the device;
// after(base, m): the piece's work is enqueued, a host caller's results are not yet copied out.  Either may be empty.
void trace_ray_pieces(rptgpu_scene* h, const RayPieces& c, const std::function<void(uint64_t, uint64_t, RaySource&)>& before,
                      const std::function<void(uint64_t, uint64_t)>& after);
// packed (with d_out, f32 or f64): d_out receives only this part's pixels, [npix][3] in the order of the part's pixel list.
// d_list (device, n_list pixel indices; requires packed and d_out): render exactly those pixels instead of the part's list,
// without touching the cached partition (the adaptive buffer's active pixels, api_buffer.cpp)
int render_impl(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* p, void* d_out, bool out_f32,
                double* host_out, hipStream_t user_stream, bool packed = false, const uint32_t* d_list = nullptr,
                uint32_t n_list = 0);

// api_aov.cpp: the checks and the device half of rptgpu_render_aov, shared with rptgpu_buffer_features (api_buffer.cpp)
const char* bad_aov(const RptAovBuffers* o);
const char* bad_aov_params(const RptRenderParams* p);
// the arrays of `channels` for n pixels inside `arrays` (grown when too small), zeroed on st (object: -1)
rptdev::AovOut aov_arrays(DevBuf<double>& arrays, hipStream_t st, uint64_t n, uint32_t channels);
// the call's route and kernels into `ao` (after ensure_partition); -> drain_call's read_overflow
bool aov_enqueue(rptgpu_scene* h, const RptCamera& camera, const RptRenderParams& p, const rptdev::AovOut& ao);
// the kernels' struct from the arrays of rptplan::AOV_ROWS; hits and the arrays of `channels` for n pixels from the device
// to the caller's (ptrs_at of its RptAovBuffers), on st
rptdev::AovOut aov_out(const ChannelPtrs& p, uint32_t channels);
void copy_aov_out(const rptdev::AovOut& src, uint32_t channels, const ChannelPtrs& dst, uint64_t n, hipStream_t st);

// api_buffer.cpp: what the Buffer's filter shares with the views' (api_views_denoise.cpp) — what is wrong with an RptDenoise
// (nullptr: nothing), the features the filter reads, and color_bytes' staircase for the device (thr[k]: the smallest v in
// [0, 1] whose byte is >= k; clean: the host's conversion is a step function around every threshold)
const char* bad_denoise(const RptDenoise* d);
constexpr uint32_t FEATURE_CHANNELS = RPT_AOV_DEPTH | RPT_AOV_NORMAL | RPT_AOV_ALBEDO | RPT_AOV_POSITION;
std::vector<double> byte_thresholds(bool& clean);

// A handle whose aborted batch never drained (rptgpu_render_batch_reduce, drain_after_abort): the abandoned stream's
// kernels may still read and write the workspace, the frame buffers and events, so every call that would enqueue work
// refuses — until rptgpu_scene_destroy.
#define REFUSE_IF_ABANDONED(h)                                                                                            \
  do {                                                                                                                    \
    if ((h) && (h)->abandoned)                                                                                            \
      return fail((h), RPTGPU_E_COMM, "an aborted batch's device work never drained on this handle: destroy it (its "    \
                                      "workspace may still be written by the abandoned stream)");                        \
  } while (0)
// the live updates' refusal of such a handle (api_scene.cpp update_refusal, tree_splice.h rebuild_target)
constexpr const char* ABANDONED_TAKES_NO_UPDATE =
    "an aborted batch's device work never drained on this handle: it takes no update (destroy it)";

} // namespace rptapi
