// kernels.h — host-callable launchers of the gfx950 kernels, one table per arithmetic mode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "hit_pool.h"
#include "launch_limits.h"
#include "flat_layout.h"

// RPT_SHADE_SPLIT=1: in rpt_paths<KdFlat, false, true>, a wave whose light is an untransformed mesh and whose hits are
// opaque takes every draw of its hits first and then shades them in one straight-line block (kernels/paths_shade.inc
// hit_draws); 0: the sequence of illuminate, bsdf, sample_f and bsdf (A/B builds)
#ifndef RPT_SHADE_SPLIT
#define RPT_SHADE_SPLIT 1
#endif
// RPT_DIV_BATCH=1: neighbouring independent f64 divisions are issued as one batch, stage by stage (kernels/vec.inc
// div_ieee): every quotient keeps the eleven operations of the compiler's own expansion of `/` on the same operands,
// only their order across the batch's slots changes, so every result keeps its bits.  0: every call site compiles to
// the plain `/` it was (A/B builds)
#ifndef RPT_DIV_BATCH
#define RPT_DIV_BATCH 1
#endif
// RPT_DRAW_PLAN=1: hit_draws (kernels/paths_shade.inc) takes a hit's single draws — the light triangle's index, gen_bool(f),
// u_theta — out of Philox blocks that every lane computes together with the pair next to them (kernels/rng.inc
// philox_block2, draw_window): the stream is random-access, so only WHEN a block is computed changes, never which draw feeds
// which value.  0: one next_u64 per single draw, a block at the lanes whose draw counter is even (A/B builds)
#ifndef RPT_DRAW_PLAN
#define RPT_DRAW_PLAN 1
#endif
// flat scenes with a texture environment: the lanes' queues of parked lookups, RPT_PARK_K entries each, at the end of the
// wave's dynamic LDS (kernels/paths.inc ParkLds)
#ifndef RPT_PARK_K
#define RPT_PARK_K 4
#endif
#define RPT_PATHS_PARK_LDS (RPT_PARK_K * 2624u)
// the paths of a depth are re-ordered by ray key in scenes without per-tree queues when there are at least this many
#ifndef RPT_PATH_REORDER_MIN
#define RPT_PATH_REORDER_MIN (1u << 20)
#endif

// RPT_VERTICES_FILL_IN_KERNEL=1: rpt_vertices_fold also writes the filler behind a path's last vertex, entry by entry, and the
// host lays none down (A/B builds: the first form of rptgpu_trace_vertices, DESIGN.md §19 has its numbers); 0: the host fills a
// piece's arrays with streaming fills before its first pass (api_vertices.cpp)
#ifndef RPT_VERTICES_FILL_IN_KERNEL
#define RPT_VERTICES_FILL_IN_KERNEL 0
#endif

// the adaptive buffer's retire-and-compact kernels (kernels/buffer.inc): active-list entries per thread and per 256-thread
// block (the host sizes the per-block counts with it)
#define RPT_RETIRE_ITEMS 16u
#define RPT_RETIRE_TILE (RPT_RETIRE_ITEMS * 256u)

// buffers of the optional ray sort in front of a per-tree traversal (all sized for the query's n)
struct SortBufs {
  uint32_t *keys_in, *keys_out, *vals_in;
  void* tmp;
  size_t tmp_bytes;
};

// waves per SIMD of the per-tree traversal kernels and the stack levels they keep in LDS
// (RPT_TT_WAVES * 4 * 64 lanes * 20 B * levels <= 160 KB per CU); deeper levels go to the spill area
#ifndef RPT_TT_WAVES
#define RPT_TT_WAVES 4
#endif
#ifndef RPT_TT_LEVELS
#define RPT_TT_LEVELS 7
#endif
#define RPT_TT_LEVELS_MIN RPT_TT_LEVELS
// spill area of the traversal stack beyond the LDS levels: [KD_MAX_STACK - RPT_TT_LEVELS_MIN][threads] per array, one
// column per thread of the traversal grid (api_render.cpp allocates it for scenes with deep trees)
// rpt_tree_generic's pending work (kernels/tree_generic.inc), one column per thread of ITS grid: deferred far children
// (six face parameters, t_split, node) and the suspended leaves of the groups above the tree being walked
struct GenericStack {
  double* defer;  // [levels][8][threads]
  double* frame;  // [frames][12][threads]
  uint32_t threads, levels, frames;
};
struct StackSpill {
  uint32_t* node;
  double* ts;
  double* bmax;
  uint32_t threads;
  uint32_t zeros_common; // scene hint for launch_query: rays with a zero direction component are frequent (full grid for their kernel)
  // [position in the query][8]: object-space origin and direction, record.time and stop distance of a ray that enters
  // the tree — written by rpt_tree_enter, which has them in registers, as ONE 64-byte row; the traversal kernels' refill
  // reads that row (and the slot from the query's queue) instead of gathering eight values from the path state's SoA
  // arrays.  The tree's queues hold positions, not slots.
  double* rays;
  // rpt_tree_generic: its columns, the flag it raises if a scene outgrows them (api_render.cpp sizes them from the scene and
  // checks the flag when the batch is done), and its grid when it takes a few handed-on rays / every ray of an object
  GenericStack gen;
  uint32_t* gen_overflow;
  uint32_t gen_blocks_few, gen_blocks_all;
};

// accounting hook of launch_query: called with (ctx, kind, 0) before and (ctx, kind, 1) after the launches of
// a phase of the query (kind = RPT_K_TREE_TRACE / RPT_K_TREE_SORT); may be null
struct QueryHook {
  void (*mark)(void* ctx, int kind, int end);
  void* ctx;
};

// launch_query's state and tuning, owned by the caller (one per handle): which of the two sets of tree counters the
// next (tree, query) pair uses — both sets cleared when the buffer is made and after a failed render — and the
// smallest query that is still sorted (RptSceneOptions::sort_min_rays)
struct QueryTuning {
  uint32_t ctr_set;
  uint32_t sort_min_rays;
};

// the forms of the persistent kernel's loop (kernels/paths_loop.inc, RPT_PATHS_FORM): where a work item's ray comes from.  The
// device pass reads them in the kernels' text; the host indexes KernelTable::paths with them
#define RPT_PATHS_FORM_CAMERA 0 // rpt_paths: a camera's pixels
#define RPT_PATHS_FORM_VIEWS 1  // rpt_paths_views: a piece of a batch of views (paths_views.inc)
#define RPT_PATHS_FORM_RAYS 2   // rpt_paths_rays: a piece of the caller's rays or light probes (paths_rays.inc)
#define RPT_PATHS_FORM_VERTICES 3 // rpt_paths_vertices: a piece of the caller's rays, the paths' vertices exported (paths_vertices.inc)
#define RPT_PATHS_FORM_COUNT 4
// a launch's rays: every form reads its own members and no other — CAMERA cam, VIEWS views, RAYS rays, VERTICES rays and
// vertices (the piece's sink with the launch's s_first)
struct PathsRays {
  const rptdev::Camera* cam;
  const rptdev::ViewRays* views;
  const rptdev::CallerRays* rays;
  const rptdev::VertexOut* vertices;
};
// ... and what a launch of any form takes besides (lds_bytes: the flat scene's tables; park: RPT_PATHS_PARK_LDS more behind
// them for parked environment lookups)
struct PathsLaunch {
  uint32_t* work_counter;
  double* rec;
  unsigned long long* ray_counters;
  double* lbuf;
  uint32_t spp, chunk, n_items, nblocks;
  const FlatLayout* lay;
  bool flat;
  uint32_t lds_bytes;
  bool park;
  uint32_t batch; // work items a wave claims at a time; 0 = by the launch's size
};
// one form of the persistent kernel, compiled in a translation unit of its own (CAMERA: with everything else):
// max_blocks_per_cu — resident 64-thread blocks per CU — and launch for the SAME instantiation of that form's kernel
struct PathsForm {
  int (*max_blocks_per_cu)(const FlatLayout* flat /* null: not a flat scene */, uint32_t lds_bytes, bool park);
  void (*launch)(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const PathsRays&, const PathsLaunch&);
};

struct KernelTable {
  void (*raygen)(hipStream_t, const rptdev::Frame&, const rptdev::Camera&, const rptdev::PathState&, uint32_t n_paths);
  // rpt_raygen's step for a piece of the caller's rays (rptgpu_trace_rays): fr.npix rays at origins / dirs ([npix][3] f64 on
  // the device), every stream continuing at first_draw; ids_out (may be null): receives the piece's stream ids id_base + i
  void (*raygen_rays)(hipStream_t, const rptdev::Frame&, const double* origins, const double* dirs, uint32_t first_draw,
                      uint32_t* ids_out, uint32_t id_base, const rptdev::PathState&, uint32_t n_paths);
  void (*extend)(hipStream_t, const rptdev::Scene&, const rptdev::PathState&, const uint32_t* queue, uint32_t n);
  void (*extend_rays)(hipStream_t, const rptdev::Scene&, const double* o, const double* d, uint64_t n, double* out_t,
                      double* out_n, int32_t* out_obj);
  // counters: [0] paths of the next depth, [1] hits, [2 + l] shadow rays queued for light l; sq: those queues ([light][cap])
  void (*shade)(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const rptdev::PathState&,
                const uint32_t* queue, uint32_t n, uint32_t depth, uint32_t* next_queue, uint32_t* counters, uint32_t* sq,
                uint32_t* zero_next /* rpt_shade clears these zero_n words: the next depth's counters */, uint32_t zero_n,
                uint32_t rec_off /* the depth's first record column (PathState::rec) */);
  // visibility of every light of the depth over its shadow-ray queue ([light][cap], lengths sq_counts[light] on the
  // device, the longest at most n_max), whole scene in the kernel (scenes without deep trees): one launch
  void (*shadow_rays)(hipStream_t, const rptdev::Scene&, const rptdev::PathState&, const uint32_t* sq_all,
                      const uint32_t* sq_counts, uint32_t n_max, int num_lights, double* srt);
  void (*resolve)(hipStream_t, const rptdev::Frame&, const rptdev::PathState&, uint32_t n_samples);
  // means into the full frame, or `packed` into a compact [npix][3] array in the order of Frame::pixels
  void (*finish)(hipStream_t, const rptdev::Frame&, double iterations, double ev_scale, void* out, bool f32, bool packed);
  // multi-GPU gather, root side: one rank's packed pixels into their places in the full f32 frame
  void (*scatter_f32)(hipStream_t, const float* src, const uint32_t* pixels, uint32_t n, float* dst);
  void (*eval_math)(hipStream_t, int fn, uint64_t n, const double* x, const double* y, double* out);
  // the persistent kernel, one element per form: [RPT_PATHS_FORM_COUNT], indexed by RPT_PATHS_FORM_*
  const PathsForm* paths;
  // pixel sums of a launch's samples, in sample order
  void (*sum_samples)(hipStream_t, const rptdev::Frame&, const double* lbuf, uint32_t spp, bool first);
  // deep-tree scenes: one closest-hit (light < 0) or visibility (light >= 0) query of a depth, run
  // object by object with per-tree ray compaction and persistent traversal
  void (*query)(hipStream_t, const rptdev::Scene&, const rptdev::PathState&, const uint32_t* queue, uint32_t n,
                int light, double* srt, const uint32_t* n_dev /* light >= 0: the device-side length of `queue` */, const uint8_t* obj_deep, const uint8_t* obj_tris, int num_objects,
                uint32_t* tq, uint32_t* tq_ctr, uint32_t trace_blocks, const SortBufs* sort, const QueryHook* hook,
                const StackSpill* spill /* the traversal stack beyond the LDS levels */, QueryTuning* qt);
  size_t (*sort_temp_bytes)(uint32_t n);
  void (*shadow_sum)(hipStream_t, const rptdev::Scene&, const rptdev::PathState&, const uint32_t* queue, uint32_t n,
                     uint32_t rec_off, const double* srt);
  // device-resident Buffer (buffer.rs).  accumulate: one batch into total and the per-pixel statistics — a full frame
  // (list == nullptr, n = pixels) or the packed values of n listed pixels, scattered into `frame`
  void (*buffer_accumulate)(hipStream_t, double* total, double* frame, const double* packed, const uint32_t* list,
                            uint32_t n, uint32_t* counts, double* mean, double* m2);
  // the stopping rule over the n listed pixels; the survivors into out_list in list order, their number into *out_n
  // (keep: n bytes, block_cnt: ceil(n / RPT_RETIRE_TILE) words of scratch; n > 0)
  void (*buffer_retire)(hipStream_t, const uint32_t* list, uint32_t n, const uint32_t* counts, const double* mean,
                        const double* m2, uint32_t min_batches, double abs_tol, double rel_tol, uint8_t* keep,
                        uint32_t* block_cnt, uint32_t* out_list, uint32_t* out_n);
  void (*buffer_image)(hipStream_t, const double* total, const uint32_t* counts, uint32_t w, uint32_t h, uint32_t radius,
                       const double* thr, uint8_t* out);
  void (*buffer_variance)(hipStream_t, const double* total, const double* const* batches, const uint32_t* counts,
                          uint64_t npix, double* out);
  // -DRPT_PROF builds: the per-phase table of kernels/prof.inc since the last call ([0] wave cycles, [1] lane cycles,
  // [2] wave iterations, [3] lane iterations); false in regular builds
  bool (*read_prof)(unsigned long long out[4][30]);
  // in-kernel-traversal scenes: the next depth's paths sorted by ray key into the current state arrays (kernels/wavefront.inc)
  void (*path_reorder)(hipStream_t, const rptdev::PathState&, uint32_t n, bool sorted, const SortBufs* sort, uint32_t* order);
  // first-hit feature buffers (kernels/aov.inc).  aov: camera ray, closest hit and the ordered fold of `iterations` samples
  // per pixel of the frame's part in one kernel (Frame::sample_base = the call's first sample).  aov_fold: the hits of a
  // pass of spp samples per pixel (rpt_raygen's slots, the depth-0 query's records) added to the sums; first = the pass
  // holds the call's first sample
  void (*aov)(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const rptdev::Camera&, const rptdev::AovOut&,
              uint32_t iterations);
  void (*aov_fold)(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const rptdev::PathState&, const rptdev::AovOut&,
                   uint32_t spp, bool first);
  // the device Buffer's denoising filter (kernels/denoise.inc; the contract: include/rpt_gpu.h).  prepare: the buffer's
  // means, prefiltered variance and the means of its held features as columns of `stride` elements.  level: one à-trous
  // pass at tap spacing `step` from (c_in, v_in) into (c_out, v_out).  finish: the colour columns as [pixel][3] f64 and /
  // or as bytes through the buffer's thresholds (either output may be null)
  void (*denoise_prepare)(hipStream_t, const double* total, const uint32_t* counts, const double* m2, const rptdev::AovOut& feat,
                          uint32_t w, uint32_t h, uint64_t stride, double* c_out, double* v_out, double* g_normal,
                          double* g_position, double* g_albedo, double* g_depth, uint8_t* g_hit);
  void (*denoise_level)(hipStream_t, const rptdev::DenoiseGuide&, const double* c_in, const double* v_in, double* c_out,
                        double* v_out, uint32_t step, const rptdev::DenoiseSigmas&);
  void (*denoise_finish)(hipStream_t, const double* c_in, uint64_t stride, uint64_t npix, const double* thr, double* out_linear,
                         uint8_t* out_rgb8);
  // light probes (rptgpu_bake_probes; kernels/wavefront.inc), beside raygen_rays / resolve / finish.  raygen_probes: the
  // first step for fr.npix probes at positions / normals ([npix][3] f64 on the device; normals only read for
  // RPT_PROBE_IRRADIANCE), ids_out / id_base as raygen_rays.  resolve_probes: a pass's paths into the probes' running sums
  // (fr.accum, [27 or 3][npix]).  finish_probes: the sums times scale into out, [npix][width]
  void (*raygen_probes)(hipStream_t, const rptdev::Frame&, const double* positions, const double* normals, uint32_t kind,
                        uint32_t* ids_out, uint32_t id_base, const rptdev::PathState&, uint32_t n_paths);
  void (*resolve_probes)(hipStream_t, const rptdev::Frame&, const rptdev::PathState&, uint32_t n_samples, uint32_t kind);
  void (*finish_probes)(hipStream_t, const rptdev::Frame&, uint32_t width, double scale, double* out);
  // a batch of views (rptgpu_render_views; kernels/wavefront.inc), beside raygen / raygen_rays: the first step for the
  // fr.npix consecutive indices j_base + i of the call, index j = view * (width * height) + pixel; views: the call's
  // records on the device; ids_out (= fr.pixels) receives the piece's stream ids, the pixels
  void (*raygen_views)(hipStream_t, const rptdev::Frame&, const rptdev::View* views, uint32_t width, uint32_t height,
                       uint64_t j_base, uint32_t* ids_out, const rptdev::PathState&, uint32_t n_paths);
  // visibility for the caller (rptgpu_occluded, rptgpu_bake_ao; kernels/occlusion.inc): the steps around a visibility query
  // of "light" 0.  occ_load: n rays of the caller ([n][3] f64 on the device, max_t [n] or null) into ps.ray and column 0 of
  // ps.shadow, the identity into sq with its length in *sq_count.  raygen_ao: the same for fr.npix points x the pass's
  // samples (n_slots = npix * samples of the pass; ids: the points' stream ids or null = id_base + i).  occ_store: the
  // answers in srt's column 0 as bytes.  ao_fold: a pass's answers into the points' running sums (fr.accum, [4][npix]);
  // last: the sums divided by the call's `samples` into out_ao [npix] and out_bent [npix][3] (may be null)
  void (*occ_load)(hipStream_t, const double* origins, const double* dirs, const double* max_t, const rptdev::PathState&,
                   uint32_t* sq, uint32_t* sq_count, uint32_t n);
  void (*raygen_ao)(hipStream_t, const rptdev::Frame&, const double* positions, const double* normals, const uint32_t* ids,
                    uint32_t id_base, double max_distance, const rptdev::PathState&, uint32_t* sq, uint32_t* sq_count,
                    uint32_t n_slots);
  void (*occ_store)(hipStream_t, const rptdev::PathState&, const double* srt, uint32_t n, uint8_t* out);
  void (*ao_fold)(hipStream_t, const rptdev::Frame&, const rptdev::PathState&, const double* srt, uint32_t n_samples, bool first,
                  bool last, uint32_t samples, double* out_ao, double* out_bent);
  // first-hit records for the caller (rptgpu_first_hits, rptgpu_render_views_aov; kernels/hits.inc).  first_hits: n rays of
  // the caller ([n][3] f64 on the device), the closest hit of each and the channels of out.channels into out's arrays at the
  // ray's index, in one kernel (scenes walked in-kernel).  hits_store: the same channels from the records of the n rays
  // rpt_raygen_rays laid into ps (one sample), behind the per-tree query.  views_aov_fold: aov_fold for a piece of a batch
  // of views — a pass's hits (slot = s * n + j) into the sums at index j of out's arrays; first = the pass holds the call's
  // first sample
  void (*first_hits)(hipStream_t, const rptdev::Scene&, const double* origins, const double* dirs, uint32_t n,
                     const rptdev::HitOut& out);
  void (*hits_store)(hipStream_t, const rptdev::Scene&, const rptdev::PathState&, uint32_t n, const rptdev::HitOut& out);
  void (*views_aov_fold)(hipStream_t, const rptdev::Scene&, const rptdev::PathState&, const rptdev::AovOut& out, uint32_t n,
                         uint32_t spp, bool first);
  // a batch of views with a seed per view (rptgpu_render_views_seeded, and rptgpu_render_views with a seed stride;
  // kernels/wavefront.inc).  raygen_views_seeded: raygen_views with view v's stream seeded by view_seeds[v] ([views of the
  // call] on the device) instead of fr.seed; seeds_out ([fr.npix]) receives the seed of each index of the piece.  One
  // launch covers the piece's indices p_lo .. p_lo + p_len - 1 (p_lo + p_len <= fr.npix, p_len > 0) with n_paths = p_len x
  // the pass's samples, in the slots s * fr.npix + index: the whole piece is (0, fr.npix).
  // shade_seeded: shade with the stream of the path of index i seeded by seeds[i] — raygen_views_seeded's seeds_out
  void (*raygen_views_seeded)(hipStream_t, const rptdev::Frame&, const rptdev::View* views, uint32_t width, uint32_t height,
                              uint64_t j_base, uint32_t* ids_out, const uint64_t* view_seeds, uint64_t* seeds_out,
                              uint32_t p_lo, uint32_t p_len, const rptdev::PathState&, uint32_t n_paths);
  void (*shade_seeded)(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const rptdev::PathState&, const uint32_t* queue,
                       uint32_t n, uint32_t depth, uint32_t* next_queue, uint32_t* counters, uint32_t* sq, uint32_t* zero_next,
                       uint32_t zero_n, uint32_t rec_off, const uint64_t* seeds);
  // the filter over a batch of views of one size (rptgpu_render_views_denoised; kernels/denoise.inc):
  // denoise_prepare / _level / _finish with every array and column holding n_views * w * h elements, view after view
  // (stride = that product), ONE launch each for the whole batch (the view in blockIdx.z; batches of more than 65535 views
  // take one launch per 65535), taps bounded by the view's own frame.  views_finish also gives the filter's unfiltered
  // inputs: out_mean = total / n ([index][3]) and out_variance = (M2 / (n - 1)) / n; any of its four outputs may be null
  void (*denoise_views_prepare)(hipStream_t, const double* total, const uint32_t* counts, const double* m2,
                                const rptdev::AovOut& feat, uint32_t w, uint32_t h, uint64_t n_views, uint64_t stride, double* c_out,
                                double* v_out, double* g_normal, double* g_position, double* g_albedo, double* g_depth,
                                uint8_t* g_hit);
  void (*denoise_views_level)(hipStream_t, const rptdev::DenoiseGuide&, uint64_t n_views, const double* c_in, const double* v_in,
                              double* c_out, double* v_out, uint32_t step, const rptdev::DenoiseSigmas&);
  void (*denoise_views_finish)(hipStream_t, const double* c_in, uint64_t stride, uint64_t n, const double* thr, double* out_linear,
                               uint8_t* out_rgb8, const double* total, const uint32_t* counts, const double* m2, double* out_mean,
                               double* out_variance);
  // path vertices for the caller (rptgpu_trace_vertices; kernels/wf_vertices.inc), beside raygen_rays' passes.  vertices_store:
  // the geometry and stream position of the n paths of depth `depth` (dense slots, behind the closest-hit query, in front of
  // shade) into out's arrays at (ray, sample, depth).  vertices_fold: at the end of a pass of n_paths paths, every path's
  // record chain — radiance, BSDF, 1/pdf, |cos|, the length — and the filler behind its last vertex
  void (*vertices_store)(hipStream_t, const rptdev::Frame&, const rptdev::PathState&, uint32_t n, uint32_t depth,
                         const rptdev::VertexOut& out);
  void (*vertices_fold)(hipStream_t, const rptdev::Frame&, const rptdev::PathState&, uint32_t n_paths, const rptdev::VertexOut& out);
  // beside the persistent kernel's forms (kernels/paths_views.inc, kernels/paths_rays.inc).  views_ids: the ids of a piece of n
  // consecutive indices of a batch of views from j_base on — pixels[i] the index's pixel in its view (the piece's
  // Frame::pixels), view_of[i] its view counted from the piece's first (ViewRays::view_of).  rays_ids: ids[i] = id_base + i for
  // the piece's n indices (a caller without stream ids).  project_probes: a launch's samples (lbuf, [spp][3][npix] as rpt_paths
  // writes it) into the probes' running sums (fr.accum, [27 or 3][npix]: resolve_probes' sums, finish_probes behind the last launch)
  void (*views_ids)(hipStream_t, uint64_t j_base, uint64_t npix_view, uint32_t n, uint32_t* pixels, uint32_t* view_of);
  void (*rays_ids)(hipStream_t, uint32_t id_base, uint32_t n, uint32_t* ids);
  void (*project_probes)(hipStream_t, const rptdev::Frame&, const double* lbuf, uint32_t spp, uint32_t kind);
  // direct light at the caller's points (rptgpu_bake_direct; kernels/direct.inc): the steps around the visibility queries of
  // every light.  raygen_direct: for fr.npix points x the pass's samples (n_slots, ids and id_base as raygen_ao) each light's
  // sample into its column of ps.shadow and the slot into the queues (sq, [light][cap]) of the lights that can add something,
  // their lengths in counters[2 + light], which the caller cleared.  direct_fold: a pass's answers into the points' running
  // sums (fr.accum, [3][npix]), sample-major; last: the sums divided by the call's `samples` into out [npix][3]
  void (*raygen_direct)(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const double* positions, const double* normals,
                        const uint32_t* ids, uint32_t id_base, const rptdev::PathState&, uint32_t* sq, uint32_t* counters,
                        uint32_t n_slots);
  void (*direct_fold)(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const rptdev::PathState&, const double* srt,
                      uint32_t n_samples, bool first, bool last, uint32_t samples, double* out);
};
// the forms' translation units (kernels_<form>_strict[_ext].hip): what the tables above point to — kernels/launch_paths.inc's
// two functions, and what else the form's file launches
#define RPT_FORM_TU_DECLS_NS(NS, ...)                                                                                  \
  namespace NS {                                                                                                       \
  int paths_max_blocks_per_cu(const FlatLayout* flat, uint32_t lds_bytes, bool park);                                  \
  void launch_paths(hipStream_t, const rptdev::Scene&, const rptdev::Frame&, const PathsRays&, const PathsLaunch&);    \
  __VA_ARGS__                                                                                                          \
  }
#define RPT_FORM_TU_DECLS(FORM, ...) \
  RPT_FORM_TU_DECLS_NS(rpt_strict_##FORM, __VA_ARGS__) RPT_FORM_TU_DECLS_NS(rpt_strict_ext_##FORM, __VA_ARGS__)
RPT_FORM_TU_DECLS(views, void launch_views_ids(hipStream_t, uint64_t j_base, uint64_t npix_view, uint32_t n, uint32_t* pixels,
                                               uint32_t* view_of);)
RPT_FORM_TU_DECLS(rays, void launch_rays_ids(hipStream_t, uint32_t id_base, uint32_t n, uint32_t* ids);
                  void launch_project_probes(hipStream_t, const rptdev::Frame&, const double* lbuf, uint32_t spp, uint32_t kind);)
RPT_FORM_TU_DECLS(vertices, )
#undef RPT_FORM_TU_DECLS
#undef RPT_FORM_TU_DECLS_NS

// rptgpu_hit_surface's resolve pass (kernels/hit_surface.inc), in translation units of its own (kernels_surface_strict[_ext].hip)
// and outside the tables: n rays of the caller ([n][3] f64 on the device), out.t / out.object the first-hit query's answers for
// them; the named channels of out are written.  gs: the walk's columns, blocks * 256 <= gs.threads.  groups_from_inf: some group
// of the scene holds a MonomialSurface (a group's walk then starts from +inf).  *overflow is raised if a walk outgrows gs
#define RPT_SURFACE_TU_DECLS(NS)                                                                                          \
  namespace NS {                                                                                                          \
  void launch_hit_surface(hipStream_t, const rptdev::Scene&, const double* origins, const double* dirs, uint32_t n,       \
                          const rptdev::SurfaceOut& out, const GenericStack& gs, bool groups_from_inf, uint32_t* overflow, \
                          uint32_t blocks);                                                                               \
  }
RPT_SURFACE_TU_DECLS(rpt_strict_surface)
RPT_SURFACE_TU_DECLS(rpt_strict_ext_surface)
#undef RPT_SURFACE_TU_DECLS

namespace rpt_strict { extern const KernelTable TABLE; } // -ffp-contract=off (parity mode)
// the same with the extended shape set (RPT_SHAPE_MONOMIAL, trees of trees) compiled in
namespace rpt_strict_ext { extern const KernelTable TABLE; }
