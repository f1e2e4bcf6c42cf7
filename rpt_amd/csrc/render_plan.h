// render_plan.h — how a render call is cut into launches (persistent pipeline) and passes (wavefront pipeline): the
// arithmetic behind api_render.cpp's drivers, as pure host functions of numbers (tests/cpp/render_plan_check.cpp), and the
// pieces rptgpu_trace_rays cuts its rays into (tests/cpp/rays_piece_check.cpp) and rptgpu_render_views its views' pixels
// (tests/cpp/views_piece_check.cpp; the working set of rptgpu_render_views_denoised: views_denoise_plan_check.cpp), rptgpu_occluded its rays and rptgpu_bake_ao its points (tests/cpp/occlusion_piece_check.cpp),
// rptgpu_first_hits its rays (tests/cpp/hits_piece_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/rpt_gpu.h"
#include "channel_plan.h"
#include "device_types.h"
#include "launch_limits.h"

namespace rptplan {

// the work items of a launch of spp samples per pixel, chunk samples per item
inline uint64_t work_items(uint32_t npix, uint32_t spp, uint32_t chunk) { return (uint64_t)npix * ((spp + chunk - 1) / chunk); }

// ---- persistent pipeline (rpt_paths): a batch runs as n_launch launches of spp_l samples each
struct PersistentPlan {
  uint32_t n_launch, spp_l, chunk; // launches, samples per pixel of each, samples per work item
  int per_cu;                      // one-wave blocks per CU
  uint64_t n_items;                // work items of a launch of spp_l samples
  uint32_t nblocks;
};

// per_cu: the occupancy query's answer; lbuf_cap: the cap on the per-sample radiance buffer (RPTGPU_LBUF_BYTES), lbuf_held:
// its bytes already allocated, free_bytes: the device's free memory (< 0: unknown); paths_chunk: RptSceneOptions::paths_chunk;
// all_flat, obj_filter: the scene is flat and runs the object filter; force_general: RPT_FLAG_GENERAL_TRAVERSAL
inline PersistentPlan plan_persistent(uint32_t npix, uint32_t iterations, uint32_t max_bounces, int cus, int per_cu,
                                      uint64_t lbuf_cap, uint64_t lbuf_held, int64_t free_bytes, uint32_t paths_chunk,
                                      bool all_flat, bool force_general, bool obj_filter) {
  PersistentPlan pl{};
  // one launch's per-sample radiance buffer (24 B per sample) stays under the cap: 512 spp at 1080p = 25.5 GB = one
  // launch; growing, it leaves half of what is free to everyone else
  uint64_t lbuf_budget = lbuf_cap;
  if (lbuf_held < lbuf_budget && free_bytes >= 0)
    lbuf_budget = std::min<uint64_t>(lbuf_budget, std::max<uint64_t>(lbuf_held, (uint64_t)free_bytes / 2));
  uint64_t spp_max = std::max<uint64_t>(1, lbuf_budget / ((uint64_t)npix * 3 * sizeof(double)));
  pl.n_launch = (uint32_t)(((uint64_t)iterations + spp_max - 1) / spp_max);
  pl.spp_l = pl.n_launch ? (iterations + pl.n_launch - 1) / pl.n_launch : 0;
  // Samples per work item.  paths_chunk = 0 (the default) chooses: 16 — 2 for flat scenes that run the object filter AND
  // trace long paths (max_bounces >= 4): there the lanes of a wave drift apart in path length and short items keep a wave
  // on one 8x8 pixel block and re-balance it often (the 23-polygon room at 8 bounces 617 -> 664 Msamples/s, spheres.rs at
  // 6 bounces 1899 -> 1981); with one or two segments per path every sample costs the same and the per-item bookkeeping
  // is all a short item adds (basic.rs 13418 -> 9391, the simple_video frame 111 -> 88 frames/s at 2:
  // profiles/r05_paths_chunk_ab.txt) — halved while a lane would get fewer than 24 items: the launch's tail is one item
  // long (a rank that owns an eighth of a 1080p frame at 128 spp: x1.056 of the ideal 1/8 with 16 samples per item, x1.014
  // with 4; profiles/r05_emulated_ranks.txt).
  uint32_t chunk = paths_chunk;
  if (chunk == 0u) {
    chunk = (all_flat && !force_general && obj_filter && max_bounces >= 4u) ? 2u : 16u;
    const uint64_t lanes = (uint64_t)std::max(1, cus) * 8u * 64u;
    while (chunk > 1u && work_items(npix, pl.spp_l, chunk) < 24u * lanes) chunk /= 2u;
  }
  chunk = std::max(1u, std::min(chunk, std::max(1u, pl.spp_l)));
  uint64_t n_items = work_items(npix, pl.spp_l, chunk);
  // 32-bit work counter: every lane of the grid may ask once past the end, and a wave's last guided claim may reach past
  // it (kernels/paths.inc fetch_item: at most 64 + 256 dead items per wave), so items + 8 x threads must fit (slack: at
  // most RPT_PATHS_WAVES_PER_CU_MAX one-wave blocks per CU — per_cu is clamped to it — each with up to 64 askers past the
  // end and one last claim of at most RPT_PATHS_BATCH_MAX, the cap of a caller's paths_batch)
  const uint64_t item_limit = 0xFFFFFFF0ull - (uint64_t)cus * RPT_PATHS_WAVES_PER_CU_MAX * (64u + RPT_PATHS_BATCH_MAX);
  if (n_items > item_limit) {
    chunk = (uint32_t)(((uint64_t)pl.spp_l * npix + item_limit - 1) / item_limit);
    while ((n_items = work_items(npix, pl.spp_l, chunk)) > item_limit) chunk++;
  }
  pl.chunk = chunk;
  pl.n_items = n_items;
  pl.per_cu = std::min(per_cu, (int)RPT_PATHS_WAVES_PER_CU_MAX);
  pl.nblocks = (uint32_t)std::max(1, cus * pl.per_cu);
  pl.nblocks = (uint32_t)std::min<uint64_t>(pl.nblocks, std::max<uint64_t>(1, (n_items + 63) / 64));
  return pl;
}

// ---- wavefront pipeline: paths in flight per pass.  Late bounces keep few paths alive, and a depth's kernels need ~10^5
// rays to fill 256 CUs, so the more paths start together the better the deep bounces run (C3 stand-in: 4 Mi -> 71, 16 Mi
// -> 106, 128 Mi -> 128 Msamples/s; 16k-triangle glass 179 -> 324; round 6, with passes of 85 % of the free memory:
// 786 -> 913, profiles/r06_pass_size_ab.txt).  288 GB of HBM is what makes that affordable.
// What a path costs: its slot and one 68-byte COLUMN per depth it reaches (PathState::rec) — as many columns as the
// depths' queues were long, not (max_bounces + 1) per path: the glass's paths average a quarter of their 17 levels.  How
// many columns a path needs is measured (the first pass of a handle is one sample per pixel with the full pool) and
// carried with a margin; a pass whose pool runs out at some depth is started over with fewer paths.
// a path's slot: ray and next ray, hit, object, draw / path id / parent column twice each, last column, per light the
// shadow state, queue entry and record time, the per-tree query's queue, row and sort words
inline uint64_t wavefront_slot_bytes(int num_lights, bool has_deep, bool sort_rays, bool path_reorder) {
  const uint64_t nl = (uint64_t)std::max(1, num_lights);
  return 2 * 6 * 8 + 4 * 8 + 4 + 6 * 4 + 4 + nl * rptdev::SHADOW_FIELDS * 8 + nl * (8 + 4) +
         (has_deep ? 12 + 64 + (sort_rays ? 12 + 16 : 0) : 0) + (path_reorder ? 16 + 16 + 4 : 0);
}
// a record column: the record and its parent link
constexpr uint64_t WAVEFRONT_REC_BYTES = rptdev::REC_FIELDS * 8 + 4;

// columns per path of a pass: measured + 10 % + 0.05, the full (max_bounces + 1) until there is a measurement (rounded up
// to a twentieth, so that the fourth digit of a pass's average does not resize a 100 GB workspace)
inline double pass_ratio(double rec_ratio, uint32_t max_bounces) {
  const double full_ratio = (double)max_bounces + 1.0;
  return rec_ratio > 0.0 ? std::min(full_ratio, std::ceil((rec_ratio * 1.10 + 0.05) * 20.0) / 20.0) : full_ratio;
}

struct PassInput {
  uint32_t npix, iterations, remaining; // pixels, samples of the call, samples still to run
  double rec_ratio, ratio;   // record columns per path measured so far (0: not yet, this pass measures); pass_ratio() of it
  uint64_t per_slot;         // wavefront_slot_bytes()
  uint64_t target_paths;     // paths per pass asked for (RPTGPU_TARGET_PATHS); 0 = from the budget
  uint64_t budget_bytes;     // the workspace cap (RPTGPU_WS_BYTES)
  int64_t free_bytes;        // the device's free memory (< 0: unknown) ...
  uint64_t free_percent;     // ... and the share of it a pass may take
  uint64_t held_slots, held_cols; // the workspace the handle holds (it counts as available)
  uint64_t fail_paths;       // the smallest pass (paths) whose workspace did not fit so far; 0 = none
};
struct PassPlan {
  uint64_t target;  // paths per pass
  uint32_t s_chunk; // samples per pixel of this pass
  uint32_t s_alloc; // samples per pixel the workspace is made for
};

inline PassPlan plan_pass(const PassInput& in) {
  PassPlan pp{};
  const double per_path = (double)in.per_slot + in.ratio * (double)WAVEFRONT_REC_BYTES;
  pp.target = in.target_paths;
  if (!pp.target) {
    uint64_t budget = in.budget_bytes;
    if (in.free_bytes >= 0) {
      const uint64_t have = in.held_slots * in.per_slot + in.held_cols * WAVEFRONT_REC_BYTES;
      budget = std::min<uint64_t>(budget, ((uint64_t)in.free_bytes + have) / 100 * in.free_percent);
    }
    pp.target = std::min<uint64_t>(RPT_MAX_PATHS_PER_PASS, std::max<uint64_t>(1ull << 20, (uint64_t)((double)budget / per_path)));
  }
  // a size that did not fit before is not tried again (several handles or processes on one GPU see the same `free`
  // figure; an explicit target_paths may be more than the device holds): allocating and freeing 100+ GB per call costs
  // seconds
  if (in.fail_paths) pp.target = std::min<uint64_t>(pp.target, in.fail_paths / 2);
  pp.s_chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(in.remaining, pp.target / in.npix));
  if (in.rec_ratio == 0.0 && in.remaining > 1u && pp.s_chunk > 1u) {
    pp.s_chunk = 1u; // the measuring pass: one sample per pixel, every path with room for all its levels
  } else if (pp.s_chunk < in.remaining) {
    // passes of EQUAL size: 256 spp with room for 123 per pass are three passes of 86 / 85 / 85, not 123 / 123 / 10 (the
    // deep bounces of a 10-spp pass run on a tenth of the rays)
    const uint32_t n_pass = (in.remaining + pp.s_chunk - 1) / pp.s_chunk;
    pp.s_chunk = (in.remaining + n_pass - 1) / n_pass;
  }
  // The workspace is made for the pass a call of this size runs once the measurement is in — not for this pass's own
  // size: the first call's passes are 1 + (n - 1) samples, and a workspace of n - 1 would be freed and made again by the
  // second call (220 GB: six seconds)
  pp.s_alloc = pp.s_chunk;
  if (in.rec_ratio > 0.0) pp.s_alloc = (uint32_t)std::max<uint64_t>(pp.s_chunk, std::min<uint64_t>(in.iterations, pp.target / in.npix));
  return pp;
}

// the path slots and record columns of the workspace a pass asks for
inline uint64_t pass_slots(uint32_t npix, const PassPlan& pp) { return (uint64_t)npix * std::max(pp.s_chunk, pp.s_alloc); }
inline uint64_t pass_rec_cols(uint64_t np, double ratio) {
  return std::max<uint64_t>(np, std::min<uint64_t>((uint64_t)std::ceil((double)np * ratio), 0xfffffff0ull));
}

// the workspace of a pass did not fit (several handles or processes on one GPU each see the same `free` figure): the pass
// shrinks instead of failing the render (a smaller pass is only slower) — first the room ahead goes, then the pass halves
inline PassPlan shrink_after_oom(PassPlan pp) {
  if (pp.s_alloc > pp.s_chunk) pp.s_alloc = pp.s_chunk;
  else { pp.s_chunk = std::max(1u, pp.s_chunk / 2); pp.s_alloc = pp.s_chunk; }
  return pp;
}
inline uint64_t fail_paths_after_oom(uint64_t fail_paths, uint64_t np) { return fail_paths ? std::min<uint64_t>(fail_paths, np) : np; }

// the columns per path measured: the largest average seen ...
inline double ratio_after_pass(double rec_ratio, uint64_t cols_used, uint32_t n_paths) { return std::max(rec_ratio, (double)cols_used / (double)n_paths); }
// ... and after a pass whose pool ran out (cols_seen: the columns up to the depth that did not fit, a lower bound of what
// it needs): room for half as many again
inline double ratio_after_restart(double rec_ratio, uint64_t cols_seen, uint32_t n_paths, uint32_t max_bounces) {
  const double seen = (double)cols_seen / (double)n_paths;
  return std::min((double)max_bounces + 1.0, std::max(rec_ratio, seen) * 1.5);
}

// ---- rptgpu_trace_rays: the caller's n rays run through the wavefront pipeline in pieces, each piece the "frame" of its
// own passes (npix = the piece's rays).  The smallest pass is one sample of every ray of the piece, so a piece holds at
// most the paths a pass may have — pass_target: plan_pass's target for the scene with room for every level of every path
// — and then piece x s_chunk <= pass_target <= RPT_MAX_PATHS_PER_PASS: the pass fits the workspace and its slots fit 32
// bits.  Without a wish a piece is at most RAYS_PIECE_MAX rays, what rptgpu_closest_hit takes at a time (48 B of ray and
// 24 B of result per ray staged for a host caller).  asked: RPTGPU_RAYS_PIECE (tests; 0 = not set), within the same bound.
constexpr uint64_t RAYS_PIECE_MAX = 4ull << 20;
inline uint64_t rays_piece(uint64_t n, uint64_t asked, uint64_t pass_target) {
  const uint64_t fit = std::max<uint64_t>(1, std::min<uint64_t>(pass_target, RPT_MAX_PATHS_PER_PASS));
  return std::max<uint64_t>(1, std::min(std::min<uint64_t>(n, asked ? asked : RAYS_PIECE_MAX), fit));
}
inline uint64_t rays_piece_count(uint64_t n, uint64_t piece) { return (n + piece - 1) / piece; }

// ---- rptgpu_render_views: n_views frames of npix pixels are the n = n_views * npix indices j = view * npix + pixel of one
// call, cut into pieces of consecutive j — the "frame" of a piece's passes, as a piece of rays is: rays_piece's bound and
// wish (asked: RPTGPU_VIEWS_PIECE) hold as they stand (the default cap of RAYS_PIECE_MAX indices was chosen for a host caller's
// staging; here it also decides how many views share a depth loop — DESIGN.md §15 has what a larger piece measured).  A piece's Frame carries ONE seed, so when the views' seeds differ
// (at_views: seed_stride != 0) no piece crosses a view boundary; otherwise pieces end inside views and span them.
inline uint64_t views_piece(uint64_t n, uint64_t asked, uint64_t pass_target) { return rays_piece(n, asked, pass_target); }
// the length of the piece that starts at index base < n
inline uint64_t views_piece_len(uint64_t base, uint64_t n, uint64_t npix, uint64_t piece, bool at_views) {
  uint64_t m = std::min(piece, n - base);
  if (at_views) m = std::min(m, npix - base % npix);
  return m;
}

// ---- rptgpu_render_views under RPT_FLAG_VIEWS_PERSISTENT: a piece's m indices are the "pixels" of rpt_paths_views'
// launches (kernels/paths_views.inc), a launch of spp samples in items of `chunk` samples of one index.  The kernel's work
// counter has 32 bits, and beside the launch's items it counts the dead claims past the end (kernels/paths.inc fetch_item:
// per one-wave block at most 64 askers and one last claim of at most batch_max items), so a launch needs
//   work_items(m, spp, chunk) + nblocks * (64 + batch_max) <= 2^32 - 1          (tests/cpp/views_items_check.cpp)
constexpr uint64_t VIEWS_COUNTER_MAX = 0xffffffffull;
inline uint64_t views_dead_room(uint32_t nblocks, uint32_t batch_max) { return (uint64_t)nblocks * (64ull + batch_max); }
struct ViewsItems {
  uint64_t m;       // the piece's length, capped so that the launch fits the counter; 0: not even one index fits
  uint64_t n_items; // work items of a launch over m indices
  bool capped;      // m is less than was asked for
};
inline ViewsItems views_items(uint64_t m, uint32_t spp, uint32_t chunk, uint32_t nblocks, uint32_t batch_max) {
  ViewsItems vi{};
  chunk = std::max(1u, chunk);
  const uint64_t per_index = ((uint64_t)spp + chunk - 1) / chunk, room = views_dead_room(nblocks, batch_max);
  const uint64_t fit = room >= VIEWS_COUNTER_MAX || !per_index ? 0 : (VIEWS_COUNTER_MAX - room) / per_index;
  vi.m = std::min(m, std::min<uint64_t>(fit, 0xffffffffull)); // (Frame::npix has 32 bits)
  vi.capped = vi.m < m;
  vi.n_items = vi.m * per_index;
  return vi;
}
// item i of a launch over m indices (fetch_item's arithmetic): its index of the piece and its samples [s_first, s_end)
struct ViewsItem { uint64_t index; uint32_t s_first, s_end; };
inline ViewsItem views_item(uint64_t item, uint64_t m, uint32_t spp, uint32_t chunk) {
  const uint64_t c = item / m;
  const uint32_t s_first = (uint32_t)(c * chunk);
  return ViewsItem{item - c * m, s_first, (uint32_t)std::min<uint64_t>((uint64_t)s_first + chunk, spp)};
}
// index i of the piece that starts at the call's index j_base: its view and its pixel there (rpt_views_ids' arithmetic;
// view_local: counted from the piece's first view, ViewRays::view_of)
struct ViewsIndex { uint64_t view; uint32_t pixel, view_local; };
inline ViewsIndex views_index(uint64_t j_base, uint64_t i, uint64_t npix_view) {
  const uint64_t j = j_base + i, v = j / npix_view;
  return ViewsIndex{v, (uint32_t)(j - v * npix_view), (uint32_t)(v - j_base / npix_view)};
}

// ---- rptgpu_trace_rays / rptgpu_bake_probes under RPT_FLAG_RAYS_PERSISTENT: a piece's m rays or probes are the "pixels" of
// rpt_paths_rays' launches (kernels/paths_rays.inc), so the piece rays_piece gives is additionally capped by what the work
// counter holds — views_items' arithmetic with npix = m, at chunk 1 (the most items a launch of `iterations` samples can have)
// and the most resident blocks any instantiation has: whatever launch plan render_persistent then runs over the piece fits
// (tests/cpp/rays_items_check.cpp).  Never 0: one ray is still a piece (render_persistent throws if even that overflows)
inline uint64_t rays_persistent_piece(uint64_t piece, uint32_t iterations, uint32_t blocks_max, uint32_t batch_max) {
  return std::max<uint64_t>(1, views_items(piece, iterations, 1, blocks_max, batch_max).m);
}

// ---- rptgpu_occluded / rptgpu_bake_ao: one visibility query per pass over rays laid into the workspace's slots, so a pass
// holds at most pass_target rays (plan_pass's target for the scene with ONE record column per path: no depth follows),
// never more than RPT_MAX_PATHS_PER_PASS (32-bit slots) and never more than OCCLUSION_PIECE_MAX (a host caller stages 56 B
// per ray; a larger pass has not been measured): occlusion_pass_max.  rptgpu_occluded cuts its n rays into runs of occlusion_piece rays,
// each one pass.  rptgpu_bake_ao cuts its n points into pieces of ao_piece WHOLE points — a point's running sums live with
// its piece — and a piece's S directions into passes of ao_pass_samples directions of every point of the piece: points x
// samples <= the bound, and when S alone exceeds it a piece is one point in several passes.  asked: RPTGPU_OCCLUSION_PIECE
// (tests; 0 = not set) — rays per piece, or points per piece —, within the same bound.
constexpr uint64_t OCCLUSION_PIECE_MAX = 16ull << 20;
inline uint64_t occlusion_pass_max(uint64_t pass_target) {
  return std::max<uint64_t>(1, std::min<uint64_t>(pass_target, std::min<uint64_t>(RPT_MAX_PATHS_PER_PASS, OCCLUSION_PIECE_MAX)));
}
inline uint64_t occlusion_piece(uint64_t n, uint64_t asked, uint64_t pass_target) {
  const uint64_t fit = occlusion_pass_max(pass_target);
  return std::max<uint64_t>(1, std::min(std::min<uint64_t>(n, asked ? asked : fit), fit));
}
inline uint64_t ao_piece(uint64_t n, uint64_t asked, uint32_t samples, uint64_t pass_target) {
  const uint64_t fit = occlusion_pass_max(pass_target);
  const uint64_t want = asked ? asked : std::max<uint64_t>(1, fit / std::max(1u, samples));
  return std::max<uint64_t>(1, std::min(std::min(n, want), fit));
}
// the directions per point of the next pass of a piece of `points` points with `remaining` directions to go
inline uint32_t ao_pass_samples(uint64_t points, uint32_t remaining, uint64_t pass_target) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(remaining, occlusion_pass_max(pass_target) / std::max<uint64_t>(1, points)));
}

// ---- rptgpu_first_hits: the caller's n rays in runs of hits_piece consecutive rays, each run one closest-hit query.
// pass_bound: the rays one query may hold — for scenes with deep trees plan_pass's target with ONE record column per path (the
// rays are laid into the workspace's slots and no depth follows), for scenes walked in-kernel no bound at all (~0: the fused
// kernel touches no workspace).  Either way a piece's indices fit 32 bits and it is at most HITS_PIECE_MAX rays, what
// rptgpu_closest_hit takes at a time: a host caller stages 48 B of ray and up to 100 B of record per ray.  asked:
// RPTGPU_HITS_PIECE (tests; 0 = not set), within the same bound.  Never 0, so `for (base = 0; base < n; base += piece)` ends.
constexpr uint64_t HITS_PIECE_MAX = RAYS_PIECE_MAX;
inline uint64_t hits_pass_max(uint64_t pass_bound) {
  return std::max<uint64_t>(1, std::min<uint64_t>(pass_bound, std::min<uint64_t>(RPT_MAX_PATHS_PER_PASS, HITS_PIECE_MAX)));
}
inline uint64_t hits_piece(uint64_t n, uint64_t asked, uint64_t pass_bound) {
  const uint64_t fit = hits_pass_max(pass_bound);
  return std::max<uint64_t>(1, std::min(std::min<uint64_t>(n, asked ? asked : fit), fit));
}

// RptHitArrays' channels in staging order (channel_plan.h): a host caller's piece of records, OBJECT behind the f64 channels
enum { HIT_R_T, HIT_R_NORMAL, HIT_R_POSITION, HIT_R_ALBEDO, HIT_R_OBJECT };
constexpr rptchan::Row HIT_ROWS[] = {RPT_CHANNEL_ROW(RptHitArrays, RPT_HIT_T, t, 1, 8, 0),
                                     RPT_CHANNEL_ROW(RptHitArrays, RPT_HIT_NORMAL, normal, 3, 8, 0),
                                     RPT_CHANNEL_ROW(RptHitArrays, RPT_HIT_POSITION, position, 3, 8, 0),
                                     RPT_CHANNEL_ROW(RptHitArrays, RPT_HIT_ALBEDO, albedo, 3, 8, 0),
                                     RPT_CHANNEL_ROW(RptHitArrays, RPT_HIT_OBJECT, object, 1, 4, 0)};
// ... and RptAovBuffers' (rptgpu_render_aov, rptgpu_render_views_aov).  hits is no channel — it is always written —: a row
// with a bit of its own that every walker of the table adds to the caller's, between the f64 arrays and OBJECT
constexpr uint32_t AOV_HITS = 1u << 31;
enum { AOV_R_DEPTH, AOV_R_NORMAL, AOV_R_ALBEDO, AOV_R_POSITION, AOV_R_HITS, AOV_R_OBJECT };
constexpr rptchan::Row AOV_ROWS[] = {RPT_CHANNEL_ROW(RptAovBuffers, RPT_AOV_DEPTH, depth, 1, 8, 0),
                                     RPT_CHANNEL_ROW(RptAovBuffers, RPT_AOV_NORMAL, normal, 3, 8, 0),
                                     RPT_CHANNEL_ROW(RptAovBuffers, RPT_AOV_ALBEDO, albedo, 3, 8, 0),
                                     RPT_CHANNEL_ROW(RptAovBuffers, RPT_AOV_POSITION, position, 3, 8, 0),
                                     rptchan::Row{AOV_HITS, 1, 4, 0, (uint32_t)offsetof(RptAovBuffers, hits),
                                                  "RptAovBuffers: hits is NULL (it is always written)"},
                                     RPT_CHANNEL_ROW(RptAovBuffers, RPT_AOV_OBJECT, object, 1, 4, 0)};

// RptVertexArrays' channels in the order of the struct's pointers, which is their staging order (channel_plan.h): per vertex,
// but LENGTH per path.  (RGB is no row: rpt_finish writes a piece's means through the ray call's own output.)
constexpr rptchan::Row VERTEX_ROWS[] = {RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_LENGTH, length, 1, 4, 1),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_T, t, 1, 8, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_NORMAL, normal, 3, 8, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_OBJECT, object, 1, 4, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_POSITION, position, 3, 8, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_DIRECTION, direction, 3, 8, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_DRAW, draw, 1, 4, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_RADIANCE, radiance, 3, 8, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_BSDF, bsdf, 3, 8, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_INV_PDF, inv_pdf, 1, 8, 0),
                                        RPT_CHANNEL_ROW(RptVertexArrays, RPT_VERTEX_ABS_COS, abs_cos, 1, 8, 0)};
// a call's counts for `rays` rays: vertices and paths
inline rptchan::Counts vertex_counts(uint64_t rays, uint32_t iterations, uint32_t max_bounces) {
  return rptchan::Counts(rays * iterations * ((uint64_t)max_bounces + 1), rays * iterations);
}

// ---- rptgpu_trace_vertices: rptgpu_trace_rays' pieces (rays_piece's bound and default hold as they stand; asked:
// RPTGPU_VERTICES_PIECE) — and for a host caller, whose records are staged on the device piece by piece, also at most the rays
// whose named channels fit VERTICES_STAGING_MAX bytes: piece x iterations x (max_bounces + 1) x vertices_vertex_bytes, plus
// vertices_path_bytes per path.  A piece is never empty: one ray whose records alone exceed the cap is still a piece.
// The cap's value is a CHOICE nobody has measured: 1 GiB is 7 M vertices with every channel, large enough that a piece's
// passes have the paths to fill the device and small against its memory.
constexpr uint64_t VERTICES_STAGING_MAX = 1ull << 30;
// bytes per vertex / per path of the channels named in `channels`, by the bit positions of RPT_VERTEX_* (include/
// rpt_gpu_vertices.h; api_vertices.cpp holds the two to each other): LENGTH is per path, RGB per ray (rays_piece's 24 B)
constexpr uint32_t VERTICES_CHANNEL_BITS = 12;
constexpr uint32_t VERTICES_VERTEX_BYTES[VERTICES_CHANNEL_BITS] = {0, 8, 24, 4, 24, 24, 4, 24, 24, 8, 8, 0};
constexpr uint64_t vertices_vertex_bytes(uint32_t channels) {
  uint64_t b = 0;
  for (uint32_t k = 0; k < VERTICES_CHANNEL_BITS; k++)
    if (channels >> k & 1u) b += VERTICES_VERTEX_BYTES[k];
  return b;
}
constexpr uint64_t vertices_path_bytes(uint32_t channels) { return (channels & 1u) ? 4u : 0u; }
// the staged bytes of `rays` rays (saturating: a product that does not fit is more than any cap)
inline uint64_t vertices_staging_bytes(uint64_t rays, uint32_t iterations, uint32_t max_bounces, uint32_t channels) {
  const uint64_t per_ray = (uint64_t)iterations * (((uint64_t)max_bounces + 1) * vertices_vertex_bytes(channels) + vertices_path_bytes(channels));
  return per_ray && rays > ~0ull / per_ray ? ~0ull : rays * per_ray;
}
inline uint64_t vertices_piece(uint64_t n, uint64_t asked, uint64_t pass_target, bool host, uint32_t iterations,
                               uint32_t max_bounces, uint32_t channels) {
  uint64_t piece = rays_piece(n, asked, pass_target);
  if (host) {
    const uint64_t per_ray = vertices_staging_bytes(1, iterations, max_bounces, channels);
    if (per_ray) piece = std::max<uint64_t>(1, std::min(piece, VERTICES_STAGING_MAX / per_ray));
  }
  return piece;
}
// ... under RPT_FLAG_VERTICES_PERSISTENT (include/rpt_gpu_vertices_persistent.h): the piece is the smaller of vertices_piece —
// the staging cap of a host caller's named channels holds as it stands — and what rpt_paths_vertices' 32-bit work counter
// holds (rays_persistent_piece).  The second only ever cuts the first, so both caps hold and a piece is never empty
// (tests/cpp/vertices_persistent_piece_check.cpp)
inline uint64_t vertices_persistent_piece(uint64_t n, uint64_t asked, uint64_t pass_target, bool host, uint32_t iterations,
                                          uint32_t max_bounces, uint32_t channels, uint32_t blocks_max, uint32_t batch_max) {
  return rays_persistent_piece(vertices_piece(n, asked, pass_target, host, iterations, max_bounces, channels), iterations, blocks_max,
                               batch_max);
}
// n * iterations * (max_bounces + 1) vertices: every per-vertex array (24 B per vertex at most) fits a 64-bit byte index
constexpr uint64_t VERTICES_MAX = 1ull << 56;
inline bool vertices_fit(uint64_t n, uint32_t iterations, uint32_t max_bounces) {
  const uint64_t per_ray = (uint64_t)iterations * ((uint64_t)max_bounces + 1); // < 2^40
  return !per_ray || n <= (VERTICES_MAX - 1) / per_ray; // n * per_ray < 2^56
}

// ---- rptgpu_render_views_denoised: the batch's n = n_views * npix indices hold their state, a batch's frame, the feature
// sums and the filter's columns at once (tests/cpp/views_denoise_plan_check.cpp).  n must fit 32 bits less one:
// rpt_buffer_accumulate indexes in uint32_t and its launch covers n rounded up to 256.  Bytes per array group, for the
// caller to report and for DESIGN.md §18's figure; `outputs` only for a host caller, whose results are staged on the device.
constexpr uint64_t VIEWS_DENOISE_MAX_N = 0xffffffffull;
struct ViewsDenoisePlan {
  uint64_t n;        // indices of the batch; 0: the batch does not fit (or there is nothing to do)
  uint64_t state;    // total [n][3], mean [n][3], M2 [n] f64 and counts [n] u32
  uint64_t staging;  // one batch's frame [n][3] f64
  uint64_t features; // hits [n] u32 (padded to a double), depth [n], normal, albedo, position [n][3] f64
  uint64_t columns;  // 18 f64 columns of n and the hit flags [n] u8
  uint64_t outputs;  // a host caller's requested outputs: denoised 24, rgb8 3, mean 24, variance 8 B per index
  uint64_t bytes() const { return state + staging + features + columns + outputs; }
};
inline ViewsDenoisePlan views_denoise_plan(uint64_t n_views, uint64_t npix, bool host, bool denoised, bool rgb8, bool mean,
                                           bool variance) {
  ViewsDenoisePlan p{};
  if (!n_views || !npix || n_views > VIEWS_DENOISE_MAX_N / npix) return p; // (the quotient first: the product may not fit 64 bits)
  const uint64_t n = n_views * npix;
  p.n = n;
  p.state = n * (24 + 24 + 8 + 4);
  p.staging = n * 24;
  p.features = rptchan::layout(AOV_ROWS, RPT_AOV_DEPTH | RPT_AOV_NORMAL | RPT_AOV_ALBEDO | RPT_AOV_POSITION | AOV_HITS, n).words * 8; // aov_arrays'
  p.columns = n * (18 * 8 + 1);
  if (host) p.outputs = n * ((denoised ? 24u : 0u) + (rgb8 ? 3u : 0u) + (mean ? 24u : 0u) + (variance ? 8u : 0u));
  return p;
}
// the samples base .. base + count - 1 (count >= 1) are all 64-bit indices
inline bool sample_range_fits(uint64_t base, uint64_t count) { return count - 1 <= ~0ull - base; }

} // namespace rptplan
