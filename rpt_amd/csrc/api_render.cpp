// api_render.cpp — workspace, the wavefront loop and the persistent launch behind every render entry point (their sizes:
// render_plan.h); rptgpu_render_batch[_device], rptgpu_closest_hit, rptgpu_eval_math (see api_internal.h)
#include "api_internal.h"

namespace rptapi {

int event_pair_begin(rptgpu_scene* h, int kind, bool on) {
  h->stats.kernel_launches[kind]++;
  if (!on || h->ev_used + 2 > MAX_EVENT_PAIRS * 2) return -1;
  while ((int)h->ev_pool.size() < h->ev_used + 2) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    h->ev_pool.push_back(e);
  }
  const int e0 = h->ev_used;
  h->ev_used += 2;
  HIP_TRY(hipEventRecord(h->ev_pool[e0], h->stream));
  return e0;
}
void event_pair_end(rptgpu_scene* h, int kind, int e0) {
  if (e0 < 0) return;
  HIP_TRY(hipEventRecord(h->ev_pool[e0 + 1], h->stream));
  h->pending.push_back({kind, e0, e0 + 1});
}

// profiling: bracket a launch with an event pair; resolved at the end of the call
struct Bracket {
  rptgpu_scene* h;
  int kind, e0;
  Bracket(rptgpu_scene* h_, int kind_, bool on) : h(h_), kind(kind_), e0(event_pair_begin(h_, kind_, on)) {}
  void done() { event_pair_end(h, kind, e0); }
};

// launch_query's accounting hook: phases of a query bracketed with pool events like every other launch
struct QueryMarks {
  rptgpu_scene* h;
  bool on;
  int e0[RPT_K_COUNT];
  QueryMarks(rptgpu_scene* h_, bool on_) : h(h_), on(on_) {
    for (int& e : e0) e = -1;
  }
};
void query_mark(void* ctx, int kind, int end) {
  QueryMarks* q = (QueryMarks*)ctx;
  if (kind < 0 || kind >= RPT_K_COUNT) return;
  if (!end) {
    q->e0[kind] = event_pair_begin(q->h, kind, q->on);
  } else {
    event_pair_end(q->h, kind, q->e0[kind]);
    q->e0[kind] = -1;
  }
}

void drain_events(rptgpu_scene* h) {
  for (auto& p : h->pending) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_pool[p.e0], h->ev_pool[p.e1]));
    h->stats.kernel_ms[p.kind] += ms;
  }
  h->pending.clear();
  h->ev_used = 0;
}

// the pixels of part pi of pc, in the order the path kernels walk them: 8x8-pixel blocks, row-major inside a block —
// the 64 lanes of a wave start on one compact block, so their paths see the same part of the scene (coherent
// traversal, similar lengths)
std::vector<uint32_t> pixel_list(uint32_t width, uint32_t height, uint32_t tw, uint32_t th, uint32_t pi, uint32_t pc) {
  std::vector<uint32_t> pix;
  uint32_t tiles_x = (width + tw - 1) / tw;
  pix.reserve((size_t)width * height / pc + 1);
  for (uint32_t by = 0; by < height; by += 8)
    for (uint32_t bx = 0; bx < width; bx += 8)
      for (uint32_t y = by; y < std::min(by + 8, height); y++)
        for (uint32_t x = bx; x < std::min(bx + 8, width); x++) {
          uint32_t tile = (y / th) * tiles_x + (x / tw);
          if (pc <= 1 || tile % pc == pi) pix.push_back(y * width + x);
        }
  return pix;
}
void ensure_partition(rptgpu_scene* h, const RptRenderParams& p) {
  uint32_t tw = p.tile_width ? p.tile_width : 32, th = p.tile_height ? p.tile_height : 8;
  uint32_t pc = p.part_count ? p.part_count : 1, pi = p.part_count ? p.part_index : 0;
  uint32_t key[6] = {p.width, p.height, tw, th, pi, pc};
  if (std::memcmp(key, h->part_key, sizeof key) == 0 && h->pixels.p) return;
  std::vector<uint32_t> pix = pixel_list(p.width, p.height, tw, th, pi, pc);
  h->pixels.upload(pix, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->npix = (uint32_t)pix.size();
  std::memcpy(h->part_key, key, sizeof key);
}

// rpt_tree_generic's columns: a small grid for the few rays the fast kernels hand on, a large one when whole objects
// (or, under RPT_FLAG_GENERAL_TRAVERSAL, everything) go through it.  Heights: what the scene's deepest nest needs.
void ensure_generic(rptgpu_scene* h, bool all) {
  const uint32_t blocks_few = 64, blocks_all = (uint32_t)std::max(64, std::min(1024, h->num_cus * 4));
  const uint32_t want = (all ? blocks_all : blocks_few) * 256u;
  if (h->gen_threads < want) {
    const uint64_t levels = std::max(1u, h->gen_levels), frames = std::max(1u, h->gen_frames);
    h->gen_defer.release(); h->gen_frame.release();
    h->gen_defer.alloc(levels * 8u * want);
    h->gen_frame.alloc(frames * 12u * want);
    h->gen_overflow.alloc(1);
    HIP_TRY(hipMemsetAsync(h->gen_overflow.p, 0, sizeof(uint32_t), h->stream));
    h->gen_threads = want;
  }
  h->spill.gen = GenericStack{h->gen_defer.p, h->gen_frame.p, h->gen_threads, std::max(1u, h->gen_levels), std::max(1u, h->gen_frames)};
  h->spill.gen_overflow = h->gen_overflow.p;
  h->spill.gen_blocks_few = blocks_few;
  h->spill.gen_blocks_all = h->gen_threads / 256u >= blocks_all ? blocks_all : blocks_few;
}

// (a profiled render's event pairs are resolved here, between the synchronisation and the flag: the stream is idle; no
// other call has any)
int drain_call(rptgpu_scene* h, bool read_overflow) {
  hipStream_t st = h->stream;
  uint32_t gen_overflow = 0;
  if (read_overflow) HIP_TRY(hipMemcpyAsync(&gen_overflow, h->gen_overflow.p, sizeof gen_overflow, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  drain_events(h);
  if (gen_overflow) {
    (void)hipMemsetAsync(h->gen_overflow.p, 0, sizeof(uint32_t), st);
    return fail(h, RPTGPU_E_TREE_TOO_DEEP, "rpt_tree_generic: the traversal outgrew the stack sized for this scene (internal error)");
  }
  return RPTGPU_OK;
}

// the keys, values and scratch of the rocPRIM sorts of cap entries (a tree's queue, or a depth's paths)
void ensure_sort_bufs(rptgpu_scene* h, uint64_t cap) {
  h->sort_kin.alloc(cap); h->sort_kout.alloc(cap); h->sort_vin.alloc(cap);
  size_t bytes = rpt_strict::TABLE.sort_temp_bytes((uint32_t)cap);
  h->sort_tmp.alloc(bytes);
  h->sort_bufs = SortBufs{h->sort_kin.p, h->sort_kout.p, h->sort_vin.p, h->sort_tmp.p, bytes};
}

uint32_t zeros_common(const std::vector<rptdev::Light>& lights) {
  for (const rptdev::Light& l : lights) // every shadow ray towards an axis-parallel directional light has a zero component
    if (l.kind == RPT_LIGHT_DIRECTIONAL && (l.vec[0] == 0.0 || l.vec[1] == 0.0 || l.vec[2] == 0.0)) return 1;
  return 0;
}

// cap: path slots; rec_cols: columns of the depth-record pool (PathState::rec: one per path and depth REACHED)
void ensure_workspace(rptgpu_scene* h, uint64_t cap, uint64_t rec_cols) {
  if (cap <= h->ws_cap && rec_cols <= h->ws_rec_cols && h->ray.p && !h->ws_stale) return;
  cap = std::max(cap, h->ws_cap);
  rec_cols = std::max(rec_cols, h->ws_rec_cols);
  int nl = std::max(1, h->dscene.num_lights);
  h->ray.alloc(6 * cap);
  h->hit.alloc(4 * cap);
  h->hit_obj.alloc(cap);
  h->draw.alloc(cap); h->pid.alloc(cap); h->col.alloc(cap);
  if (h->path_reorder) { // the survivors' next state as 64-byte rows (gathered in sorted order by rpt_path_permute)
    h->next_rows.alloc(8 * cap);
  } else {               // ... or as a second set of the arrays, swapped per depth
    h->ray_next.alloc(6 * cap);
    h->draw_next.alloc(cap); h->pid_next.alloc(cap); h->col_next.alloc(cap);
  }
  h->last_col.alloc(cap);
  h->rec.release();
  h->rec.alloc((uint64_t)rptdev::REC_FIELDS * rec_cols);
  h->rec_parent.alloc(rec_cols);
  h->shadow.release();
  h->shadow.alloc((uint64_t)nl * rptdev::SHADOW_FIELDS * cap);
  h->counters.alloc(2 * (2 + (size_t)nl)); // two sets (rpt_shade clears the other one) of: [0] next-depth paths, [1] hits, [2 + l] shadow rays queued for light l
  h->shadow_q.release();
  h->shadow_q.alloc((uint64_t)nl * cap); // per light: the paths that cast a shadow ray towards it at the current depth
  h->srt.release();
  h->srt.alloc((uint64_t)nl * cap);      // per light and path: record.time of the shadow ray (rpt_shadow_sum reads it)
  if (h->has_deep) {
    h->tq.alloc(3 * cap); // a tree's ray queue | its rays with a zero direction component | those handed to the general form
    h->tq_ctr.alloc(16); // two sets of a tree's five counters, eight words apart (launch_query, QueryTuning::ctr_set)
    { // the traversal grid's stack spill area: one column per thread, as high as the scene's deepest tree (at least KD_MAX_STACK) less the LDS levels
      const uint64_t threads = (uint64_t)std::max(1, h->num_cus * 4) / 4 * RPT_TT_WAVES * 256;
      const uint64_t levels = (uint64_t)(std::max<uint32_t>((uint32_t)rptdev::KD_MAX_STACK, h->max_tree_depth + 1u) - RPT_TT_LEVELS_MIN);
      h->spill_node.alloc(levels * threads); h->spill_ts.alloc(levels * threads); h->spill_bmax.alloc(levels * threads);
      h->tree_rays.alloc(8 * cap); // one 64-byte row per position of a query: the rays that enter a tree (StackSpill::rays)
      h->spill = StackSpill{h->spill_node.p, h->spill_ts.p, h->spill_bmax.p, (uint32_t)threads, zeros_common(h->host_lights),
                            h->tree_rays.p};
    }
    ensure_generic(h, h->gen_all);
    if (h->sort_rays) ensure_sort_bufs(h, cap);
  }
  if (h->path_reorder) { // the per-depth re-order of the paths (in-kernel-traversal scenes): keys, positions, rocPRIM's scratch
    h->path_order.alloc(cap);
    ensure_sort_bufs(h, cap);
  }
  h->ws_cap = cap;
  h->ws_rec_cols = rec_cols;
  h->ws_stale = false;
}

// -DRPT_PROF builds (kernels/prof.inc): per phase, the share of the waves' time, the lanes that were active while it
// ran (lane time / wave time, of 64), and for loop bodies the iteration count and the lanes per iteration.  One line
// per slot that was used, machine-readable enough to be committed under profiles/ as it is.
void print_prof(const KernelTable* kt, const char* what) {
  static const char* const NAMES[30] = {
      "tree_trace refill", "tree_trace node steps", "tree_trace box tests", "tree_trace pop", "tree_trace write-out",
      "tree_trace exact tests", "in-kernel node step", "in-kernel box batch", "in-kernel child test",
      "in-kernel triangle batch", "in-kernel object", "paths fetch", "paths raygen", "paths closest_hit",
      "paths illuminate", "paths visible", "paths nee_bsdf", "paths sample_f", "paths bsdf", "paths record",
      "paths fold+store", "flat candidate walk", "fold iteration", "rejection round", "paths fused query",
      "paths draws", "paths shade block", "pre-trace pass", "pre-trace pass, cubes skipped",
      "fused query, shadow leaf test"};
  unsigned long long t[4][30];
  if (!kt->read_prof(t)) return;
  unsigned long long tot = 0;
  for (int i = 0; i < 30; i++) tot += t[0][i];
  std::fprintf(stderr, "prof[%s] %-28s %8s %10s %14s %10s\n", what, "phase", "time %", "lanes/64", "iterations", "lanes/64");
  for (int i = 0; i < 30; i++) {
    if (!t[0][i] && !t[2][i]) continue;
    char a[32] = "-", b[32] = "-", c[32] = "-", d[32] = "-";
    if (t[0][i]) {
      std::snprintf(a, sizeof a, "%.2f", tot ? 100.0 * (double)t[0][i] / (double)tot : 0.0);
      std::snprintf(b, sizeof b, "%.1f", (double)t[1][i] / (double)t[0][i]);
    }
    if (t[2][i]) {
      std::snprintf(c, sizeof c, "%llu", t[2][i]);
      std::snprintf(d, sizeof d, "%.1f", (double)t[3][i] / (double)t[2][i]);
    }
    std::fprintf(stderr, "prof[%s] %-28s %8s %10s %14s %10s\n", what, NAMES[i], a, b, c, d);
  }
}

void release_workspace(rptgpu_scene* h) {
  h->ray.release(); h->ray_next.release(); h->hit.release(); h->hit_obj.release(); h->draw.release(); h->draw_next.release();
  h->pid.release(); h->pid_next.release(); h->col.release(); h->col_next.release(); h->rec.release();
  h->rec_parent.release(); h->last_col.release();
  h->shadow.release(); h->tq.release(); h->srt.release(); h->shadow_q.release();
  h->sort_kin.release(); h->sort_kout.release(); h->sort_vin.release(); h->sort_tmp.release(); h->tree_rays.release();
  h->path_order.release(); h->next_rows.release();
  h->gen_defer.release(); h->gen_frame.release(); h->gen_threads = 0; // rpt_tree_generic's columns (ensure_generic makes them again)
  h->ws_cap = 0; h->ws_rec_cols = 0;
}

rptplan::PassPlan size_pass(rptgpu_scene* h, const rptplan::PassInput& in, uint32_t npix, bool generic_all) {
  rptplan::PassPlan pp = rptplan::plan_pass(in);
  for (;;) {
    const uint64_t np = rptplan::pass_slots(npix, pp);
    try {
      ensure_workspace(h, np, rptplan::pass_rec_cols(np, in.ratio));
      if (generic_all) ensure_generic(h, true);
      return pp;
    } catch (const HipError& e) {
      if (e.e != hipErrorOutOfMemory || pp.s_chunk == 1) throw;
      (void)hipGetLastError(); // clear the sticky error before retrying
      release_workspace(h);
      h->ws_fail_paths = rptplan::fail_paths_after_oom(h->ws_fail_paths, np);
      pp = rptplan::shrink_after_oom(pp);
    }
  }
}

void reset_tree_counters(rptgpu_scene* h) {
  HIP_TRY(hipMemsetAsync(h->tq_ctr.p, 0, 16 * sizeof(uint32_t), h->stream));
  h->qtune.ctr_set = 0;
}
static void tree_query(rptgpu_scene* h, const KernelTable* kt, const rptdev::PathState& ps, const uint32_t* queue, uint32_t n,
                       int light, double* srt, const uint32_t* d_n, const QueryHook* hook) {
  kt->query(h->stream, h->dscene, ps, queue, n, light, srt, d_n, h->obj_deep.data(), h->obj_tris.data(), h->dscene.num_objects,
            h->tq.p, h->tq_ctr.p, (uint32_t)std::max(1, h->num_cus * 4), h->sort_rays ? &h->sort_bufs : nullptr, hook, &h->spill,
            &h->qtune);
}
void query_closest(rptgpu_scene* h, const KernelTable* kt, const rptdev::PathState& ps, uint32_t n, const QueryHook* hook) {
  tree_query(h, kt, ps, nullptr, n, -1, nullptr, nullptr, hook);
}
void query_visibility(rptgpu_scene* h, const KernelTable* kt, const rptdev::PathState& ps, int l, uint32_t n,
                      const uint32_t* d_n, const QueryHook* hook) {
  tree_query(h, kt, ps, h->shadow_q.p + (uint64_t)l * ps.cap, n, l, h->srt.p, d_n, hook);
}

rptdev::Camera make_camera(const RptCamera& c) {
  // Camera::cast_ray derives d and right on every call (camera.rs:66-67); they are constants
  // of the batch, so they are computed once here with the same expressions.
  rptdev::Camera d{};
  std::memcpy(d.eye, c.eye, sizeof d.eye);
  std::memcpy(d.direction, c.direction, sizeof d.direction);
  std::memcpy(d.up, c.up, sizeof d.up);
  d.d = 1.0 / std::tan(c.fov / 2.0);
  const double* a = c.direction;
  const double* b = c.up;
  double cr[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  double len = std::sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
  for (int k = 0; k < 3; k++) d.right[k] = cr[k] / len;
  d.aperture = c.aperture;
  d.focal_distance = c.focal_distance;
  return d;
}

// what is wrong with a batch's parameters (nullptr: nothing) — the same answer on every rank of a multi-GPU job
const char* bad_params(const RptRenderParams* p) {
  if (!p->width || !p->height || !p->iterations) return "width, height and iterations must be non-zero";
  if (p->max_bounces > 254) return "max_bounces > 254";
  if ((uint64_t)p->width * p->height >= (1ull << 31)) return "frame too large";
  if (p->part_count && p->part_index >= p->part_count) return "part_index >= part_count";
  if (p->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  return nullptr;
}

// the device's free memory in bytes (-1: the runtime cannot say)
int64_t free_memory() {
  size_t free_b = 0, total_b = 0;
  return hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (int64_t)free_b : -1;
}

// the wavefront pipeline's view of the workspace
rptdev::PathState path_state(rptgpu_scene* h) {
  rptdev::PathState ps{};
  ps.ray = h->ray.p; ps.hit = h->hit.p; ps.hit_obj = h->hit_obj.p; ps.draw = h->draw.p;
  ps.pid = h->pid.p; ps.col = h->col.p;
  ps.ray_next = h->ray_next.p; ps.draw_next = h->draw_next.p; ps.pid_next = h->pid_next.p; ps.col_next = h->col_next.p;
  ps.rec = h->rec.p; ps.rec_parent = h->rec_parent.p; ps.last_col = h->last_col.p;
  ps.shadow = h->shadow.p; ps.cap = h->ws_cap; ps.rec_cap = h->ws_rec_cols;
  if (h->path_reorder) { // (never with per-tree queues: scene_plan.h fold_routes)
    ps.sort_keys = h->sort_kin.p; ps.sort_vals = h->sort_vin.p; ps.next_rows = h->next_rows.p;
    std::memcpy(ps.key_bounds, h->scene_bounds, sizeof ps.key_bounds);
  }
  return ps;
}

// the form of the persistent kernel that runs src (RaySource says which fields name which source), and what
// render_persistent does differently for it
static int paths_form(const RaySource& src) {
  if (src.views) return RPT_PATHS_FORM_VIEWS;
  if (src.cam || !src.origins) return RPT_PATHS_FORM_CAMERA;
  return src.probe < 0 && src.vertices ? RPT_PATHS_FORM_VERTICES : RPT_PATHS_FORM_RAYS;
}
struct PathsFormProps {
  const char* kname;
  bool fused_forms; // the kernel has the fused query and the hit pool where the layout offers them
  bool cull_rects;  // its rays are one camera's: the pre-trace pass gets that camera's screen rectangles
  bool piece;       // fr is a piece its caller cut to the work counter: checked here
  bool probes;      // src.probe >= 0 means light probes
};
static constexpr PathsFormProps PATHS_FORM_PROPS[RPT_PATHS_FORM_COUNT] = {
    {"rpt_paths", true, true, false, false},
    {"rpt_paths_views", true, false, true, false},
    {"rpt_paths_rays", true, false, true, true},
    // (the plain hand-out only: neither the fused query nor the pool, whatever the layout offers)
    {"rpt_paths_vertices", false, false, true, false}};

// the default pipeline: one persistent kernel, the whole path in registers; the batch runs as launches of at most
// spp_l samples per pixel (rptplan::plan_persistent) of the form src asks for — fr is the frame, or the piece of a call's
// views, rays or probes with its ids in fr.pixels (api_views.cpp, api_rays.cpp) — with rpt_sum_samples behind each and
// rpt_finish at the end.  Probes project each launch's samples into the piece's running sums with rpt_project_probes where
// rpt_sum_samples stands and end with rpt_finish_probes; a vertex sink's s_first is set per launch, as run_pass sets it per pass
void render_persistent(rptgpu_scene* h, const KernelTable* kt, const RptRenderParams& p, rptdev::Frame fr,
                       const RaySource& src, void* out, bool out_f32, bool packed, bool prof) {
  hipStream_t st = h->stream;
  const uint32_t npix = fr.npix;
  const PathsForm& form = kt->paths[paths_form(src)];
  const PathsFormProps& fp = PATHS_FORM_PROPS[paths_form(src)];
  const char* const kname = fp.kname;
  const bool probes = fp.probes && src.probe >= 0;
  const bool fused_forms = fp.fused_forms;
  // the launches' rays, whichever the form reads
  const rptdev::CallerRays cr{src.origins, src.dirs, src.first_draw, probes ? (int32_t)src.probe : -1};
  rptdev::VertexOut vo = src.vertices ? *src.vertices : rptdev::VertexOut{};
  rptdev::ViewRays vr{};
  if (src.views) {
    const uint64_t v0 = src.view_base / ((uint64_t)src.view_width * src.view_height); // the piece's first view
    vr = rptdev::ViewRays{src.views + v0, src.view_seeds + v0, src.view_of, src.view_width, src.view_height};
  }
  const PathsRays from{src.cam, &vr, &cr, &vo};
  const bool print_launch = std::getenv("RPTGPU_PRINT_LAUNCH") != nullptr;
  const uint64_t lbuf_held = h->lbuf.n * sizeof(double);
  const int64_t free_b = lbuf_held < h->opt.lbuf_bytes ? free_memory() : -1;
  const bool flat = h->all_flat && !h->dscene.force_general;
  FlatLayout lay = flat ? h->flat_layout : FlatLayout{};
  const uint32_t flat_lds = lay.off_end;
  // the fused kernel's pre-trace pass: this render's screen rectangles of the objects it may skip (host_scene.cpp
  // pinhole_screen_rect; none under a lens).  An object without a rectangle is always tested.  A piece of views gets none
  // (cull_n = 0: every test runs — the rectangles are one camera's), and so does a piece of the caller's rays
  if (RPT_PRETRACE_CULL && lay.pretrace_cull && fp.cull_rects) {
    const rptdev::Camera& cam = *src.cam;
    for (size_t i = 0; i < h->obj_geom.size() && i < 64 && lay.cull_n < (uint32_t)RPT_CULL_MAX; i++) {
      uint32_t r[4];
      if (((lay.cull_always >> i) & 1ull) ||
          !rpthost::pinhole_screen_rect(rpthost::world_box(h->obj_geom[i], h->top_insts[i]), cam, fr.width, fr.height, r))
        continue;
      lay.cull_obj[lay.cull_n] = (uint32_t)i;
      const bool off = r[0] > r[1] || r[2] > r[3]; // off screen
      lay.cull_lo[lay.cull_n] = off ? 0xffffffffu : (r[0] | (r[2] << 16));
      lay.cull_ext[lay.cull_n] = off ? 0u : ((r[1] - r[0]) | ((r[3] - r[2]) << 16));
      lay.cull_n++;
    }
  }
  const rptplan::PersistentPlan pl = rptplan::plan_persistent(
      npix, p.iterations, p.max_bounces, h->num_cus, form.max_blocks_per_cu(flat ? &lay : nullptr, flat_lds, false),
      h->opt.lbuf_bytes, lbuf_held, free_b, h->opt.paths_chunk, h->all_flat, h->dscene.force_general, h->flat_layout.obj_filter);
  // a texture environment: the lanes park their lookups in what the wave's LDS share has left (kernels/paths.inc) —
  // unless that costs a resident wave (a flat scene that fills the share)
  bool park = flat && h->opt.env_park != 0 && h->dscene.env_kind != RPT_ENV_COLOR; // (flat scenes: rpt_paths<KdLds>'s stack fills the share)
  if (park && form.max_blocks_per_cu(&lay, flat_lds, true) < pl.per_cu) park = false;
  // (a piece: its caller cut it so that every launch fits the work counter — persistent_piece, api_internal.h)
  if (fp.piece && rptplan::views_items(npix, pl.spp_l, pl.chunk, pl.nblocks, RPT_PATHS_BATCH_MAX).capped)
    throw std::runtime_error(std::string(kname) + ": the piece's work items do not fit the 32-bit work counter (internal error)");
  h->prec.alloc((uint64_t)rpt_fold_ring_slots(p.max_bounces) * rptdev::REC_FIELDS * ((uint64_t)pl.nblocks * 64));
  h->lbuf.alloc(std::max<uint64_t>(1, (uint64_t)pl.spp_l * 3 * npix));
  if (print_launch)
    std::fprintf(stderr, "%s<%s>: %d blocks/CU x %d CUs -> %u blocks, %u samples per work item, %u launch(es) of %u spp, "
                 "dynamic LDS %u B per wave (the flat scene's tables)%s%s%s%s\n",
                 kname, flat ? (lay.obj_filter ? "KdFlatF" : lay.n_tris ? "KdFlat" : "KdFlatG") : "KdLds", pl.per_cu, h->num_cus, pl.nblocks,
                 pl.chunk, pl.n_launch, pl.spp_l, flat_lds, park ? " + parked environment lookups" : "",
                 fused_forms && flat && lay.n_tris && lay.fuse_query && !park ? ", shadow and bounce rays in one query" : "",
                 fused_forms && flat && lay.n_tris && lay.fuse_query && !park && lay.scene_consts ? ", a hit's scene constants from the wave's tables" : "",
                 fused_forms && RPT_HIT_POOL && flat && lay.n_tris && lay.fuse_query && !park ? ", pre-traced hits in a wave-level pool" : "");
  h->counters.alloc(4);
  h->pcounters.alloc(16);
  HIP_TRY(hipMemsetAsync(h->pcounters.p, 0, 16 * sizeof(unsigned long long), st));
  // probes: the piece's running sums start at zero, as render_wavefront starts them (rpt_project_probes continues them)
  if (probes) HIP_TRY(hipMemsetAsync(h->accum.p, 0, (uint64_t)npix * probe_width((uint32_t)src.probe) * sizeof(double), st));
  for (uint32_t s0 = 0; s0 < p.iterations; s0 += pl.spp_l) {
    const uint32_t spp = std::min(pl.spp_l, p.iterations - s0);
    const uint64_t items = rptplan::work_items(npix, spp, pl.chunk);
    fr.sample_base = p.sample_index_base + s0;
    HIP_TRY(hipMemsetAsync(h->counters.p, 0, sizeof(uint32_t), st));
    { Bracket b(h, RPT_K_PATHS, prof);
      vo.s_first = s0; // (the launch's first sample, counted from the call's)
      form.launch(st, h->dscene, fr, from,
                  PathsLaunch{h->counters.p, h->prec.p, h->pcounters.p, h->lbuf.p, spp, pl.chunk, (uint32_t)items, pl.nblocks, &lay, flat,
                              flat_lds, park, h->opt.paths_batch});
      b.done(); }
    if (probes) kt->project_probes(st, fr, h->lbuf.p, spp, (uint32_t)src.probe);
    else kt->sum_samples(st, fr, h->lbuf.p, spp, s0 == 0);
    if (print_launch) { // diagnostics: where the 32-bit work counter ended (kernels/paths.inc fetch_item)
      uint32_t ended = 0;
      HIP_TRY(hipMemcpyAsync(&ended, h->counters.p, sizeof ended, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const uint32_t batch_used = h->opt.paths_batch ? std::min<uint32_t>(h->opt.paths_batch, RPT_PATHS_BATCH_MAX)
                                                      : std::min(256u, std::max((uint32_t)items / (std::max(1u, pl.nblocks) * 32u), 16u));
      std::fprintf(stderr, "rpt_paths work counter: ended at %u for %llu items; %u waves, claims of at most %u: dead claims %lld of at most %llu\n",
                   ended, (unsigned long long)items, pl.nblocks, batch_used, (long long)ended - (long long)items,
                   (unsigned long long)pl.nblocks * (64u + batch_used));
    }
  }
  HIP_TRY(hipGetLastError());
  if (probes) kt->finish_probes(st, fr, probe_width((uint32_t)src.probe), src.probe_scale, (double*)out);
  else kt->finish(st, fr, (double)p.iterations, std::pow(2.0, p.exposure_value), out, out_f32, packed);
  unsigned long long rc[16] = {0};
  HIP_TRY(hipMemcpyAsync(rc, h->pcounters.p, sizeof rc, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (std::getenv("RPTGPU_PRINT_PHASES")) print_prof(kt, kname);
  h->stats.samples += (uint64_t)npix * p.iterations;
  h->stats.extend_rays += rc[0];
  h->stats.shadow_rays += rc[1];
  h->stats.shadow_rays_traced += rc[1]; // the persistent kernel traces every shadow ray (a skip there saves no wave time)
}

// One pass of the wavefront pipeline over n_paths = npix x spp paths: the ray source's kernel (rpt_raygen for a camera's
// pixels, rpt_raygen_rays for a piece of the caller's rays, rpt_raygen_probes for a piece of light probes, rpt_raygen_views
// for a piece of a batch of views — with a seed per view: rpt_raygen_views_seeded, and rpt_shade_seeded for rpt_shade), per depth {
// closest-hit query, rpt_shade, the visibility queries, rpt_shadow_sum }, rpt_resolve (probes: rpt_resolve_probes).  *cols: the record columns the pass used.  false: the
// pool ran out at some depth (*cols: the columns up to and with that depth) — the pass did not resolve, and nothing of it
// has left the workspace.
bool run_pass(rptgpu_scene* h, const KernelTable* kt, const RptRenderParams& p, const rptdev::Frame& fr,
              const RaySource& src, uint32_t n_paths, uint32_t spp, bool prof, const QueryHook& qhook, uint64_t* cols) {
  hipStream_t st = h->stream;
  rptdev::PathState ps = path_state(h);
  const int nlights = h->dscene.num_lights;
  const uint32_t nctr = 2u + (uint32_t)nlights;
  // the counter sets the kernels clear for each other start cleared (one memset per pass, not one per depth and
  // per tree and query: 102 of the wine glass's 354 fills per step)
  HIP_TRY(hipMemsetAsync(h->counters.p, 0, 2 * (size_t)nctr * sizeof(uint32_t), st));
  uint32_t cset = 0;
  if (h->has_deep) reset_tree_counters(h);
  rptdev::VertexOut vertices{}; // (rptgpu_trace_vertices only) the sink with this pass's first sample, counted from the call's
  if (src.vertices) {
    vertices = *src.vertices;
    vertices.s_first = (uint32_t)(fr.sample_base - p.sample_index_base);
  }
  if (src.views && src.view_seeds) {
    // one launch for every view the piece holds: the raygen count of RptStats stays at least the number of views rendered
    // under seeds of their own, as it was when such a view was a piece — the depth loop behind it is the piece's, shared
    const uint64_t npix_view = (uint64_t)src.view_width * src.view_height;
    for (uint32_t p_lo = 0, p_len; p_lo < fr.npix; p_lo += p_len) {
      const uint64_t j = src.view_base + p_lo;
      p_len = (uint32_t)std::min<uint64_t>(fr.npix - p_lo, (j / npix_view + 1) * npix_view - j);
      Bracket b(h, RPT_K_RAYGEN, prof);
      kt->raygen_views_seeded(st, fr, src.views, src.view_width, src.view_height, src.view_base, src.ids_out, src.view_seeds,
                              src.seeds_out, p_lo, p_len, ps, p_len * spp);
      b.done();
    }
  } else { Bracket b(h, RPT_K_RAYGEN, prof);
    if (src.cam) kt->raygen(st, fr, *src.cam, ps, n_paths);
    else if (src.views) kt->raygen_views(st, fr, src.views, src.view_width, src.view_height, src.view_base, src.ids_out, ps, n_paths);
    else if (src.probe >= 0) kt->raygen_probes(st, fr, src.origins, src.dirs, (uint32_t)src.probe, src.ids_out, src.id_base, ps, n_paths);
    else kt->raygen_rays(st, fr, src.origins, src.dirs, src.first_draw, src.ids_out, src.id_base, ps, n_paths);
    b.done(); }
  h->stats.samples += n_paths;
  uint32_t n_active = n_paths;
  const uint32_t* const queue = nullptr; // the paths of a depth stand densely in its state arrays: the identity
  uint32_t* const next = nullptr;
  uint64_t rec_off = 0; // the depth's first record column
  // per-tree queries for scenes with deep trees; under RPT_FLAG_GENERAL_TRAVERSAL the whole scene is walked
  // in-kernel in the general form — unless it has a group with tree children, which only the per-tree pipeline
  // walks (there the flag sends every ray of every such object through rpt_tree_generic)
  const bool by_object = h->has_deep && (!(p.flags & RPT_FLAG_GENERAL_TRAVERSAL) || h->tree_kids);
  for (uint32_t depth = 0; depth <= p.max_bounces && n_active; depth++) {
    if (rec_off + n_active > h->ws_rec_cols) {
      *cols = rec_off + n_active;
      return false;
    }
    { Bracket b(h, RPT_K_EXTEND, prof);
      if (by_object)
        query_closest(h, kt, ps, n_active, &qhook);
      else
        kt->extend(st, h->dscene, ps, queue, n_active);
      b.done(); }
    // rptgpu_trace_vertices: the depth's hits and rays into the caller's arrays while the rays still are the ones the query
    // ran for (rpt_shade puts the hit position where the origin is).  A pass that starts over writes the same entries again
    if (src.vertices) kt->vertices_store(st, fr, ps, n_active, depth, vertices);
    h->stats.extend_rays += n_active;
    uint32_t* const ctrs = h->counters.p + (size_t)cset * nctr;       // this depth's counters (cleared by the depth before)
    uint32_t* const ctrs_next = h->counters.p + (size_t)(cset ^ 1u) * nctr;
    cset ^= 1u;
    { Bracket b(h, RPT_K_SHADE, prof);
      if (src.view_seeds) kt->shade_seeded(st, h->dscene, fr, ps, queue, n_active, depth, next, ctrs, h->shadow_q.p, ctrs_next, nctr, (uint32_t)rec_off, src.seeds_out);
      else kt->shade(st, h->dscene, fr, ps, queue, n_active, depth, next, ctrs, h->shadow_q.p, ctrs_next, nctr, (uint32_t)rec_off);
      b.done(); }
    // The depth's counts come back right after rpt_shade — the one point of a depth where the host waits — so the
    // visibility queries are sized for the shadow rays there ARE (50-70 % of the paths on closed meshes: less to
    // sort, smaller grids, and a light without a single ray at this depth costs no launch at all) and the next
    // depth for its survivors.  Until round 5 the wait stood at the depth's end and the queries ran over the
    // host's bound, the number of paths.  Everything up to the next rpt_shade is then enqueued without a wait.
    h->cnt_host.resize(2 + (size_t)nlights);
    uint32_t* cnt = h->cnt_host.data();
    HIP_TRY(hipMemcpyAsync(cnt, ctrs, (2 + (size_t)nlights) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int l = 0; l < nlights; l++) h->stats.shadow_rays_traced += cnt[2 + l];
    if (prof && h->pending.size() >= 256) drain_events(h); // the stream is idle here: cheap
    h->stats.shadow_rays += (uint64_t)cnt[1] * (uint64_t)h->dscene.num_shadow_lights;
    if (nlights > 0) {
      // the visibility queries run over rpt_shade's per-light shadow-ray queues (their lengths also stay on the
      // device: ctrs + 2 + l is what the kernels read)
      Bracket b(h, RPT_K_SHADOW, prof);
      if (by_object) {
        for (int l = 0; l < nlights; l++)
          if (h->light_casts[l] && cnt[2 + l]) query_visibility(h, kt, ps, l, cnt[2 + l], ctrs + 2 + l, &qhook);
      } else { // one launch for all lights of the depth (the grid's y is the light)
        uint32_t n_max = 0;
        for (int l = 0; l < nlights; l++)
          if (h->light_casts[l]) n_max = std::max(n_max, cnt[2 + l]);
        if (n_max) kt->shadow_rays(st, h->dscene, ps, h->shadow_q.p, ctrs + 2, n_max, nlights, h->srt.p);
      }
      kt->shadow_sum(st, h->dscene, ps, queue, n_active, (uint32_t)rec_off, h->srt.p);
      b.done();
    }
    rec_off += n_active;
    n_active = cnt[0];
    // the survivors' state is what rpt_shade wrote to the *_next arrays at their new positions
    if (h->path_reorder) {
      // ... as rows, gathered into the current arrays in the order of their rays' keys — or, a depth too small to be
      // worth a sort, as they stand (behind the depth's shadow queries, which read the current arrays: same stream)
      if (n_active && depth < p.max_bounces) {
        Bracket b(h, RPT_K_TREE_SORT, prof);
        kt->path_reorder(st, ps, n_active, n_active >= h->path_reorder_min, &h->sort_bufs, h->path_order.p);
        b.done();
      }
    } else {
      std::swap(ps.ray, ps.ray_next); std::swap(ps.draw, ps.draw_next); std::swap(ps.pid, ps.pid_next); std::swap(ps.col, ps.col_next);
    }
  }
  // ... and, now that every path of the pass has ended (last_col is final), what the records hold of each and the filler
  if (src.vertices) kt->vertices_fold(st, fr, ps, n_paths, vertices);
  { Bracket b(h, RPT_K_RESOLVE, prof);
    if (src.probe >= 0) kt->resolve_probes(st, fr, ps, spp, (uint32_t)src.probe);
    else kt->resolve(st, fr, ps, spp);
    b.done(); }
  HIP_TRY(hipGetLastError()); // a failed launch is reported here, not by the stream sync
  *cols = rec_off;
  return true;
}

// what the passes of a call over npix pixels (or rays) have in common ...
rptplan::PassInput pass_input(rptgpu_scene* h, uint32_t npix, uint32_t iterations) {
  rptplan::PassInput in{};
  in.npix = npix; in.iterations = iterations;
  in.per_slot = rptplan::wavefront_slot_bytes(h->dscene.num_lights, h->has_deep, h->sort_rays, h->path_reorder);
  in.target_paths = h->opt.target_paths; in.budget_bytes = h->opt.workspace_bytes;
  // the share of the free memory a pass may take (round 6: 85 %, was 1/2 — the passes of a 288 GB device were
  // sized for 140 GB).  RPTGPU_WS_FREE_FRACTION (percent): experiments only
  in.free_percent = RPT_WS_FREE_PERCENT;
  if (const char* e = std::getenv("RPTGPU_WS_FREE_FRACTION")) in.free_percent = (uint64_t)std::min(95, std::max(5, std::atoi(e)));
  return in;
}
// ... and what the device and the handle hold right now
void pass_input_now(rptgpu_scene* h, rptplan::PassInput& in) {
  in.free_bytes = in.target_paths ? -1 : free_memory();
  in.held_slots = h->ws_cap; in.held_cols = h->ws_rec_cols; // (what the handle holds counts as available)
  in.fail_paths = h->ws_fail_paths;
}

// scenes with deep trees (and RPT_FLAG_WAVEFRONT): the batch runs as passes of many paths in flight, each sized by
// rptplan::plan_pass; a pass changes nothing outside the workspace before its rpt_resolve.  Of p it reads iterations,
// max_bounces, sample_index_base, exposure_value and flags (the calls over pieces fill in little more: piece_params)
void render_wavefront(rptgpu_scene* h, const KernelTable* kt, const RptRenderParams& p, rptdev::Frame fr,
                      const RaySource& src, void* out, bool out_f32, bool packed, bool prof) {
  hipStream_t st = h->stream;
  const uint32_t npix = fr.npix;
  const bool print_launch = std::getenv("RPTGPU_PRINT_LAUNCH") != nullptr;
  if (h->rec_ratio_bounces != p.max_bounces) {
    h->rec_ratio = 0.0; h->rec_ratio_bounces = p.max_bounces;
    // tests: start from a given (too small) figure instead of measuring, so that passes run out of columns and start over
    if (const char* e = std::getenv("RPTGPU_REC_RATIO")) h->rec_ratio = std::max(0.0, std::atof(e));
  }
  rptplan::PassInput in = pass_input(h, npix, p.iterations);
  // (rpt_tree_generic's large grid — whole objects, or under RPT_FLAG_GENERAL_TRAVERSAL everything, go through it: up to
  // several hundred MB of columns for a deep mesh — is part of a pass's workspace: if it does not fit, the pass shrinks)
  const bool generic_all = h->has_deep && (h->gen_all || h->dscene.force_general);
  const uint32_t acc_w = src.probe >= 0 ? probe_width((uint32_t)src.probe) : 3u; // running sums per pixel, ray or probe
  HIP_TRY(hipMemsetAsync(h->accum.p, 0, (uint64_t)npix * acc_w * sizeof(double), st));
  QueryMarks qm(h, prof);
  const QueryHook qhook{query_mark, &qm};

  for (uint32_t s0 = 0; s0 < p.iterations;) {
    in.remaining = p.iterations - s0;
    in.rec_ratio = h->rec_ratio;
    in.ratio = rptplan::pass_ratio(h->rec_ratio, p.max_bounces);
    pass_input_now(h, in);
    const rptplan::PassPlan pp = size_pass(h, in, npix, generic_all);
    const uint32_t n_paths = npix * pp.s_chunk;
    fr.sample_base = p.sample_index_base + s0;
    const RptStats stats_at_start = h->stats; // (a pass that is started over counts once)
    uint64_t cols = 0;
    if (!run_pass(h, kt, p, fr, src, n_paths, pp.s_chunk, prof, qhook, &cols)) {
      // more levels per path than the pool was sized for (another camera, a margin too thin): the pass starts over
      // with room for half as many paths again per column budget; nothing of it has left the workspace
      HIP_TRY(hipStreamSynchronize(st));
      h->stats = stats_at_start;
      h->rec_ratio = rptplan::ratio_after_restart(h->rec_ratio, cols, n_paths, p.max_bounces);
      if (print_launch)
        std::fprintf(stderr, "wavefront pass of %u spp started over: the record pool (%.2f columns per path) ran out; now %.2f\n", pp.s_chunk, in.ratio, h->rec_ratio);
      continue;
    }
    h->rec_ratio = rptplan::ratio_after_pass(h->rec_ratio, cols, n_paths);
    if (print_launch)
      std::fprintf(stderr, "wavefront pass: %u spp, %u paths, %llu record columns used of %llu (%.3f per path, pool sized for %.3f)\n",
                   pp.s_chunk, n_paths, (unsigned long long)cols, (unsigned long long)h->ws_rec_cols, (double)cols / (double)n_paths, in.ratio);
    s0 += pp.s_chunk;
  }
  if (src.probe >= 0) kt->finish_probes(st, fr, acc_w, src.probe_scale, (double*)out);
  else kt->finish(st, fr, (double)p.iterations, std::pow(2.0, p.exposure_value), out, out_f32, packed);
  if (std::getenv("RPTGPU_PRINT_PHASES")) {
    HIP_TRY(hipStreamSynchronize(st));
    print_prof(kt, "wavefront");
  }
}

// packed (with d_out, f32 or f64): d_out receives only this part's pixels, [npix][3] in the order of the part's pixel list;
// d_list: the n_list pixels of that list instead (the partition cache h->pixels / h->npix / h->part_key stays as it is)
int render_impl(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* p, void* d_out, bool out_f32,
                double* host_out, hipStream_t user_stream, bool packed, const uint32_t* d_list, uint32_t n_list) {
  if (!h || !camera || !p) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  REFUSE_IF_ABANDONED(h);
  if (const char* why = bad_params(p)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (d_list && (!packed || !d_out || host_out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "a pixel list renders packed into device memory");
  // (the frame gets no caller's stream: the partition and the frame's array are made first, and the body waits itself)
  return device_call(h, nullptr, [&]() {
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(p->precision_mode, h->ext_shapes);
    const bool prof = (p->flags & RPT_FLAG_PROFILE_KERNELS) != 0;
    if (!d_list) ensure_partition(h, *p);
    const uint32_t npix = d_list ? n_list : h->npix;
    const uint64_t frame_elems = (uint64_t)p->width * p->height * 3;
    const size_t out_elem = out_f32 ? sizeof(float) : sizeof(double);
    void* out = d_out;
    if (!out) {
      h->out_full.alloc(frame_elems);
      out = h->out_full.p;
    }
    if (user_stream) HIP_TRY(hipStreamSynchronize(user_stream));
    if (!packed) HIP_TRY(hipMemsetAsync(out, 0, frame_elems * out_elem, st));
    const bool wavefront = use_wavefront(h, p->flags, h->prefer_wavefront);
    h->dscene.force_general = (p->flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
    if (npix) {
      h->accum.alloc((uint64_t)npix * 3);
      rptdev::Frame fr{};
      fr.width = p->width; fr.height = p->height; fr.npix = npix; fr.pixels = d_list ? d_list : h->pixels.p;
      fr.max_bounces = p->max_bounces; fr.seed = p->seed; fr.accum = h->accum.p;
      const rptdev::Camera cam = make_camera(*camera);
      RaySource src{};
      src.cam = &cam;
      if (wavefront) render_wavefront(h, kt, *p, fr, src, out, out_f32, packed, prof);
      else render_persistent(h, kt, *p, fr, src, out, out_f32, packed, prof);
    }
    HIP_TRY(hipGetLastError());
    if (host_out) HIP_TRY(hipMemcpyAsync(host_out, out, frame_elems * out_elem, hipMemcpyDeviceToHost, st));
    return wavefront && h->has_deep && h->gen_overflow.p;
  });
}

} // namespace rptapi

extern "C" {

int rptgpu_render_batch(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* params, double* out_rgb) {
  if (!out_rgb) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null out_rgb");
  return render_impl(h, camera, params, nullptr, false, out_rgb, nullptr);
}

int rptgpu_render_batch_device(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* params, void* d_out,
                               int out_is_f32, void* stream) {
  if (!d_out) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null d_out");
  return render_impl(h, camera, params, d_out, out_is_f32 != 0, nullptr, (hipStream_t)stream);
}

int rptgpu_closest_hit(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs,
                       uint32_t precision_mode, double* out_t, double* out_normal, int32_t* out_object) {
  if (!h || (n && (!origins || !dirs || !out_t || !out_normal || !out_object)))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (precision_mode != RPT_PRECISION_F64_STRICT) return fail(h, RPTGPU_E_INVALID_ARGUMENT, BAD_MODE);
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return guarded(h, h->device, [&]() -> int {
    hipStream_t st = h->stream;
    if (h->has_deep && (!h->opt.rays_in_kernel || h->tree_kids)) {
      // a scene with deep trees: the rays take the route a render's rays take — object by object, every deep tree with
      // its own queue, sort and persistent traversal (launch_query) — in pieces of at most 4 Mi rays
      const KernelTable* kt = table_for(precision_mode, h->ext_shapes);
      const uint64_t piece = std::min<uint64_t>(n, 4ull << 20);
      ensure_workspace(h, piece, piece);
      const rptdev::PathState ps = path_state(h);
      std::vector<double> soa(6 * piece), hit(4 * piece);
      for (uint64_t base = 0; base < n; base += piece) {
        const uint64_t m = std::min(piece, n - base);
        for (uint64_t i = 0; i < m; i++)
          for (int k = 0; k < 3; k++) {
            soa[(uint64_t)k * m + i] = origins[3 * (base + i) + k];
            soa[(uint64_t)(3 + k) * m + i] = dirs[3 * (base + i) + k];
          }
        for (int k = 0; k < 6; k++)
          HIP_TRY(hipMemcpyAsync(ps.ray + (uint64_t)k * ps.cap, soa.data() + (uint64_t)k * m, m * sizeof(double), hipMemcpyHostToDevice, st));
        reset_tree_counters(h);
        query_closest(h, kt, ps, (uint32_t)m, nullptr);
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < 4; k++)
          HIP_TRY(hipMemcpyAsync(hit.data() + (uint64_t)k * m, ps.hit + (uint64_t)k * ps.cap, m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_object + base, ps.hit_obj, m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < m; i++) {
          out_t[base + i] = hit[i];
          for (int k = 0; k < 3; k++) out_normal[3 * (base + i) + k] = hit[(uint64_t)(1 + k) * m + i];
        }
      }
      return drain_call(h, h->gen_overflow.p != nullptr);
    }
    DevBuf<double> d_o, d_d, d_t, d_n;
    DevBuf<int32_t> d_obj;
    d_o.alloc(3 * n); d_d.alloc(3 * n); d_t.alloc(n); d_n.alloc(3 * n); d_obj.alloc(n);
    HIP_TRY(hipMemcpyAsync(d_o.p, origins, 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_d.p, dirs, 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
    table_for(precision_mode, h->ext_shapes)->extend_rays(st, h->dscene, d_o.p, d_d.p, n, d_t.p, d_n.p, d_obj.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_t, d_t.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_normal, d_n.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_object, d_obj.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RPTGPU_OK;
  });
}

int rptgpu_eval_math(rptgpu_scene* h, int fn, uint64_t n, const double* x, const double* y, double* out) {
  if (!h || (n && (!x || !out)) || fn < 0 || fn > 13 || (fn >= 6 && fn <= 11 && n && !y))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "bad argument");
  if (!n) return RPTGPU_OK;
  if (fn >= 12) { // a hit's draws: an element whose rejection loops could not end is refused here
    for (uint64_t e = 0; e < n / 9; e++) {
      uint64_t w[9];
      memcpy(w, x + e * 9, sizeof w);
      double f;
      memcpy(&f, &w[6], sizeof f);
      if (w[1] > 0xFFFFFFFFull || w[3] > 0x7FFFFFFFull || !w[4] || w[4] > 0xFFFFFFFFull || w[5] < (1ull << 62) || !(f >= 0.0 && f <= 1.0) ||
          w[7] > 3ull)
        return fail(h, RPTGPU_E_INVALID_ARGUMENT, "bad argument");
    }
  }
  return guarded(h, h->device, [&]() -> int {
    DevBuf<double> dx, dy, dout;
    dx.alloc(n); dy.alloc(n); dout.alloc(n);
    HIP_TRY(hipMemcpyAsync(dx.p, x, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (y) HIP_TRY(hipMemcpyAsync(dy.p, y, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(hipMemsetAsync(dy.p, 0, n * sizeof(double), h->stream));
    rpt_strict::TABLE.eval_math(h->stream, fn, n, dx.p, dy.p, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RPTGPU_OK;
  });
}

} // extern "C"
