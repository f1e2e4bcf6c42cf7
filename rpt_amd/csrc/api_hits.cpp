// api_hits.cpp — rptgpu_first_hits[_device] and rptgpu_render_views_aov[_seeded][_device]: the first hit's record for the caller
// (include/rpt_gpu.h; see api_internal.h).  Both run ONE closest-hit query of a render per piece or pass —
// closest_hit<KdLdsW> inside a kernel for scenes walked in-kernel, query_closest for scenes with deep trees, chosen as
// render_wavefront's run_pass chooses — and carry its record into the caller's layout (kernels/hits.inc): the channels of a
// ray's record as they come (rpt_first_hits fused, or rpt_raygen_rays + the query + rpt_hits_store), or folded per (view,
// pixel) as rptgpu_render_aov folds them (rpt_raygen_views + the query + rpt_views_aov_fold, in passes over
// rptgpu_render_views' pieces).  No rpt_shade, no records, no shadow rays.  Pieces: rptplan::hits_piece / views_piece.
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t HIT_ALL = RPT_HIT_T | RPT_HIT_NORMAL | RPT_HIT_OBJECT | RPT_HIT_POSITION | RPT_HIT_ALBEDO;

// what is wrong with an RptHitQuery (nullptr: nothing)
static const char* bad_hit_query(const RptHitQuery* q) {
  if (const char* why = bad_channel_query(q, RPT_QUERY_TEXTS(RptHitQuery, RPT_HIT), HIT_ALL)) return why;
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; first hits run the closest-hit query only";
  return nullptr;
}

namespace {

// the kernels' struct from the arrays of rptplan::HIT_ROWS (a channel that is not named: nullptr, and not read)
rptdev::HitOut hit_out(const ChannelPtrs& p, uint32_t channels) {
  rptdev::HitOut ho{};
  ho.channels = channels;
  ho.t = p.at<double>(rptplan::HIT_R_T); ho.normal = p.at<double>(rptplan::HIT_R_NORMAL);
  ho.position = p.at<double>(rptplan::HIT_R_POSITION); ho.albedo = p.at<double>(rptplan::HIT_R_ALBEDO);
  ho.object = p.at<int32_t>(rptplan::HIT_R_OBJECT);
  return ho;
}

// (run_pass's decision: per-tree queries for scenes with deep trees — under RPT_FLAG_GENERAL_TRAVERSAL only where a group
// with tree children leaves no other walker)
bool query_by_object(const rptgpu_scene* h, uint32_t flags) {
  return h->has_deep && (!(flags & RPT_FLAG_GENERAL_TRAVERSAL) || h->tree_kids);
}

} // namespace

HitPieces plan_hit_pieces(rptgpu_scene* h, uint64_t n, uint32_t flags, const char* piece_env) {
  HitPieces hp{};
  h->dscene.force_general = (flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
  hp.by_object = query_by_object(h, flags);
  uint64_t bound = ~0ull; // the fused kernel touches no workspace
  if (hp.by_object) {
    rptplan::PassInput in = pass_input(h, 1, 1);
    in.remaining = 1;
    in.ratio = 1.0; // no depth follows the rays: one record column is all ensure_workspace is asked for
    pass_input_now(h, in);
    bound = rptplan::plan_pass(in).target;
  }
  uint64_t asked = 0; // tests: pieces of a few rays
  if (const char* e = std::getenv(piece_env)) asked = std::strtoull(e, nullptr, 10);
  hp.piece = rptplan::hits_piece(n, asked, bound);
  if (hp.by_object) {
    ensure_workspace(h, hp.piece, 1);
    if (h->gen_all || h->dscene.force_general) ensure_generic(h, true); // (as render_wavefront's size_pass)
    hp.ps = path_state(h);
  }
  return hp;
}

void hit_piece(rptgpu_scene* h, const KernelTable* kt, const HitPieces& hp, const double* d_o, const double* d_d, uint32_t m,
               const rptdev::HitOut& ho, bool prof) {
  hipStream_t st = h->stream;
  if (hp.by_object) {
    rptdev::Frame fr{};
    fr.width = m; fr.height = 1; fr.npix = m;
    kt->raygen_rays(st, fr, d_o, d_d, 0, nullptr, 0, hp.ps, m); // one sample: slot = the ray's position in the piece
    reset_tree_counters(h);
  }
  const int pair = event_pair_begin(h, RPT_K_EXTEND, prof);
  if (hp.by_object) query_closest(h, kt, hp.ps, m, nullptr);
  else kt->first_hits(st, h->dscene, d_o, d_d, m, ho);
  event_pair_end(h, RPT_K_EXTEND, pair);
  if (hp.by_object) kt->hits_store(st, h->dscene, hp.ps, m, ho);
  HIP_TRY(hipGetLastError());
}

namespace {

// on_device: origins, dirs and out's arrays are device pointers (user_stream: the stream their producer ran on)
int first_hits(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const RptHitQuery* q,
               const RptHitArrays* out, bool on_device, hipStream_t user_stream) {
  // (the query first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_hit_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_channel_arrays(out, RPT_ARRAYS_TEXTS(RptHitArrays), rptplan::HIT_ROWS, q->channels))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!origins || !dirs)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(q->precision_mode, h->ext_shapes);
    const bool prof = (q->flags & RPT_FLAG_PROFILE_KERNELS) != 0;
    const uint32_t ch = q->channels;
    const HitPieces hp = plan_hit_pieces(h, n, q->flags, "RPTGPU_HITS_PIECE");
    const uint64_t piece = hp.piece;
    ChannelPtrs stage{}; // a host caller's piece of records on the device
    if (!on_device) {
      h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece);
      const rptchan::Layout lay = rptchan::layout(rptplan::HIT_ROWS, ch, piece);
      h->hits_out.alloc(lay.words);
      stage = ptrs_in(h->hits_out.p, lay);
    }
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const double *d_o = origins + 3 * base, *d_d = dirs + 3 * base;
      const ChannelPtrs mine = ptrs_at(rptplan::HIT_ROWS, out, ch, base);
      if (!on_device) stage_rays(h, d_o, d_d, m);
      hit_piece(h, kt, hp, d_o, d_d, m, hit_out(on_device ? mine : stage, ch), prof);
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_out(rptplan::HIT_ROWS, stage, mine, ch, m, st);
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return h->has_deep && h->gen_overflow.p;
  });
}

} // namespace

// out's arrays: host memory, or — on_device — device memory (user_stream: the stream their producer ran on); views and the
// structs are host memory either way.  seeded: the _seeded entry points — view v's seed is seeds[v] (host memory), and
// q's seed and seed_stride are not read
int render_views_aov(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q, bool seeded,
                     const uint64_t* seeds, const RptAovBuffers* out, bool on_device, hipStream_t user_stream) {
  // (the query, the buffers, then the views: each is refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_view_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_aov(out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n_views && !views) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (seeded && n_views && !seeds) return fail(h, RPTGPU_E_INVALID_ARGUMENT, NULL_SEEDS);
  const uint64_t npix = (uint64_t)q->width * q->height;
  if (n_views > (1ull << 58) / npix) // (3 values of 8 bytes per index: an array's size in bytes fits 64 bits)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "n_views * width * height does not fit: the frames would not fit any memory");
  for (uint64_t v = 0; v < n_views; v++)
    if (const char* why = bad_view(views[v], *q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n_views) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(q->precision_mode, h->ext_shapes);
    const uint32_t ch = out->channels;
    h->dscene.force_general = (q->flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
    const bool by_object = query_by_object(h, q->flags);
    const bool generic_all = h->has_deep && (h->gen_all || h->dscene.force_general);
    // the views' device records: the camera constants by the host function a render uses (as rptgpu_render_views)
    std::vector<rptdev::View> recs(n_views);
    for (uint64_t v = 0; v < n_views; v++) {
      recs[v].cam = make_camera(views[v].camera);
      recs[v].projection = views[v].projection;
      recs[v].ortho_scale = views[v].ortho_scale;
    }
    h->view_recs.upload(recs, st);
    // views with seeds of their own: the first step alone reads a seed here (no rpt_shade follows it)
    const std::vector<uint64_t> seed_list = view_seed_list(n_views, *q, seeded ? seeds : nullptr);
    const bool per_view = !seed_list.empty();
    if (per_view) h->view_seeds.upload(seed_list, st);
    // the piece: at most the rays one pass may hold; a camera ray reaches depth 0 only, hence one record column per path
    const uint64_t n = n_views * npix;
    rptplan::PassInput in = pass_input(h, 1, q->iterations);
    in.remaining = q->iterations;
    in.rec_ratio = 1.0; in.ratio = 1.0;
    pass_input_now(h, in);
    uint64_t asked = 0; // tests: pieces of a few pixels
    if (const char* e = std::getenv("RPTGPU_VIEWS_PIECE")) asked = std::strtoull(e, nullptr, 10);
    const uint64_t piece = rptplan::views_piece(n, asked, rptplan::plan_pass(in).target);
    const bool at_views = false; // a piece spans views whatever their seeds
    h->ray_ids.alloc(piece);
    if (per_view) h->ray_seeds.alloc(piece);
    rptdev::AovOut stage{};
    if (!on_device) stage = aov_arrays(h->aov_out, st, piece, ch);
    for (uint64_t base = 0, m; base < n; base += m) {
      m = rptplan::views_piece_len(base, n, npix, piece, at_views);
      const ChannelPtrs mine = ptrs_at(rptplan::AOV_ROWS, out, ch | rptplan::AOV_HITS, base);
      const rptdev::AovOut ao = on_device ? aov_out(mine, ch) : stage;
      rptdev::Frame fr{};
      fr.width = (uint32_t)m; fr.height = 1; fr.npix = (uint32_t)m; fr.pixels = h->ray_ids.p;
      fr.seed = per_view ? 0 : q->seed;
      rptplan::PassInput pin = pass_input(h, (uint32_t)m, q->iterations);
      pin.rec_ratio = 1.0; pin.ratio = 1.0;
      // passes are sample-major and run in ascending sample order, so an index's additions happen in sample order whatever
      // the pass size (as rptgpu_render_aov's aov_wavefront)
      for (uint32_t s0 = 0; s0 < q->iterations;) {
        pin.remaining = q->iterations - s0;
        pass_input_now(h, pin);
        const rptplan::PassPlan pp = size_pass(h, pin, (uint32_t)m, generic_all);
        const uint32_t n_paths = (uint32_t)m * pp.s_chunk;
        fr.sample_base = q->sample_index_base + s0;
        const rptdev::PathState ps = path_state(h);
        if (h->has_deep) reset_tree_counters(h);
        if (per_view)
          kt->raygen_views_seeded(st, fr, h->view_recs.p, q->width, q->height, base, h->ray_ids.p, h->view_seeds.p, h->ray_seeds.p, 0, (uint32_t)m, ps, n_paths);
        else kt->raygen_views(st, fr, h->view_recs.p, q->width, q->height, base, h->ray_ids.p, ps, n_paths);
        if (by_object) query_closest(h, kt, ps, n_paths, nullptr);
        else kt->extend(st, h->dscene, ps, nullptr, n_paths);
        kt->views_aov_fold(st, h->dscene, ps, ao, (uint32_t)m, pp.s_chunk, s0 == 0);
        HIP_TRY(hipGetLastError());
        s0 += pp.s_chunk;
      }
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_aov_out(stage, ch, mine, m, st);
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return h->has_deep && h->gen_overflow.p;
  });
}

} // namespace rptapi

extern "C" {

int rptgpu_first_hits(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const RptHitQuery* q,
                      const RptHitArrays* out) {
  return first_hits(h, n, origins, dirs, q, out, false, nullptr);
}

int rptgpu_first_hits_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, const RptHitQuery* q,
                             const RptHitArrays* d_out, void* stream) {
  return first_hits(h, n, (const double*)d_origins, (const double*)d_dirs, q, d_out, true, (hipStream_t)stream);
}

int rptgpu_render_views_aov(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                            const RptAovBuffers* out) {
  return render_views_aov(h, n_views, views, q, false, nullptr, out, false, nullptr);
}

int rptgpu_render_views_aov_seeded(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                   const uint64_t* seeds, const RptAovBuffers* out) {
  return render_views_aov(h, n_views, views, q, true, seeds, out, false, nullptr);
}

int rptgpu_render_views_aov_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                   const RptAovBuffers* d_out, void* stream) {
  return render_views_aov(h, n_views, views, q, false, nullptr, d_out, true, (hipStream_t)stream);
}

int rptgpu_render_views_aov_seeded_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                          const uint64_t* seeds, const RptAovBuffers* d_out, void* stream) {
  return render_views_aov(h, n_views, views, q, true, seeds, d_out, true, (hipStream_t)stream);
}

} // extern "C"
