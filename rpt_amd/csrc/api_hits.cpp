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

// what is wrong with an RptHitQuery / with the RptHitArrays of a call that names `channels` (nullptr: nothing)
static const char* bad_hit_query(const RptHitQuery* q) {
  if (!q) return "null RptHitQuery";
  if (q->struct_size != sizeof(RptHitQuery)) return "RptHitQuery: struct_size is not sizeof(RptHitQuery)";
  if (!q->channels) return "RptHitQuery: channels == 0 (name at least one RPT_HIT_* channel)";
  if (q->channels & ~HIT_ALL) return "RptHitQuery: channels names an unknown RPT_HIT_* bit";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; first hits run the closest-hit query only";
  return nullptr;
}
static const char* bad_hit_arrays(const RptHitArrays* o, uint32_t channels) {
  if (!o) return "null RptHitArrays";
  if (o->struct_size != sizeof(RptHitArrays)) return "RptHitArrays: struct_size is not sizeof(RptHitArrays)";
  if (o->reserved) return "RptHitArrays: reserved != 0";
  if ((channels & RPT_HIT_T) && !o->t) return "RptHitArrays: RPT_HIT_T is named but t is NULL";
  if ((channels & RPT_HIT_NORMAL) && !o->normal) return "RptHitArrays: RPT_HIT_NORMAL is named but normal is NULL";
  if ((channels & RPT_HIT_OBJECT) && !o->object) return "RptHitArrays: RPT_HIT_OBJECT is named but object is NULL";
  if ((channels & RPT_HIT_POSITION) && !o->position) return "RptHitArrays: RPT_HIT_POSITION is named but position is NULL";
  if ((channels & RPT_HIT_ALBEDO) && !o->albedo) return "RptHitArrays: RPT_HIT_ALBEDO is named but albedo is NULL";
  return nullptr;
}

namespace {

// the arrays of the named channels from ray `base` on (a channel that is not named: its pointer is not read)
rptdev::HitOut hit_arrays_at(const RptHitArrays& a, uint32_t channels, uint64_t base) {
  rptdev::HitOut ho{};
  ho.channels = channels;
  if (channels & RPT_HIT_T) ho.t = a.t + base;
  if (channels & RPT_HIT_NORMAL) ho.normal = a.normal + 3 * base;
  if (channels & RPT_HIT_OBJECT) ho.object = a.object + base;
  if (channels & RPT_HIT_POSITION) ho.position = a.position + 3 * base;
  if (channels & RPT_HIT_ALBEDO) ho.albedo = a.albedo + 3 * base;
  return ho;
}
// a host caller's piece of records on the device: the named channels of `piece` rays back to back inside `arrays`, the f64
// channels first, each 16-byte aligned
rptdev::HitOut hit_staging(DevBuf<double>& arrays, uint64_t piece, uint32_t channels) {
  const uint64_t one = (piece + 1) / 2 * 2, three = (3 * piece + 1) / 2 * 2;
  uint64_t off = 0, off_t = 0, off_normal = 0, off_position = 0, off_albedo = 0, off_object = 0;
  if (channels & RPT_HIT_T) { off_t = off; off += one; }
  if (channels & RPT_HIT_NORMAL) { off_normal = off; off += three; }
  if (channels & RPT_HIT_POSITION) { off_position = off; off += three; }
  if (channels & RPT_HIT_ALBEDO) { off_albedo = off; off += three; }
  if (channels & RPT_HIT_OBJECT) { off_object = off; off += (piece + 3) / 4 * 2; }
  arrays.alloc(off);
  rptdev::HitOut ho{};
  ho.channels = channels;
  if (channels & RPT_HIT_T) ho.t = arrays.p + off_t;
  if (channels & RPT_HIT_NORMAL) ho.normal = arrays.p + off_normal;
  if (channels & RPT_HIT_POSITION) ho.position = arrays.p + off_position;
  if (channels & RPT_HIT_ALBEDO) ho.albedo = arrays.p + off_albedo;
  if (channels & RPT_HIT_OBJECT) ho.object = (int32_t*)(arrays.p + off_object);
  return ho;
}
void copy_hits_out(const rptdev::HitOut& src, const rptdev::HitOut& dst, uint64_t m, hipStream_t st) {
  const uint32_t ch = src.channels;
  if (ch & RPT_HIT_T) HIP_TRY(hipMemcpyAsync(dst.t, src.t, m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_HIT_NORMAL) HIP_TRY(hipMemcpyAsync(dst.normal, src.normal, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_HIT_OBJECT) HIP_TRY(hipMemcpyAsync(dst.object, src.object, m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (ch & RPT_HIT_POSITION) HIP_TRY(hipMemcpyAsync(dst.position, src.position, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_HIT_ALBEDO) HIP_TRY(hipMemcpyAsync(dst.albedo, src.albedo, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
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
  if (const char* why = bad_hit_arrays(out, q->channels)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
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
    rptdev::HitOut stage{};
    if (!on_device) {
      h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece);
      stage = hit_staging(h->hits_out, piece, ch);
    }
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const double *d_o = origins + 3 * base, *d_d = dirs + 3 * base;
      const rptdev::HitOut mine = hit_arrays_at(*out, ch, base);
      if (!on_device) {
        HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_o, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_d, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        d_o = h->rays_o.p; d_d = h->rays_d.p;
      }
      hit_piece(h, kt, hp, d_o, d_d, m, on_device ? mine : stage, prof);
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_hits_out(stage, mine, m, st);
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return h->has_deep && h->gen_overflow.p;
  });
}

// rptgpu_render_aov's arrays from index `base` of the call on
RptAovBuffers aov_buffers_at(const RptAovBuffers& a, uint64_t base) {
  RptAovBuffers b = a;
  const uint32_t ch = a.channels;
  b.hits = a.hits + base;
  b.depth = (ch & RPT_AOV_DEPTH) ? a.depth + base : nullptr;
  b.normal = (ch & RPT_AOV_NORMAL) ? a.normal + 3 * base : nullptr;
  b.albedo = (ch & RPT_AOV_ALBEDO) ? a.albedo + 3 * base : nullptr;
  b.position = (ch & RPT_AOV_POSITION) ? a.position + 3 * base : nullptr;
  b.object = (ch & RPT_AOV_OBJECT) ? a.object + base : nullptr;
  return b;
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
      const RptAovBuffers mine = aov_buffers_at(*out, base);
      rptdev::AovOut ao = stage;
      if (on_device) {
        ao.channels = ch;
        ao.hits = mine.hits; ao.depth = mine.depth; ao.normal = mine.normal; ao.albedo = mine.albedo;
        ao.position = mine.position; ao.object = mine.object;
      }
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
