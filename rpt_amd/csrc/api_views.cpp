// api_views.cpp — rptgpu_render_views[_seeded][_device]: a batch of frames in one call, each from a camera of its own under one of
// three projections (include/rpt_gpu.h; see api_internal.h).  The n_views x width x height pixels of the call
// are the indices j = view * npix + pixel; they go through the wavefront driver of api_render.cpp in pieces of consecutive
// j (rptplan::views_piece) — a piece is the "frame" of its own passes, as a piece of rptgpu_trace_rays' rays is —,
// rpt_raygen_views makes each index's ray from its pixel's own stream (RaySource::views), and everything behind it — the
// depth loop, the pass planning with its restarts, rpt_resolve, rpt_finish in packed form straight into `out` at j — is a
// render's.  So the launches of a depth and its one host wait are shared by every view a piece holds — whatever the views'
// seeds: where they differ (rptgpu_render_views_seeded[_device], or a seed stride) the seed travels with the path
// (RaySource::view_seeds: rpt_raygen_views_seeded, rpt_shade_seeded), and pieces are cut where the one-seed route cuts them.
// Under RPT_FLAG_VIEWS_PERSISTENT (include/rpt_gpu_views_persistent.h) the same pieces go through the
// persistent driver instead: rpt_views_ids names each index's pixel and view, rpt_paths_views runs the piece's launches of at
// most spp_l samples, and rpt_sum_samples and the packed rpt_finish behind them are a render's.  The same bits.
// The loop over the pieces is this file's own — its indices are made on the device, not staged —; the steps it shares with
// api_rays.cpp's loop are api_internal.h's (piece_params, piece_pass_target, piece_persistent, persistent_piece, piece_frame,
// render_piece).
#include "api_internal.h"

namespace rptapi {

// what is wrong with an RptViewQuery (nullptr: nothing)
const char* bad_view_query(const RptViewQuery* q, bool views_persistent_ok) {
  if (!q) return "null RptViewQuery";
  if (q->struct_size != sizeof(RptViewQuery)) return "RptViewQuery: struct_size is not sizeof(RptViewQuery)";
  if (!q->width || !q->height || !q->iterations) return "RptViewQuery: width, height and iterations must be non-zero";
  if (q->max_bounces > 254) return "RptViewQuery: max_bounces > 254";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RptViewQuery: RPT_FLAG_PERSISTENT — the persistent kernel renders one camera's frame; a batch of views runs the "
           "wavefront pipeline only";
  if (q->flags & RPT_FLAG_VIEWS_PERSISTENT) {
    if (!views_persistent_ok)
      return "RptViewQuery: RPT_FLAG_VIEWS_PERSISTENT — only rptgpu_render_views and its _seeded and _device forms run a batch "
             "of views in the persistent kernel";
    if (q->flags & RPT_FLAG_WAVEFRONT)
      return "RptViewQuery: RPT_FLAG_VIEWS_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes";
  }
  if ((uint64_t)q->width * q->height > (1ull << 32)) return "RptViewQuery: width * height > 2^32 (a pixel is a 32-bit stream id)";
  return nullptr;
}

// what is wrong with one view of a call with query q (nullptr: nothing)
const char* bad_view(const RptView& v, const RptViewQuery& q) {
  switch (v.projection) {
    case RPT_VIEW_PERSPECTIVE: return nullptr;
    case RPT_VIEW_ORTHOGRAPHIC:
      if (!std::isfinite(v.ortho_scale) || !(v.ortho_scale > 0.0)) return "RptView: RPT_VIEW_ORTHOGRAPHIC needs a finite ortho_scale > 0";
      if (v.camera.aperture > 0.0) return "RptView: aperture > 0 — only RPT_VIEW_PERSPECTIVE has a lens";
      return nullptr;
    case RPT_VIEW_PANORAMA:
      if (v.camera.aperture > 0.0) return "RptView: aperture > 0 — only RPT_VIEW_PERSPECTIVE has a lens";
      if (q.width < 2 || q.height < 2) return "RptView: RPT_VIEW_PANORAMA needs width >= 2 and height >= 2";
      return nullptr;
    default: return "RptView: unknown projection (RPT_VIEW_PERSPECTIVE = 0, RPT_VIEW_ORTHOGRAPHIC = 1, RPT_VIEW_PANORAMA = 2)";
  }
}

std::vector<uint64_t> view_seed_list(uint64_t n_views, const RptViewQuery& q, const uint64_t* seeds) {
  if (seeds) return std::vector<uint64_t>(seeds, seeds + n_views);
  std::vector<uint64_t> list;
  if (q.seed_stride) {
    list.resize(n_views);
    for (uint64_t v = 0; v < n_views; v++) list[v] = q.seed + v * q.seed_stride; // (wraps: u64)
  }
  return list;
}

// out: host memory ([n_views][height][width][3] f64), or — on_device — device memory of f64 or f32 (user_stream: the
// stream its producer ran on); views is host memory either way.  seeded: the _seeded entry points — view v's seed is
// seeds[v] (host memory), and q's seed and seed_stride are not read
int render_views(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q, bool seeded, const uint64_t* seeds,
                 void* out, bool on_device, bool out_f32, hipStream_t user_stream) {
  // (the query first, then the views: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_view_query(q, true)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n_views && (!views || !out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (seeded && n_views && !seeds) return fail(h, RPTGPU_E_INVALID_ARGUMENT, NULL_SEEDS);
  const uint64_t npix = (uint64_t)q->width * q->height;
  if (n_views > (1ull << 58) / npix) // (3 values of 8 bytes per index: the frames' size in bytes fits 64 bits)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "n_views * width * height does not fit: the frames would not fit any memory");
  for (uint64_t v = 0; v < n_views; v++)
    if (const char* why = bad_view(views[v], *q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n_views) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(q->precision_mode, h->ext_shapes);
    h->dscene.force_general = (q->flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
    const RptRenderParams p = piece_params(*q, q->iterations, q->exposure_value);
    // the views' device records: the camera constants by the host function a render uses
    std::vector<rptdev::View> recs(n_views);
    for (uint64_t v = 0; v < n_views; v++) {
      recs[v].cam = make_camera(views[v].camera);
      recs[v].projection = views[v].projection;
      recs[v].ortho_scale = views[v].ortho_scale;
    }
    h->view_recs.upload(recs, st);
    const bool persistent = piece_persistent(h, q->flags, RPT_FLAG_VIEWS_PERSISTENT);
    std::vector<uint64_t> seed_list = view_seed_list(n_views, *q, seeded ? seeds : nullptr);
    // rpt_paths_views always reads a seed per view (its key is per lane): views that share the query's seed get equal ones
    if (persistent && seed_list.empty()) seed_list.assign(n_views, q->seed);
    const bool per_view = !seed_list.empty(); // the seed travels with the path
    if (per_view) h->view_seeds.upload(seed_list, st);
    // the piece: at most the paths one pass may hold with every level of every path (rptplan::views_piece)
    const uint64_t n = n_views * npix;
    uint64_t asked = 0; // tests: pieces of a few pixels
    if (const char* e = std::getenv("RPTGPU_VIEWS_PIECE")) asked = std::strtoull(e, nullptr, 10);
    uint64_t piece = rptplan::views_piece(n, asked, piece_pass_target(h, q->iterations, q->max_bounces));
    if (persistent) piece = persistent_piece(h, piece, q->iterations); // (rptplan::views_items at one sample per item)
    const bool at_views = false; // a piece spans views whatever their seeds
    const size_t out_elem = out_f32 ? sizeof(float) : sizeof(double);
    h->accum.alloc(3 * piece);
    h->ray_ids.alloc(piece);
    if (per_view && !persistent) h->ray_seeds.alloc(piece);
    if (persistent) h->view_of.alloc(piece);
    if (!on_device) h->rays_out.alloc(3 * piece);
    for (uint64_t base = 0, m; base < n; base += m) {
      m = rptplan::views_piece_len(base, n, npix, piece, at_views);
      void* d_out = on_device ? (void*)((char*)out + 3 * base * out_elem) : (void*)h->rays_out.p;
      rptdev::Frame fr = piece_frame(h, p, h->ray_ids.p, m);
      if (per_view) fr.seed = 0;
      RaySource src{};
      src.ids_out = h->ray_ids.p;
      src.views = h->view_recs.p; src.view_width = q->width; src.view_height = q->height; src.view_base = base;
      if (per_view) { src.view_seeds = h->view_seeds.p; src.seeds_out = h->ray_seeds.p; }
      if (persistent) {
        src.view_of = h->view_of.p;
        kt->views_ids(st, base, npix, (uint32_t)m, h->ray_ids.p, h->view_of.p);
      }
      render_piece(h, kt, p, fr, src, d_out, out_f32, persistent);
      if (!on_device) { // the staging array is the next piece's, too
        HIP_TRY(hipMemcpyAsync((double*)out + 3 * base, d_out, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return !persistent && h->has_deep && h->gen_overflow.p;
  });
}

} // namespace rptapi

extern "C" {

int rptgpu_render_views(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q, double* out) {
  return render_views(h, n_views, views, q, false, nullptr, out, false, false, nullptr);
}

int rptgpu_render_views_seeded(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                               const uint64_t* seeds, double* out) {
  return render_views(h, n_views, views, q, true, seeds, out, false, false, nullptr);
}

int rptgpu_render_views_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q, void* d_out,
                               int out_is_f32, void* stream) {
  return render_views(h, n_views, views, q, false, nullptr, d_out, true, out_is_f32 != 0, (hipStream_t)stream);
}

int rptgpu_render_views_seeded_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q,
                                      const uint64_t* seeds, void* d_out, int out_is_f32, void* stream) {
  return render_views(h, n_views, views, q, true, seeds, d_out, true, out_is_f32 != 0, (hipStream_t)stream);
}

int rptgpu_views_persistent_supported(void) { return 1; }

} // extern "C"
