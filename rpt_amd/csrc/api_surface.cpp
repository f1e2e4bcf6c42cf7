// api_surface.cpp — rptgpu_hit_surface[_device]: the triangle, the barycentrics and the group's child behind a ray's first hit
// (include/rpt_gpu_hit_surface.h; see api_internal.h).  Per piece: rptgpu_first_hits' own query for T and
// OBJECT (api_hits.cpp plan_hit_pieces / hit_piece, unchanged: rpt_first_hits, or rpt_raygen_rays + the per-tree query +
// rpt_hits_store) into the caller's arrays where named, else into a pair the handle keeps; then rpt_hit_surface
// (kernels/hit_surface.inc), which walks each ray's hit object alone with the record cut at the hit.  The sizes — the walk's
// columns, the pair, a host caller's staging — and RptSurfaceArrays' channel table are surface_plan.h's.
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t SURFACE_ALL = RPT_SURFACE_T | RPT_SURFACE_OBJECT | RPT_SURFACE_CHILD | RPT_SURFACE_PRIMITIVE | RPT_SURFACE_BARYCENTRIC;
static_assert(rptsurface::CH_T == RPT_SURFACE_T && rptsurface::CH_OBJECT == RPT_SURFACE_OBJECT &&
              rptsurface::CH_CHILD == RPT_SURFACE_CHILD && rptsurface::CH_PRIMITIVE == RPT_SURFACE_PRIMITIVE &&
              rptsurface::CH_BARYCENTRIC == RPT_SURFACE_BARYCENTRIC && rptsurface::CH_ALL == SURFACE_ALL,
              "surface_plan.h restates the header's channel bits");

// what is wrong with an RptSurfaceQuery (nullptr: nothing)
static const char* bad_surface_query(const RptSurfaceQuery* q) {
  if (const char* why = bad_channel_query(q, RPT_QUERY_TEXTS(RptSurfaceQuery, RPT_SURFACE), SURFACE_ALL)) return why;
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; hit surfaces run the closest-hit query "
           "and a resolve walk only";
  return nullptr;
}

// (these three: also rptgpu_lookup_lightmap's, api_lightmap_lookup.cpp — declared in api_internal.h)
// rpt_hit_surface's columns for pieces of `piece` rays, as high as the scene needs now (a live rebuild may have raised
// gen_levels: taller columns hold the same walk), and the flag a walk raises if it outgrows them
GenericStack ensure_surface_columns(rptgpu_scene* h, uint64_t piece) {
  const rptsurface::Columns want = rptsurface::columns(piece, h->gen_levels, h->gen_frames);
  rptsurface::Columns& have = h->surf_cols;
  if (!h->surf_defer.p || have.threads < want.threads || have.levels < want.levels || have.frames < want.frames) {
    h->surf_defer.release(); h->surf_frame.release();
    have = rptsurface::Columns{};
    h->surf_defer.alloc(want.defer_words);
    h->surf_frame.alloc(want.frame_words);
    have = want;
  }
  if (!h->gen_overflow.p) {
    h->gen_overflow.alloc(1);
    HIP_TRY(hipMemsetAsync(h->gen_overflow.p, 0, sizeof(uint32_t), h->stream));
  }
  return GenericStack{h->surf_defer.p, h->surf_frame.p, have.threads, have.levels, have.frames};
}

// does some group of the scene hold a MonomialSurface?  (its accept guard is not `time >= record.time`: hit_surface.inc)
bool group_holds_monomial(const rptgpu_scene* h) {
  for (size_t i = h->top_insts.size(); i < h->inst_sig.size(); i++)
    if ((h->inst_sig[i] & 0x7f) == RPT_SHAPE_MONOMIAL) return true;
  return false;
}

// the resolve walk over m rays at d_o / d_d whose T and OBJECT stand in `so`, into so's named channels
void surface_walk_piece(rptgpu_scene* h, const double* d_o, const double* d_d, uint32_t m, const rptdev::SurfaceOut& so,
                        const GenericStack& gs, bool from_inf) {
  const uint32_t blocks = rptsurface::launch_blocks(m, h->surf_cols);
  if (h->ext_shapes) rpt_strict_ext_surface::launch_hit_surface(h->stream, h->dscene, d_o, d_d, m, so, gs, from_inf, h->gen_overflow.p, blocks);
  else rpt_strict_surface::launch_hit_surface(h->stream, h->dscene, d_o, d_d, m, so, gs, from_inf, h->gen_overflow.p, blocks);
  HIP_TRY(hipGetLastError());
}

namespace {

// on_device: origins, dirs and out's arrays are device pointers (user_stream: the stream their producer ran on)
int hit_surface(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const RptSurfaceQuery* q,
                const RptSurfaceArrays* out, bool on_device, hipStream_t user_stream) {
  // (the query first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_surface_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_channel_arrays(out, RPT_ARRAYS_TEXTS(RptSurfaceArrays), rptsurface::ROWS, q->channels))
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
    const bool walk = rptsurface::needs_walk(ch);
    const HitPieces hp = plan_hit_pieces(h, n, q->flags, "RPTGPU_SURFACE_PIECE");
    const uint64_t piece = hp.piece;
    // the handle's arrays for a piece: a host caller's channels, and T / OBJECT for the walk where the caller's do not serve
    const rptsurface::Layout lay = rptsurface::layout(piece, ch, on_device);
    h->surface_out.alloc(lay.words);
    const ChannelPtrs mine_dev = ptrs_in(h->surface_out.p, lay);
    if (!on_device) { h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); }
    GenericStack gs{};
    bool from_inf = false;
    if (walk) {
      gs = ensure_surface_columns(h, piece);
      from_inf = group_holds_monomial(h);
    }
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const double *d_o = origins + 3 * base, *d_d = dirs + 3 * base;
      const ChannelPtrs theirs = ptrs_at(rptsurface::ROWS, out, ch, base);
      if (!on_device) stage_rays(h, d_o, d_d, m);
      // where this piece's results lie on the device: the caller's arrays (device callers), else the handle's — the
      // kernels' struct from the arrays of rptsurface::ROWS
      const ChannelPtrs& dev = on_device ? theirs : mine_dev;
      double* const t = (lay.has & RPT_SURFACE_T ? mine_dev : dev).at<double>(rptsurface::R_T);
      int32_t* const object = (lay.has & RPT_SURFACE_OBJECT ? mine_dev : dev).at<int32_t>(rptsurface::R_OBJECT);
      rptdev::SurfaceOut so{};
      so.t = t; so.object = object;
      so.child = dev.at<int32_t>(rptsurface::R_CHILD); so.primitive = dev.at<int32_t>(rptsurface::R_PRIMITIVE);
      so.barycentric = dev.at<double>(rptsurface::R_BARYCENTRIC);
      so.channels = ch & (RPT_SURFACE_CHILD | RPT_SURFACE_PRIMITIVE | RPT_SURFACE_BARYCENTRIC);
      // 1. rptgpu_first_hits' query for T | OBJECT — what the caller named of the two, and both where the walk follows
      rptdev::HitOut ho{};
      if (t) { ho.channels |= RPT_HIT_T; ho.t = t; }
      if (object) { ho.channels |= RPT_HIT_OBJECT; ho.object = object; }
      hit_piece(h, kt, hp, d_o, d_d, m, ho, prof);
      // 2. the resolve walk
      if (walk) surface_walk_piece(h, d_o, d_d, m, so, gs, from_inf);
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_out(rptsurface::ROWS, mine_dev, theirs, ch, m, st);
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return (walk || h->has_deep) && h->gen_overflow.p;
  });
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_hit_surface(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const RptSurfaceQuery* q,
                       const RptSurfaceArrays* out) {
  return hit_surface(h, n, origins, dirs, q, out, false, nullptr);
}

int rptgpu_hit_surface_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, const RptSurfaceQuery* q,
                              const RptSurfaceArrays* d_out, void* stream) {
  return hit_surface(h, n, (const double*)d_origins, (const double*)d_dirs, q, d_out, true, (hipStream_t)stream);
}

} // extern "C"
