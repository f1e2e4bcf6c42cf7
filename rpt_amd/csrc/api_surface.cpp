// api_surface.cpp — rptgpu_hit_surface[_device]: the triangle, the barycentrics and the group's child behind a ray's first hit
// (include/rpt_gpu_hit_surface.h; see api_internal.h).  Per piece: rptgpu_first_hits' own query for T and
// OBJECT (api_hits.cpp plan_hit_pieces / hit_piece, unchanged: rpt_first_hits, or rpt_raygen_rays + the per-tree query +
// rpt_hits_store) into the caller's arrays where named, else into a pair the handle keeps; then rpt_hit_surface
// (kernels/hit_surface.inc), which walks each ray's hit object alone with the record cut at the hit.  The sizes — the walk's
// columns, the pair, a host caller's staging — are surface_plan.h's.
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t SURFACE_ALL = RPT_SURFACE_T | RPT_SURFACE_OBJECT | RPT_SURFACE_CHILD | RPT_SURFACE_PRIMITIVE | RPT_SURFACE_BARYCENTRIC;
static_assert(rptsurface::CH_T == RPT_SURFACE_T && rptsurface::CH_OBJECT == RPT_SURFACE_OBJECT &&
              rptsurface::CH_CHILD == RPT_SURFACE_CHILD && rptsurface::CH_PRIMITIVE == RPT_SURFACE_PRIMITIVE &&
              rptsurface::CH_BARYCENTRIC == RPT_SURFACE_BARYCENTRIC && rptsurface::CH_ALL == SURFACE_ALL,
              "surface_plan.h restates the header's channel bits");

// what is wrong with an RptSurfaceQuery / with the RptSurfaceArrays of a call that names `channels` (nullptr: nothing)
static const char* bad_surface_query(const RptSurfaceQuery* q) {
  if (!q) return "null RptSurfaceQuery";
  if (q->struct_size != sizeof(RptSurfaceQuery)) return "RptSurfaceQuery: struct_size is not sizeof(RptSurfaceQuery)";
  if (!q->channels) return "RptSurfaceQuery: channels == 0 (name at least one RPT_SURFACE_* channel)";
  if (q->channels & ~SURFACE_ALL) return "RptSurfaceQuery: channels names an unknown RPT_SURFACE_* bit";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; hit surfaces run the closest-hit query "
           "and a resolve walk only";
  return nullptr;
}
static const char* bad_surface_arrays(const RptSurfaceArrays* o, uint32_t channels) {
  if (!o) return "null RptSurfaceArrays";
  if (o->struct_size != sizeof(RptSurfaceArrays)) return "RptSurfaceArrays: struct_size is not sizeof(RptSurfaceArrays)";
  if (o->reserved) return "RptSurfaceArrays: reserved != 0";
  if ((channels & RPT_SURFACE_T) && !o->t) return "RptSurfaceArrays: RPT_SURFACE_T is named but t is NULL";
  if ((channels & RPT_SURFACE_OBJECT) && !o->object) return "RptSurfaceArrays: RPT_SURFACE_OBJECT is named but object is NULL";
  if ((channels & RPT_SURFACE_CHILD) && !o->child) return "RptSurfaceArrays: RPT_SURFACE_CHILD is named but child is NULL";
  if ((channels & RPT_SURFACE_PRIMITIVE) && !o->primitive)
    return "RptSurfaceArrays: RPT_SURFACE_PRIMITIVE is named but primitive is NULL";
  if ((channels & RPT_SURFACE_BARYCENTRIC) && !o->barycentric)
    return "RptSurfaceArrays: RPT_SURFACE_BARYCENTRIC is named but barycentric is NULL";
  return nullptr;
}

namespace {

// the arrays of a piece: where the first-hit query writes T and OBJECT, and what the resolve walk reads and writes
struct PieceArrays {
  double* t;
  int32_t* object;
  int32_t* child;
  int32_t* primitive;
  double* barycentric;
};
// the caller's arrays from ray `base` on (a channel that is not named: its pointer is not read)
PieceArrays surface_arrays_at(const RptSurfaceArrays& a, uint32_t ch, uint64_t base) {
  PieceArrays p{};
  if (ch & RPT_SURFACE_T) p.t = a.t + base;
  if (ch & RPT_SURFACE_OBJECT) p.object = a.object + base;
  if (ch & RPT_SURFACE_CHILD) p.child = a.child + base;
  if (ch & RPT_SURFACE_PRIMITIVE) p.primitive = a.primitive + base;
  if (ch & RPT_SURFACE_BARYCENTRIC) p.barycentric = a.barycentric + 3 * base;
  return p;
}
// ... and those of layout l inside the handle's allocation
PieceArrays surface_arrays_in(double* base, const rptsurface::Layout& l) {
  PieceArrays p{};
  if (l.has & RPT_SURFACE_T) p.t = base + l.t;
  if (l.has & RPT_SURFACE_OBJECT) p.object = (int32_t*)(base + l.object);
  if (l.has & RPT_SURFACE_CHILD) p.child = (int32_t*)(base + l.child);
  if (l.has & RPT_SURFACE_PRIMITIVE) p.primitive = (int32_t*)(base + l.primitive);
  if (l.has & RPT_SURFACE_BARYCENTRIC) p.barycentric = base + l.barycentric;
  return p;
}
void copy_surface_out(const PieceArrays& src, const PieceArrays& dst, uint32_t ch, uint64_t m, hipStream_t st) {
  if (ch & RPT_SURFACE_T) HIP_TRY(hipMemcpyAsync(dst.t, src.t, m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_SURFACE_OBJECT) HIP_TRY(hipMemcpyAsync(dst.object, src.object, m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (ch & RPT_SURFACE_CHILD) HIP_TRY(hipMemcpyAsync(dst.child, src.child, m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (ch & RPT_SURFACE_PRIMITIVE) HIP_TRY(hipMemcpyAsync(dst.primitive, src.primitive, m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (ch & RPT_SURFACE_BARYCENTRIC)
    HIP_TRY(hipMemcpyAsync(dst.barycentric, src.barycentric, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
}

} // namespace

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
  if (const char* why = bad_surface_arrays(out, q->channels)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
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
    const PieceArrays mine_dev = surface_arrays_in(h->surface_out.p, lay);
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
      const PieceArrays theirs = surface_arrays_at(*out, ch, base);
      if (!on_device) {
        HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_o, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_d, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        d_o = h->rays_o.p; d_d = h->rays_d.p;
      }
      // where this piece's results lie on the device: the caller's arrays (device callers), else the handle's
      PieceArrays dev = on_device ? theirs : mine_dev;
      if (lay.has & RPT_SURFACE_T) dev.t = mine_dev.t;
      if (lay.has & RPT_SURFACE_OBJECT) dev.object = mine_dev.object;
      // 1. rptgpu_first_hits' query for T | OBJECT — what the caller named of the two, and both where the walk follows
      rptdev::HitOut ho{};
      if (dev.t) { ho.channels |= RPT_HIT_T; ho.t = dev.t; }
      if (dev.object) { ho.channels |= RPT_HIT_OBJECT; ho.object = dev.object; }
      hit_piece(h, kt, hp, d_o, d_d, m, ho, prof);
      // 2. the resolve walk
      if (walk) {
        rptdev::SurfaceOut so{};
        so.t = dev.t; so.object = dev.object;
        so.child = dev.child; so.primitive = dev.primitive; so.barycentric = dev.barycentric;
        so.channels = ch & (RPT_SURFACE_CHILD | RPT_SURFACE_PRIMITIVE | RPT_SURFACE_BARYCENTRIC);
        surface_walk_piece(h, d_o, d_d, m, so, gs, from_inf);
      }
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_surface_out(mine_dev, theirs, ch, m, st);
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
