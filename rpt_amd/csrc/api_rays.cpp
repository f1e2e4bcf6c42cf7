// api_rays.cpp — rptgpu_trace_rays[_device]: the full path estimator for rays the caller supplies (include/rpt_gpu.h,
// DESIGN.md §13; see api_internal.h), and the piece loop it shares with rptgpu_bake_probes (api_probes.cpp) and
// rptgpu_trace_vertices (api_vertices.cpp): trace_ray_pieces.  The rays go through the wavefront driver of api_render.cpp in
// pieces: a piece is the "frame" of its own passes, its rays are the pixels, rpt_raygen_rays is the passes' first step
// (RaySource) and everything behind it — the depth loop, the pass planning with its restarts, rpt_resolve, rpt_finish in
// packed form — is a render's.  A host caller's piece is staged in arrays the handle keeps; a device caller's is read where
// it lies.
// Under RPT_FLAG_RAYS_PERSISTENT (include/rpt_gpu_rays_persistent.h) the same pieces, staged the same way,
// go through the persistent driver instead: rpt_paths_rays reads each ray where it hands out its work, and rpt_sum_samples
// and the packed rpt_finish behind its launches are a render's.  The same bits.
#include "api_internal.h"

namespace rptapi {

// what is wrong with an RptRayQuery (nullptr: nothing)
const char* bad_ray_query(const RptRayQuery* q) {
  if (!q) return "null RptRayQuery";
  if (q->struct_size != sizeof(RptRayQuery)) return "RptRayQuery: struct_size is not sizeof(RptRayQuery)";
  if (!q->iterations) return "RptRayQuery: iterations == 0";
  if (q->max_bounces > 254) return "RptRayQuery: max_bounces > 254";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RptRayQuery: RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; caller-supplied rays run "
           "the wavefront pipeline only";
  if ((q->flags & RPT_FLAG_RAYS_PERSISTENT) && (q->flags & RPT_FLAG_WAVEFRONT))
    return "RptRayQuery: RPT_FLAG_RAYS_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes";
  return nullptr;
}

void trace_ray_pieces(rptgpu_scene* h, const RayPieces& c, const std::function<void(uint64_t, uint64_t, RaySource&)>& before,
                      const std::function<void(uint64_t, uint64_t)>& after) {
  hipStream_t st = h->stream;
  const KernelTable* kt = table_for(c.p.precision_mode, h->ext_shapes);
  h->dscene.force_general = (c.p.flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
  const uint64_t piece = c.piece, w = c.width;
  h->accum.alloc(w * piece);
  // the drivers write a piece's results somewhere: the device caller's array, or the handle's
  if (!c.on_device || !c.out) h->rays_out.alloc(w * piece);
  if (!c.on_device) {
    h->rays_o.alloc(3 * piece);
    if (c.b) h->rays_d.alloc(3 * piece);
  }
  if (!c.on_device || !c.streams) h->ray_ids.alloc(piece);
  for (uint64_t base = 0; base < c.n; base += piece) {
    const uint64_t m = std::min(piece, c.n - base);
    const double *d_a = c.a + 3 * base, *d_b = c.b ? c.b + 3 * base : nullptr;
    const uint32_t* d_ids = c.streams ? c.streams + base : h->ray_ids.p;
    double* d_out = c.on_device && c.out ? c.out + w * base : h->rays_out.p;
    if (!c.on_device) {
      HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_a, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
      if (c.b) HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_b, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
      if (c.streams) HIP_TRY(hipMemcpyAsync(h->ray_ids.p, d_ids, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      d_a = h->rays_o.p; d_b = c.b ? h->rays_d.p : nullptr; d_ids = h->ray_ids.p;
    }
    const rptdev::Frame fr = piece_frame(h, c.p, d_ids, m);
    RaySource src{nullptr, d_a, d_b, c.first_draw, (uint32_t)base, c.streams ? nullptr : h->ray_ids.p};
    src.probe = c.probe; src.probe_scale = c.probe_scale;
    if (before) before(base, m, src);
    // (the ids the wavefront's first step would write: the persistent kernel reads them from the first launch on)
    if (c.persistent && !c.streams) kt->rays_ids(st, (uint32_t)base, (uint32_t)m, h->ray_ids.p);
    render_piece(h, kt, c.p, fr, src, d_out, false, c.persistent);
    if (after) after(base, m);
    if (!c.on_device) { // the staging arrays are the next piece's, too
      if (c.out) HIP_TRY(hipMemcpyAsync(c.out + w * base, d_out, w * m * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
  }
}

namespace {

// on_device: origins, dirs, streams and out are device pointers (user_stream: the stream their producer ran on)
int trace_rays(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const uint32_t* streams,
               const RptRayQuery* q, double* out, bool on_device, hipStream_t user_stream) {
  // (the query first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_ray_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!origins || !dirs || !out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!streams && n > (1ull << 32))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "more than 2^32 rays without stream ids (a stream id has 32 bits)");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() {
    // the piece: at most the paths one pass may hold with every level of every path (rptplan::rays_piece)
    uint64_t asked = 0; // tests: pieces of a few rays
    if (const char* e = std::getenv("RPTGPU_RAYS_PIECE")) asked = std::strtoull(e, nullptr, 10);
    uint64_t piece = rptplan::rays_piece(n, asked, piece_pass_target(h, q->iterations, q->max_bounces));
    const bool persistent = piece_persistent(h, q->flags, RPT_FLAG_RAYS_PERSISTENT);
    if (persistent) piece = persistent_piece(h, piece, q->iterations);
    trace_ray_pieces(h, RayPieces{n, origins, dirs, streams, on_device, piece, persistent,
                                  piece_params(*q, q->iterations, q->exposure_value), q->first_draw, 3, out},
                     nullptr, nullptr);
    return !persistent && h->has_deep && h->gen_overflow.p;
  });
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_trace_rays(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const uint32_t* streams,
                      const RptRayQuery* q, double* out_rgb) {
  return trace_rays(h, n, origins, dirs, streams, q, out_rgb, false, nullptr);
}

int rptgpu_trace_rays_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, const void* d_streams,
                             const RptRayQuery* q, void* d_out_rgb, void* stream) {
  return trace_rays(h, n, (const double*)d_origins, (const double*)d_dirs, (const uint32_t*)d_streams, q, (double*)d_out_rgb, true,
                    (hipStream_t)stream);
}

int rptgpu_rays_persistent_supported(void) { return 1; }

} // extern "C"
