// api_rays.cpp — rptgpu_trace_rays[_device]: the full path estimator for rays the caller supplies (include/rpt_gpu.h,
// DESIGN.md §13; see api_internal.h).  The rays go through the wavefront driver of api_render.cpp in pieces: a piece is
// the "frame" of its own passes, its rays are the pixels, rpt_raygen_rays is the passes' first step (RaySource) and
// everything behind it — the depth loop, the pass planning with its restarts, rpt_resolve, rpt_finish in packed form —
// is a render's.  A host caller's piece is staged in arrays the handle keeps; a device caller's is read where it lies.
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
  auto t0 = std::chrono::steady_clock::now();
  const int rc = guarded(h, h->device, [&]() -> int {
    struct EventPairs { // (as render_impl: a call leaves no event pair behind, however it ends)
      rptgpu_scene* h;
      ~EventPairs() { h->pending.clear(); h->ev_used = 0; }
    } event_pairs{h};
    (void)hipGetLastError();
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(q->precision_mode, h->ext_shapes);
    const bool prof = (q->flags & RPT_FLAG_PROFILE_KERNELS) != 0;
    if (user_stream) HIP_TRY(hipStreamSynchronize(user_stream));
    h->dscene.force_general = (q->flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
    RptRenderParams p{}; // what render_wavefront reads of it
    p.max_bounces = q->max_bounces; p.iterations = q->iterations; p.exposure_value = q->exposure_value;
    p.seed = q->seed; p.sample_index_base = q->sample_index_base; p.precision_mode = q->precision_mode; p.flags = q->flags;
    // the piece: at most the paths one pass may hold with every level of every path (rptplan::rays_piece)
    rptplan::PassInput in = pass_input(h, 1, q->iterations);
    in.remaining = q->iterations;
    in.ratio = (double)q->max_bounces + 1.0;
    pass_input_now(h, in);
    uint64_t asked = 0; // tests: pieces of a few rays
    if (const char* e = std::getenv("RPTGPU_RAYS_PIECE")) asked = std::strtoull(e, nullptr, 10);
    uint64_t piece = rptplan::rays_piece(n, asked, rptplan::plan_pass(in).target);
    // the persistent kernel on request — unless the scene has a group with tree children, which only the wavefront
    // pipeline walks (use_wavefront: such a scene cannot honour the request, as for a render); a piece is then also at
    // most what a launch's work counter holds
    const bool persistent = (q->flags & RPT_FLAG_RAYS_PERSISTENT) && !use_wavefront(h, 0, false);
    if (persistent) piece = handle_rays_persistent_piece(h, piece, q->iterations);
    h->accum.alloc(3 * piece);
    if (!on_device) { h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); h->rays_out.alloc(3 * piece); }
    if (!on_device || !streams) h->ray_ids.alloc(piece);
    for (uint64_t base = 0; base < n; base += piece) {
      const uint64_t m = std::min(piece, n - base);
      const double *d_o = origins + 3 * base, *d_d = dirs + 3 * base;
      const uint32_t* d_ids = streams ? streams + base : h->ray_ids.p;
      double* d_out = out + 3 * base;
      if (!on_device) {
        HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_o, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_d, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
        if (streams) HIP_TRY(hipMemcpyAsync(h->ray_ids.p, d_ids, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        d_o = h->rays_o.p; d_d = h->rays_d.p; d_ids = h->ray_ids.p; d_out = h->rays_out.p;
      }
      rptdev::Frame fr{};
      fr.width = (uint32_t)m; fr.height = 1; fr.npix = (uint32_t)m; fr.pixels = d_ids;
      fr.max_bounces = q->max_bounces; fr.seed = q->seed; fr.accum = h->accum.p;
      const RaySource src{nullptr, d_o, d_d, q->first_draw, (uint32_t)base, streams ? nullptr : h->ray_ids.p};
      if (persistent) { // (the ids the wavefront's first step would write: the kernel reads them from the first launch on)
        if (!streams) kt->rays_ids(st, (uint32_t)base, (uint32_t)m, h->ray_ids.p);
        render_persistent(h, kt, p, fr, src, d_out, false, true, prof);
      } else {
        render_wavefront(h, kt, p, fr, src, d_out, false, true, prof);
      }
      HIP_TRY(hipGetLastError());
      if (!on_device) { // the staging arrays are the next piece's, too
        HIP_TRY(hipMemcpyAsync(out + 3 * base, d_out, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return drain_call(h, !persistent && h->has_deep && h->gen_overflow.p);
  });
  if (rc != RPTGPU_OK) return rc;
  h->stats.total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return RPTGPU_OK;
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
