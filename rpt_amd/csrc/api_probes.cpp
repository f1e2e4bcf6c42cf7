// api_probes.cpp — rptgpu_bake_probes[_device]: light probes baked on the device (include/rpt_gpu.h; see
// api_internal.h).  A probe is `samples` paths whose first rays the library makes itself, so the call is rptgpu_trace_rays'
// with another first step and another last one: the probes go through the wavefront driver of api_render.cpp in pieces of
// whole probes — a piece is the "frame" of its own passes, its probes are the pixels, the samples are the iterations —,
// rpt_raygen_probes draws the directions (RaySource::probe), rpt_resolve_probes projects the paths' radiance into the
// piece's running sums and rpt_finish_probes scales them into the caller's layout.  The depth loop, the pass planning with
// its restarts and the piece arithmetic (rptplan::rays_piece) are the ray call's, unchanged.
// Under RPT_FLAG_RAYS_PERSISTENT (include/rpt_gpu_rays_persistent.h) the same pieces go through the persistent
// driver instead: rpt_paths_rays draws each direction where it hands out its work, rpt_project_probes adds a launch's samples
// to the sums with rpt_resolve_probes' expressions, and rpt_finish_probes is the one above.  The same bits.
#include "api_internal.h"

namespace rptapi {

// what is wrong with an RptProbeQuery (nullptr: nothing)
const char* bad_probe_query(const RptProbeQuery* q) {
  if (!q) return "null RptProbeQuery";
  if (q->struct_size != sizeof(RptProbeQuery)) return "RptProbeQuery: struct_size is not sizeof(RptProbeQuery)";
  if (q->kind != RPT_PROBE_SH9 && q->kind != RPT_PROBE_IRRADIANCE) return "RptProbeQuery: unknown kind (RPT_PROBE_SH9 = 0, RPT_PROBE_IRRADIANCE = 1)";
  if (!q->samples) return "RptProbeQuery: samples == 0";
  if (q->max_bounces > 254) return "RptProbeQuery: max_bounces > 254";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RptProbeQuery: RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; light probes run the "
           "wavefront pipeline only";
  if ((q->flags & RPT_FLAG_RAYS_PERSISTENT) && (q->flags & RPT_FLAG_WAVEFRONT))
    return "RptProbeQuery: RPT_FLAG_RAYS_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes";
  return nullptr;
}

namespace {

// on_device: positions, normals, streams and out are device pointers (user_stream: the stream their producer ran on)
int bake_probes(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                const RptProbeQuery* q, double* out, bool on_device, hipStream_t user_stream) {
  // (the query first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_probe_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!positions || !out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (n && q->kind == RPT_PROBE_IRRADIANCE && !normals)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null normals: RPT_PROBE_IRRADIANCE gathers about each probe's normal");
  if (!streams && n > (1ull << 32))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "more than 2^32 probes without stream ids (a stream id has 32 bits)");
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
    const bool with_normals = q->kind == RPT_PROBE_IRRADIANCE;
    const uint32_t width = probe_width(q->kind);
    if (user_stream) HIP_TRY(hipStreamSynchronize(user_stream));
    h->dscene.force_general = (q->flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
    RptRenderParams p{}; // what render_wavefront reads of it
    p.max_bounces = q->max_bounces; p.iterations = q->samples; p.seed = q->seed;
    p.sample_index_base = q->sample_index_base; p.precision_mode = q->precision_mode; p.flags = q->flags;
    // the piece: whole probes, at most the paths one pass may hold with every level of every path — a pass is at least
    // one sample of every probe of the piece (rptplan::rays_piece, as it stands)
    rptplan::PassInput in = pass_input(h, 1, q->samples);
    in.remaining = q->samples;
    in.ratio = (double)q->max_bounces + 1.0;
    pass_input_now(h, in);
    uint64_t asked = 0; // tests: pieces of a few probes
    if (const char* e = std::getenv("RPTGPU_PROBES_PIECE")) asked = std::strtoull(e, nullptr, 10);
    uint64_t piece = rptplan::rays_piece(n, asked, rptplan::plan_pass(in).target);
    // the persistent kernel on request, as in api_rays.cpp: not for a scene only the wavefront pipeline walks, and in
    // pieces a launch's work counter holds
    const bool persistent = (q->flags & RPT_FLAG_RAYS_PERSISTENT) && !use_wavefront(h, 0, false);
    if (persistent) piece = handle_rays_persistent_piece(h, piece, q->samples);
    h->accum.alloc((uint64_t)width * piece);
    if (!on_device) {
      h->rays_o.alloc(3 * piece);
      if (with_normals) h->rays_d.alloc(3 * piece);
      h->rays_out.alloc((uint64_t)width * piece);
    }
    if (!on_device || !streams) h->ray_ids.alloc(piece);
    const double scale = (with_normals ? 3.141592653589793 : 12.566370614359172) / (double)q->samples;
    for (uint64_t base = 0; base < n; base += piece) {
      const uint64_t m = std::min(piece, n - base);
      const double *d_pos = positions + 3 * base, *d_nrm = with_normals ? normals + 3 * base : nullptr;
      const uint32_t* d_ids = streams ? streams + base : h->ray_ids.p;
      double* d_out = out + (uint64_t)width * base;
      if (!on_device) {
        HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_pos, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
        if (with_normals) HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_nrm, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
        if (streams) HIP_TRY(hipMemcpyAsync(h->ray_ids.p, d_ids, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        d_pos = h->rays_o.p; d_nrm = with_normals ? h->rays_d.p : nullptr; d_ids = h->ray_ids.p; d_out = h->rays_out.p;
      }
      rptdev::Frame fr{};
      fr.width = (uint32_t)m; fr.height = 1; fr.npix = (uint32_t)m; fr.pixels = d_ids;
      fr.max_bounces = q->max_bounces; fr.seed = q->seed; fr.accum = h->accum.p;
      RaySource src{nullptr, d_pos, d_nrm, 0u, (uint32_t)base, streams ? nullptr : h->ray_ids.p};
      src.probe = (int)q->kind; src.probe_scale = scale;
      if (persistent) { // (the ids the wavefront's first step would write: the kernel reads them from the first launch on)
        if (!streams) kt->rays_ids(st, (uint32_t)base, (uint32_t)m, h->ray_ids.p);
        render_persistent(h, kt, p, fr, src, d_out, false, true, prof);
      } else {
        render_wavefront(h, kt, p, fr, src, d_out, false, true, prof);
      }
      HIP_TRY(hipGetLastError());
      if (!on_device) { // the staging arrays are the next piece's, too
        HIP_TRY(hipMemcpyAsync(out + (uint64_t)width * base, d_out, (uint64_t)width * m * sizeof(double), hipMemcpyDeviceToHost, st));
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

int rptgpu_bake_probes(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                       const RptProbeQuery* q, double* out) {
  return bake_probes(h, n, positions, normals, streams, q, out, false, nullptr);
}

int rptgpu_bake_probes_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals, const void* d_streams,
                              const RptProbeQuery* q, void* d_out, void* stream) {
  return bake_probes(h, n, (const double*)d_positions, (const double*)d_normals, (const uint32_t*)d_streams, q, (double*)d_out, true,
                     (hipStream_t)stream);
}

} // extern "C"
