// api_probes.cpp — rptgpu_bake_probes[_device]: light probes baked on the device (include/rpt_gpu.h; see
// api_internal.h).  A probe is `samples` paths whose first rays the library makes itself, so the call is rptgpu_trace_rays'
// with another first step and another last one, and runs api_rays.cpp's piece loop (trace_ray_pieces) with a probe kind in
// its description: the probes go through the wavefront driver of api_render.cpp in pieces of whole probes — a piece is the
// "frame" of its own passes, its probes are the pixels, the samples are the iterations —,
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

// the call's device work, behind its checks (n > 0): the body of its device_call, which rptgpu_bake_lightmap runs inside its
// own (api_lightmap.cpp) -> drain_call's read_overflow
bool enqueue_probes(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                    const RptProbeQuery* q, double* out, bool on_device) {
  const bool with_normals = q->kind == RPT_PROBE_IRRADIANCE;
  // the piece: whole probes, at most the paths one pass may hold with every level of every path — a pass is at least
  // one sample of every probe of the piece (rptplan::rays_piece, as it stands)
  uint64_t asked = 0; // tests: pieces of a few probes
  if (const char* e = std::getenv("RPTGPU_PROBES_PIECE")) asked = std::strtoull(e, nullptr, 10);
  uint64_t piece = rptplan::rays_piece(n, asked, piece_pass_target(h, q->samples, q->max_bounces));
  const bool persistent = piece_persistent(h, q->flags, RPT_FLAG_RAYS_PERSISTENT);
  if (persistent) piece = persistent_piece(h, piece, q->samples);
  const double scale = (with_normals ? 3.141592653589793 : 12.566370614359172) / (double)q->samples;
  // (the normals are staged and read for RPT_PROBE_IRRADIANCE only; a probe's streams start at draw 0, and it has no exposure)
  trace_ray_pieces(h, RayPieces{n, positions, with_normals ? normals : nullptr, streams, on_device, piece, persistent,
                                piece_params(*q, q->samples, 0.0), 0u, probe_width(q->kind), out, (int)q->kind, scale},
                   nullptr, nullptr);
  return !persistent && h->has_deep && h->gen_overflow.p;
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
  return device_call(h, user_stream, [&]() { return enqueue_probes(h, n, positions, normals, streams, q, out, on_device); });
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
