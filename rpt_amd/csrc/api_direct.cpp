// api_direct.cpp — rptgpu_bake_direct[_device] and rptgpu_bake_lightmap_direct[_device]: direct light at points the caller
// chooses (include/rpt_gpu_direct.h; see api_internal.h).  sample_lights without a hit in front of it, in
// rptgpu_bake_ao's pieces and passes: per pass rpt_raygen_direct lays every light's sample of every (sample, point) slot
// where a depth's shadow rays of that light lie and queues the slots whose light can add something, the queues' lengths come
// back as they do behind rpt_shade, the visibility queries of a render run over them — ONE rpt_shadow_rays launch with the
// light as the grid's y for scenes walked in-kernel, query_visibility per light for scenes with deep trees (Occlusion) — and
// rpt_direct_fold adds the answers into the points' running sums, sample by sample and light by light.  The lightmap form is
// api_lightmap.cpp's pipeline with enqueue_direct as its gather.
#include "api_internal.h"

namespace rptapi {

static const char* bad_direct_query(const RptDirectQuery* q) {
  if (!q) return "null RptDirectQuery";
  if (q->struct_size != sizeof(RptDirectQuery)) return "RptDirectQuery: struct_size is not sizeof(RptDirectQuery)";
  if (!q->samples) return "RptDirectQuery: samples == 0";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; direct light at caller points runs the "
           "wavefront pipeline's shadow-ray query only";
  return nullptr;
}

// rptgpu_bake_direct's device work, behind its checks (n > 0): the body of its device_call -> drain_call's read_overflow
bool enqueue_direct(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                    const RptDirectQuery* q, double* out, bool on_device) {
  hipStream_t st = h->stream;
  const int nl = h->dscene.num_lights;
  const uint64_t casting = (uint64_t)h->dscene.num_shadow_lights; // the non-ambient lights
  if (!casting) { // nothing to sample: +0.0, and no query
    if (on_device) HIP_TRY(hipMemsetAsync(out, 0, 3 * n * sizeof(double), st));
    else std::fill(out, out + 3 * n, 0.0);
    return false;
  }
  Occlusion oc(h, q->precision_mode, q->flags, "RPTGPU_DIRECT_PIECE");
  const uint32_t S = q->samples;
  const uint64_t piece = rptplan::ao_piece(n, oc.asked, S, oc.pass_target);
  // (a pass of m <= piece points holds m * ao_pass_samples(m, ...) <= min(m * S, the pass bound) slots, each with every
  // light's shadow column: pass_input counts them)
  const rptdev::PathState ps = oc.workspace(std::min<uint64_t>(piece * S, rptplan::occlusion_pass_max(oc.pass_target)));
  h->accum.alloc(3 * piece); // per point: the running sum, [3][points] (rpt_direct_fold)
  if (!on_device) {
    h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); h->rays_out.alloc(3 * piece);
    if (streams) h->ray_ids.alloc(piece);
  }
  h->cnt_host.resize(2 + (size_t)nl);
  uint32_t* const cnt = h->cnt_host.data() + 2; // the queues' lengths on the host, beside oc.queue_length() on the device
  for (uint64_t base = 0; base < n; base += piece) {
    const uint64_t m = std::min(piece, n - base);
    const double *d_pos = positions + 3 * base, *d_nrm = normals + 3 * base;
    const uint32_t* d_ids = streams ? streams + base : nullptr;
    double* d_out = out + 3 * base;
    if (!on_device) {
      HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_pos, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_nrm, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
      if (streams) HIP_TRY(hipMemcpyAsync(h->ray_ids.p, d_ids, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      d_pos = h->rays_o.p; d_nrm = h->rays_d.p; d_ids = streams ? h->ray_ids.p : nullptr;
      d_out = h->rays_out.p;
    }
    rptdev::Frame fr{};
    fr.width = (uint32_t)m; fr.height = 1; fr.npix = (uint32_t)m; fr.seed = q->seed; fr.accum = h->accum.p;
    for (uint32_t s0 = 0; s0 < S;) { // the piece's passes: s_pass light samples of every point
      const uint32_t s_pass = rptplan::ao_pass_samples(m, S - s0, oc.pass_target);
      const uint32_t n_slots = (uint32_t)(m * s_pass);
      fr.sample_base = q->sample_index_base + s0;
      HIP_TRY(hipMemsetAsync(oc.queue_length(), 0, (size_t)nl * sizeof(uint32_t), st));
      oc.kt->raygen_direct(st, h->dscene, fr, d_pos, d_nrm, d_ids, (uint32_t)base, ps, h->shadow_q.p, h->counters.p, n_slots);
      // the queues' lengths, as behind rpt_shade: the queries are sized for the rays there are
      HIP_TRY(hipMemcpyAsync(cnt, oc.queue_length(), (size_t)nl * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      h->stats.shadow_rays += (uint64_t)n_slots * casting;
      h->stats.shadow_rays_traced += oc.query_lights(ps, cnt);
      oc.kt->direct_fold(st, h->dscene, fr, ps, h->srt.p, s_pass, s0 == 0, s0 + s_pass == S, S, d_out);
      HIP_TRY(hipGetLastError());
      s0 += s_pass;
    }
    if (!on_device) { // the staging arrays are the next piece's, too
      HIP_TRY(hipMemcpyAsync(out + 3 * base, d_out, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
  }
  return h->has_deep && h->gen_overflow.p;
}

namespace {

// on_device: positions, normals, streams and out are device pointers
int bake_direct(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                const RptDirectQuery* q, double* out, bool on_device, hipStream_t user_stream) {
  if (const char* why = bad_direct_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!positions || !normals || !out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!streams && n > (1ull << 32))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "more than 2^32 points without stream ids (a stream id has 32 bits)");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() { return enqueue_direct(h, n, positions, normals, streams, q, out, on_device); });
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_bake_direct(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                       const RptDirectQuery* q, double* out) {
  return bake_direct(h, n, positions, normals, streams, q, out, false, nullptr);
}

int rptgpu_bake_direct_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals, const void* d_streams,
                              const RptDirectQuery* q, void* d_out, void* stream) {
  return bake_direct(h, n, (const double*)d_positions, (const double*)d_normals, (const uint32_t*)d_streams, q, (double*)d_out,
                     true, (hipStream_t)stream);
}

int rptgpu_bake_lightmap_direct(rptgpu_scene* h, uint64_t n_tris, const double* positions, const double* normals,
                                const double* uvs, const RptLightmapQuery* q, double* out) {
  return bake_lightmap_direct(h, n_tris, positions, normals, uvs, q, out, false, nullptr);
}

int rptgpu_bake_lightmap_direct_device(rptgpu_scene* h, uint64_t n_tris, const void* d_positions, const void* d_normals,
                                       const void* d_uvs, const RptLightmapQuery* q, void* d_out, void* stream) {
  return bake_lightmap_direct(h, n_tris, (const double*)d_positions, (const double*)d_normals, (const double*)d_uvs, q,
                              (double*)d_out, true, (hipStream_t)stream);
}

} // extern "C"
