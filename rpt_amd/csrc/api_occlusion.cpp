// api_occlusion.cpp — rptgpu_occluded[_device] and rptgpu_bake_ao[_device]: visibility for the caller (include/rpt_gpu.h,
// DESIGN.md §16; see api_internal.h).  Both lay rays where a depth's shadow rays of "light" 0 lie (kernels/occlusion.inc:
// rpt_occ_load for a piece of the caller's rays, rpt_raygen_ao for a piece of points x a pass's directions) and run ONE
// visibility query of a render over them — rpt_shadow_rays with one light for scenes walked in-kernel, query_visibility(...,
// 0, ...) for scenes with deep trees, chosen as render_wavefront's run_pass chooses —, then read column 0 of srt back:
// rpt_occ_store as bytes, rpt_ao_fold into the points' running sums.  No closest-hit query, no rpt_shade, no records: the
// workspace is asked for with one record column.  Pieces and passes: rptplan::occlusion_piece / ao_piece / ao_pass_samples.
#include "api_internal.h"

namespace rptapi {

static const char* const OCC_PERSISTENT =
    "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; visibility queries run the wavefront "
    "pipeline's shadow-ray query only";

// what is wrong with an RptVisibilityQuery / RptAoQuery (nullptr: nothing)
static const char* bad_visibility_query(const RptVisibilityQuery* q) {
  if (!q) return "null RptVisibilityQuery";
  if (q->struct_size != sizeof(RptVisibilityQuery)) return "RptVisibilityQuery: struct_size is not sizeof(RptVisibilityQuery)";
  if (q->reserved) return "RptVisibilityQuery: reserved != 0";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT) return OCC_PERSISTENT;
  return nullptr;
}
static const char* bad_ao_query(const RptAoQuery* q) {
  if (!q) return "null RptAoQuery";
  if (q->struct_size != sizeof(RptAoQuery)) return "RptAoQuery: struct_size is not sizeof(RptAoQuery)";
  if (!q->samples) return "RptAoQuery: samples == 0";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT) return OCC_PERSISTENT;
  return nullptr;
}

namespace {

// on_device: origins, dirs, max_t and out are device pointers (user_stream: the stream their producer ran on)
int occluded(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const double* max_t,
             const RptVisibilityQuery* q, uint8_t* out, bool on_device, hipStream_t user_stream) {
  // (the query first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_visibility_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!origins || !dirs || !out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    Occlusion oc(h, q->precision_mode, q->flags, "RPTGPU_OCCLUSION_PIECE");
    const uint64_t piece = rptplan::occlusion_piece(n, oc.asked, oc.pass_target);
    const rptdev::PathState ps = oc.workspace(piece);
    if (!on_device) {
      h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); h->occ_out.alloc(piece);
      if (max_t) h->rays_out.alloc(piece);
    }
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const double *d_o = origins + 3 * base, *d_d = dirs + 3 * base, *d_t = max_t ? max_t + base : nullptr;
      uint8_t* d_out = out + base;
      if (!on_device) {
        HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_o, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_d, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        if (max_t) HIP_TRY(hipMemcpyAsync(h->rays_out.p, d_t, (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        d_o = h->rays_o.p; d_d = h->rays_d.p; d_t = max_t ? h->rays_out.p : nullptr; d_out = h->occ_out.p;
      }
      oc.kt->occ_load(st, d_o, d_d, d_t, ps, h->shadow_q.p, oc.queue_length(), m);
      oc.query(ps, m);
      oc.kt->occ_store(st, ps, h->srt.p, m, d_out);
      HIP_TRY(hipGetLastError());
      if (!on_device) { // the staging arrays are the next piece's, too
        HIP_TRY(hipMemcpyAsync(out + base, d_out, m, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return h->has_deep && h->gen_overflow.p;
  });
}

} // namespace

// rptgpu_bake_ao's device work, behind its checks (n > 0): the body of its device_call, which rptgpu_bake_lightmap runs
// inside its own (api_lightmap.cpp) -> drain_call's read_overflow
bool enqueue_ao(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                const RptAoQuery* q, double* out_ao, double* out_bent, bool on_device) {
  hipStream_t st = h->stream;
  Occlusion oc(h, q->precision_mode, q->flags, "RPTGPU_OCCLUSION_PIECE");
  const uint32_t S = q->samples;
  const uint64_t piece = rptplan::ao_piece(n, oc.asked, S, oc.pass_target);
  // (a pass of m <= piece points holds m * ao_pass_samples(m, ...) <= min(m * S, the pass bound) slots)
  const rptdev::PathState ps = oc.workspace(std::min<uint64_t>(piece * S, rptplan::occlusion_pass_max(oc.pass_target)));
  h->accum.alloc(4 * piece); // per point: the count of visible directions and their sum, [4][points] (rpt_ao_fold)
  if (!on_device) {
    h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); h->rays_out.alloc(4 * piece);
    if (streams) h->ray_ids.alloc(piece);
  }
  for (uint64_t base = 0; base < n; base += piece) {
    const uint64_t m = std::min(piece, n - base);
    const double *d_pos = positions + 3 * base, *d_nrm = normals + 3 * base;
    const uint32_t* d_ids = streams ? streams + base : nullptr;
    double *d_ao = out_ao + base, *d_bent = out_bent ? out_bent + 3 * base : nullptr;
    if (!on_device) {
      HIP_TRY(hipMemcpyAsync(h->rays_o.p, d_pos, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(h->rays_d.p, d_nrm, 3 * m * sizeof(double), hipMemcpyHostToDevice, st));
      if (streams) HIP_TRY(hipMemcpyAsync(h->ray_ids.p, d_ids, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      d_pos = h->rays_o.p; d_nrm = h->rays_d.p; d_ids = streams ? h->ray_ids.p : nullptr;
      d_ao = h->rays_out.p; d_bent = out_bent ? h->rays_out.p + piece : nullptr;
    }
    rptdev::Frame fr{};
    fr.width = (uint32_t)m; fr.height = 1; fr.npix = (uint32_t)m; fr.seed = q->seed; fr.accum = h->accum.p;
    for (uint32_t s0 = 0; s0 < S;) { // the piece's passes: s_pass directions of every point
      const uint32_t s_pass = rptplan::ao_pass_samples(m, S - s0, oc.pass_target);
      const uint32_t n_slots = (uint32_t)(m * s_pass);
      fr.sample_base = q->sample_index_base + s0;
      oc.kt->raygen_ao(st, fr, d_pos, d_nrm, d_ids, (uint32_t)base, q->max_distance, ps, h->shadow_q.p, oc.queue_length(), n_slots);
      oc.query(ps, n_slots);
      oc.kt->ao_fold(st, fr, ps, h->srt.p, s_pass, s0 == 0, s0 + s_pass == S, S, d_ao, d_bent);
      HIP_TRY(hipGetLastError());
      s0 += s_pass;
    }
    if (!on_device) { // the staging arrays are the next piece's, too
      HIP_TRY(hipMemcpyAsync(out_ao + base, d_ao, m * sizeof(double), hipMemcpyDeviceToHost, st));
      if (out_bent) HIP_TRY(hipMemcpyAsync(out_bent + 3 * base, d_bent, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
  }
  return h->has_deep && h->gen_overflow.p;
}

namespace {

// on_device: positions, normals, streams and both outputs are device pointers
int bake_ao(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
            const RptAoQuery* q, double* out_ao, double* out_bent, bool on_device, hipStream_t user_stream) {
  if (const char* why = bad_ao_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!positions || !normals || !out_ao)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!streams && n > (1ull << 32))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "more than 2^32 points without stream ids (a stream id has 32 bits)");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() { return enqueue_ao(h, n, positions, normals, streams, q, out_ao, out_bent, on_device); });
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_occluded(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const double* max_t,
                    const RptVisibilityQuery* q, uint8_t* out) {
  return occluded(h, n, origins, dirs, max_t, q, out, false, nullptr);
}

int rptgpu_occluded_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, const void* d_max_t,
                           const RptVisibilityQuery* q, void* d_out, void* stream) {
  return occluded(h, n, (const double*)d_origins, (const double*)d_dirs, (const double*)d_max_t, q, (uint8_t*)d_out, true,
                  (hipStream_t)stream);
}

int rptgpu_bake_ao(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals, const uint32_t* streams,
                   const RptAoQuery* q, double* out_ao, double* out_bent) {
  return bake_ao(h, n, positions, normals, streams, q, out_ao, out_bent, false, nullptr);
}

int rptgpu_bake_ao_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals, const void* d_streams,
                          const RptAoQuery* q, void* d_out_ao, void* d_out_bent, void* stream) {
  return bake_ao(h, n, (const double*)d_positions, (const double*)d_normals, (const uint32_t*)d_streams, q, (double*)d_out_ao,
                 (double*)d_out_bent, true, (hipStream_t)stream);
}

} // extern "C"
