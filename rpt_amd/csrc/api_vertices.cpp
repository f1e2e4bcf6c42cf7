// api_vertices.cpp — rptgpu_trace_vertices[_device]: the vertices of the paths rptgpu_trace_rays runs (include/
// rpt_gpu_vertices.h; see api_internal.h).  The call runs api_rays.cpp's piece loop (trace_ray_pieces) — the
// same pieces through the same driver, the same rpt_raygen_rays, depth loop, restarts, rpt_resolve and rpt_finish — and adds,
// through the loop's two hooks, one thing to the piece's RaySource: the vertex sink.  run_pass (api_render.cpp) then launches
// rpt_vertices_store behind every depth's closest-hit query and rpt_vertices_fold at the end of every pass that resolved
// (kernels/wf_vertices.inc); the filler behind the paths' last vertices is laid down here, per piece, before its passes.  A
// host caller's records are staged piece by piece in an array the handle keeps (rptplan::vertices_piece bounds it) and copied
// out behind the piece; a device caller's are written where they lie.  RptVertexArrays' channel table: render_plan.h
// VERTEX_ROWS (channel_plan.h).
// Under RPT_FLAG_VERTICES_PERSISTENT (include/rpt_gpu_vertices_persistent.h) the same pieces, staged and
// filled the same way, go through the persistent driver instead: rpt_paths_vertices writes each vertex where it makes it, and
// rpt_sum_samples and the packed rpt_finish behind its launches are a render's.  The same bytes.
#include "api_internal.h"

namespace rptapi {
namespace {

constexpr uint32_t VERTEX_ALL = RPT_VERTEX_LENGTH | RPT_VERTEX_T | RPT_VERTEX_NORMAL | RPT_VERTEX_OBJECT | RPT_VERTEX_POSITION |
                                RPT_VERTEX_DIRECTION | RPT_VERTEX_DRAW | RPT_VERTEX_RADIANCE | RPT_VERTEX_BSDF |
                                RPT_VERTEX_INV_PDF | RPT_VERTEX_ABS_COS | RPT_VERTEX_RGB;
// render_plan.h counts a vertex's bytes by bit position
static_assert(RPT_VERTEX_LENGTH == 1u << 0 && RPT_VERTEX_T == 1u << 1 && RPT_VERTEX_NORMAL == 1u << 2 && RPT_VERTEX_OBJECT == 1u << 3 &&
              RPT_VERTEX_POSITION == 1u << 4 && RPT_VERTEX_DIRECTION == 1u << 5 && RPT_VERTEX_DRAW == 1u << 6 &&
              RPT_VERTEX_RADIANCE == 1u << 7 && RPT_VERTEX_BSDF == 1u << 8 && RPT_VERTEX_INV_PDF == 1u << 9 &&
              RPT_VERTEX_ABS_COS == 1u << 10 && RPT_VERTEX_RGB == 1u << 11 && VERTEX_ALL == (1u << rptplan::VERTICES_CHANNEL_BITS) - 1u,
              "rptplan::VERTICES_VERTEX_BYTES is indexed by the RPT_VERTEX_* bit positions");
static_assert(rptplan::vertices_vertex_bytes(VERTEX_ALL) == 152 && rptplan::vertices_path_bytes(VERTEX_ALL) == 4, "a vertex with every channel");

using rptplan::VERTEX_ROWS;
constexpr int N_ROWS = sizeof VERTEX_ROWS / sizeof VERTEX_ROWS[0];

// what is wrong with an RptVertexQuery / with the RptVertexArrays of a call that names `channels` (nullptr: nothing)
const char* bad_vertex_query(const RptVertexQuery* q) {
  const QueryTexts texts = RPT_QUERY_TEXTS(RptVertexQuery, RPT_VERTEX);
  if (const char* why = bad_query_struct(q, texts)) return why;
  if (!q->iterations) return "RptVertexQuery: iterations == 0";
  if (q->max_bounces > 254) return "RptVertexQuery: max_bounces > 254";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RptVertexQuery: RPT_FLAG_PERSISTENT — the persistent kernel keeps a path in registers and leaves no vertices behind; "
           "path vertices run the wavefront pipeline only";
  if (q->flags & RPT_FLAG_RAYS_PERSISTENT)
    return "RptVertexQuery: RPT_FLAG_RAYS_PERSISTENT — only rptgpu_trace_rays, rptgpu_bake_probes and their _device forms run "
           "in the persistent kernel, which leaves no vertices behind";
  if ((q->flags & RPT_FLAG_VERTICES_PERSISTENT) && (q->flags & RPT_FLAG_WAVEFRONT))
    return "RptVertexQuery: RPT_FLAG_VERTICES_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes";
  if (const char* why = bad_query_channels(*q, texts, VERTEX_ALL)) return why;
  if (q->reserved) return "RptVertexQuery: reserved != 0";
  return nullptr;
}
const char* bad_vertex_arrays(const RptVertexArrays* o, uint32_t ch) {
  if (const char* why = bad_channel_arrays(o, RPT_ARRAYS_TEXTS(RptVertexArrays), VERTEX_ROWS, ch)) return why;
  // (no row: rpt_finish writes the means through the ray call's own output; the highest bit, so the last check)
  if ((ch & RPT_VERTEX_RGB) && !o->rgb) return "RptVertexArrays: RPT_VERTEX_RGB is named but rgb is NULL";
  return nullptr;
}

// the kernels' struct from the arrays of VERTEX_ROWS, which stand in the order of its pointers
rptdev::VertexOut sink_of(const ChannelPtrs& p, const RptVertexQuery& q) {
  rptdev::VertexOut vo{};
  vo.length = (uint32_t*)p.p[0]; vo.t = (double*)p.p[1]; vo.normal = (double*)p.p[2]; vo.object = (int32_t*)p.p[3];
  vo.position = (double*)p.p[4]; vo.direction = (double*)p.p[5]; vo.draw = (uint32_t*)p.p[6]; vo.radiance = (double*)p.p[7];
  vo.bsdf = (double*)p.p[8]; vo.inv_pdf = (double*)p.p[9]; vo.abs_cos = (double*)p.p[10];
  vo.channels = q.channels; vo.iterations = q.iterations; vo.stride = q.max_bounces + 1u;
  return vo;
}

// on_device: origins, dirs, streams and out's arrays are device pointers (user_stream: the stream their producer ran on)
int trace_vertices(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const uint32_t* streams,
                   const RptVertexQuery* q, const RptVertexArrays* out, bool on_device, hipStream_t user_stream) {
  // (the query first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_vertex_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_vertex_arrays(out, q->channels)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!origins || !dirs)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!streams && n > (1ull << 32))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "more than 2^32 rays without stream ids (a stream id has 32 bits)");
  if (!rptplan::vertices_fit(n, q->iterations, q->max_bounces))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "n * iterations * (max_bounces + 1) does not fit: 2^56 vertices or more would not fit any memory");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const uint32_t ch = q->channels;
    const auto counts = [&](uint64_t rays) { return rptplan::vertex_counts(rays, q->iterations, q->max_bounces); };
    // the piece: rptgpu_trace_rays' (at most the paths one pass may hold with every level of every path), and for a host
    // caller what the staging of the named channels allows (rptplan::vertices_piece); in the persistent kernel also at most
    // what a launch's work counter holds (rptplan::vertices_persistent_piece is this composition)
    uint64_t asked = 0; // tests: pieces of a few rays
    if (const char* e = std::getenv("RPTGPU_VERTICES_PIECE")) asked = std::strtoull(e, nullptr, 10);
    uint64_t piece = rptplan::vertices_piece(n, asked, piece_pass_target(h, q->iterations, q->max_bounces), !on_device, q->iterations,
                                             q->max_bounces, ch);
    const bool persistent = piece_persistent(h, q->flags, RPT_FLAG_VERTICES_PERSISTENT);
    if (persistent) piece = persistent_piece(h, piece, q->iterations);
    ChannelPtrs stage{}, mine{};
    if (!on_device) { // a host caller's piece of records on the device
      const rptchan::Layout lay = rptchan::layout(VERTEX_ROWS, ch, counts(piece));
      h->vertices_out.alloc(lay.words);
      stage = ptrs_in(h->vertices_out.p, lay);
    }
    rptdev::VertexOut sink{};
    // rpt_finish writes a piece's means somewhere: the caller's rgb, or (RGB not named) the handle's array
    const RayPieces c{n, origins, dirs, streams, on_device, piece, persistent, piece_params(*q, q->iterations, q->exposure_value),
                      q->first_draw, 3, (ch & RPT_VERTEX_RGB) ? out->rgb : nullptr};
    trace_ray_pieces(
        h, c,
        [&](uint64_t base, uint64_t m, RaySource& src) {
          mine = ptrs_at(VERTEX_ROWS, out, ch, counts(base));
          const ChannelPtrs& where = on_device ? mine : stage;
          sink = sink_of(where, *q);
          src.vertices = &sink;
          // the filler — +0.0, OBJECT -1, DRAW 0 — over the piece's entries of every named per-vertex channel, in front of the
          // piece's first pass: the kernels write d < len only, so behind a path's last vertex this is what stays.  (Streaming
          // fills instead of 8- to 24-byte stores a path's stride apart: RPT_VERTICES_FILL_IN_KERNEL=1 builds that form.)
#if !RPT_VERTICES_FILL_IN_KERNEL
          for (int k = 0; k < N_ROWS; k++)
            if ((ch & VERTEX_ROWS[k].bit) && !VERTEX_ROWS[k].per_path)
              HIP_TRY(hipMemsetAsync(where.p[k], VERTEX_ROWS[k].bit == RPT_VERTEX_OBJECT ? 0xff : 0,
                                     rptchan::row_bytes(VERTEX_ROWS[k], counts(m)), st));
#endif
        },
        [&](uint64_t, uint64_t m) {
          if (!on_device) copy_out(VERTEX_ROWS, stage, mine, ch, counts(m), st);
        });
    return !persistent && h->has_deep && h->gen_overflow.p;
  });
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_trace_vertices(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const uint32_t* streams,
                          const RptVertexQuery* q, const RptVertexArrays* out) {
  return trace_vertices(h, n, origins, dirs, streams, q, out, false, nullptr);
}

int rptgpu_trace_vertices_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, const void* d_streams,
                                 const RptVertexQuery* q, const RptVertexArrays* d_out, void* stream) {
  return trace_vertices(h, n, (const double*)d_origins, (const double*)d_dirs, (const uint32_t*)d_streams, q, d_out, true,
                        (hipStream_t)stream);
}

int rptgpu_vertices_persistent_supported(void) { return 1; }

} // extern "C"
