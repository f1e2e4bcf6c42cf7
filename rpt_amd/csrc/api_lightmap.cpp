// api_lightmap.cpp — rptgpu_bake_lightmap[_device]: a lightmap from a mesh's UV charts (include/rpt_gpu_lightmap.h, DESIGN.md
// §22; see api_internal.h).  The call: rpt_lightmap_owners rasterises the triangles into the owner map, which stays for the
// whole call; then per piece of consecutive texels (lightmap_plan.h piece: the probe call's pass bound) a scan of the owned
// flags, rpt_lightmap_texels — the raw channels, and the owned texels' gather points, normals and stream ids compacted in
// texel order —, the count read back, the device work of rptgpu_bake_probes and rptgpu_bake_ao over the compacted arrays
// (enqueue_probes, enqueue_ao: their drivers, not copies) and rpt_lightmap_scatter; at the end rpt_lightmap_dilate, one launch
// per round and channel over the whole map.  A device caller's arrays are written where they lie; a host caller's triangles
// and named channels are staged whole in arrays the handle keeps (RptLightmapArrays' channel table: lightmap_plan.h ROWS,
// channel_plan.h).
// rptgpu_bake_lightmap_direct[_device] (include/rpt_gpu_direct.h; the entry points: api_direct.cpp) is the same
// pipeline — run_lightmap — with rptgpu_bake_direct's device work, enqueue_direct, as the one gather of its one channel.
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t LIGHTMAP_ALL = RPT_LIGHTMAP_IRRADIANCE | RPT_LIGHTMAP_AO | RPT_LIGHTMAP_OWNER | RPT_LIGHTMAP_BARYCENTRIC |
                                  RPT_LIGHTMAP_POSITION | RPT_LIGHTMAP_NORMAL;
constexpr uint32_t LIGHTMAP_GATHERS = RPT_LIGHTMAP_IRRADIANCE | RPT_LIGHTMAP_AO;

// what is wrong with an RptLightmapQuery (nullptr: nothing)
static const char* bad_lightmap_query(const RptLightmapQuery* q) {
  if (const char* why = bad_channel_query(q, RPT_QUERY_TEXTS(RptLightmapQuery, RPT_LIGHTMAP), LIGHTMAP_ALL)) return why;
  if (!q->width || !q->height) return "RptLightmapQuery: width == 0 or height == 0";
  if (!rptlightmap::streams_fit(q->width, q->height, q->stream_base))
    return "RptLightmapQuery: width * height + stream_base > 2^32 (a texel's stream id has 32 bits)";
  if ((q->channels & LIGHTMAP_GATHERS) && !q->samples)
    return "RptLightmapQuery: samples == 0 with RPT_LIGHTMAP_IRRADIANCE or RPT_LIGHTMAP_AO named";
  if (q->max_bounces > 254) return "RptLightmapQuery: max_bounces > 254";
  if (!std::isfinite(q->offset)) return "RptLightmapQuery: offset is not finite";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a lightmap's gathers run the probe "
           "and the ambient-occlusion calls' drivers";
  if ((q->flags & RPT_FLAG_RAYS_PERSISTENT) && (q->flags & RPT_FLAG_WAVEFRONT))
    return "RptLightmapQuery: RPT_FLAG_RAYS_PERSISTENT | RPT_FLAG_WAVEFRONT — the two flags name different routes";
  return nullptr;
}

namespace {

// `rounds` rounds of the dilation over the map's IRRADIANCE and AO (nullptr: not named), with the filled flags of the call
// — flags: two arrays of n, [0] the state before the first round.  Each round is one launch per channel from the round's
// source into its destination (the ping-pong: the map and the handle's second copy), both reading the same flags, the
// first writing the next ones; what ended in the copy goes back into the map
void dilate_map(rptgpu_scene* h, uint32_t width, uint32_t height, uint32_t rounds, double* irradiance, double* ao, uint8_t* flags) {
  const uint64_t n = rptlightmap::texels(width, height);
  double *s3 = irradiance, *d3 = h->lm_pong.p, *s1 = ao, *d1 = h->lm_pong.p + (irradiance ? 3 * n : 0);
  for (uint32_t r = 0; r < rounds; r++) {
    uint8_t *fsrc = flags + (r % 2) * n, *fdst = flags + ((r + 1) % 2) * n;
    if (irradiance) {
      HIP_TRY(rptlightmap::dilate(h->stream, width, height, 3, s3, fsrc, d3, fdst));
      std::swap(s3, d3);
    }
    if (ao) {
      HIP_TRY(rptlightmap::dilate(h->stream, width, height, 1, s1, fsrc, d1, irradiance ? nullptr : fdst));
      std::swap(s1, d1);
    }
  }
  if (irradiance && s3 != irradiance) HIP_TRY(hipMemcpyAsync(irradiance, s3, 3 * n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (ao && s1 != ao) HIP_TRY(hipMemcpyAsync(ao, s1, n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}

// the checks both forms of the call make behind their query and arrays
int bad_lightmap_call(rptgpu_scene* h, uint64_t n_tris, const double* positions, const double* uvs) {
  if (n_tris > rptlightmap::TRIS_MAX) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "more than 2^31 - 1 triangles (an owner is an int32)");
  if (n_tris && (!positions || !uvs)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  return RPTGPU_OK;
}

// The pipeline behind the checks.  ch: the channels to make, theirs: the caller's arrays for them.  direct: the gather of the
// IRRADIANCE slot — the only channel then — is enqueue_direct instead of enqueue_probes (rptgpu_bake_lightmap_direct: q's
// channels, max_bounces and max_distance are not read)
int run_lightmap(rptgpu_scene* h, uint64_t n_tris, const double* positions, const double* normals, const double* uvs,
                 const RptLightmapQuery* q, uint32_t ch, const ChannelPtrs& theirs, bool direct, bool on_device,
                 hipStream_t user_stream) {
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const uint32_t W = q->width, H = q->height, max_bounces = direct ? 0u : q->max_bounces;
    const uint64_t n = rptlightmap::texels(W, H);
    const bool irr = (ch & RPT_LIGHTMAP_IRRADIANCE) != 0, ao = (ch & RPT_LIGHTMAP_AO) != 0, gather = irr || ao;
    bool overflow = false;

    // the triangles on the device
    rptlightmap::Triangles tris{positions, normals, uvs, (uint32_t)n_tris};
    if (!on_device && n_tris) {
      const uint64_t wp = 9 * n_tris, wn = normals ? 9 * n_tris : 0, wu = 6 * n_tris;
      h->lm_tris.alloc(wp + wn + wu);
      double* d = h->lm_tris.p;
      HIP_TRY(hipMemcpyAsync(d, positions, wp * sizeof(double), hipMemcpyHostToDevice, st));
      if (normals) HIP_TRY(hipMemcpyAsync(d + wp, normals, wn * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d + wp + wn, uvs, wu * sizeof(double), hipMemcpyHostToDevice, st));
      tris.positions = d; tris.normals = normals ? d + wp : nullptr; tris.uvs = d + wp + wn;
    }
    // where the map's channels lie on the device: the caller's arrays, or the handle's staging
    ChannelPtrs map = theirs;
    if (!on_device) {
      const rptchan::Layout lay = rptchan::layout(rptlightmap::ROWS, ch, n);
      h->lm_stage.alloc(lay.words);
      map = ptrs_in(h->lm_stage.p, lay);
    }
    // (a channel that is not named: nullptr)
    double *const map_irr = map.at<double>(rptlightmap::R_IRRADIANCE), *const map_ao = map.at<double>(rptlightmap::R_AO);

    // 1. the owner map
    h->lm_owner.alloc(n);
    h->lm_large.alloc(1 + n_tris);
    HIP_TRY(rptlightmap::owners(st, tris, W, H, h->lm_owner.p, h->lm_large.p));

    // 2. the pieces
    uint64_t asked = 0; // tests: pieces of a few texels
    if (const char* e = std::getenv("RPTGPU_LIGHTMAP_PIECE")) asked = std::strtoull(e, nullptr, 10);
    const uint64_t fit = gather ? std::min<uint64_t>(piece_pass_target(h, q->samples, max_bounces), RPT_MAX_PATHS_PER_PASS)
                                : rptlightmap::PIECE_MAX;
    const uint64_t piece = rptlightmap::piece(n, asked, fit);
    const rptlightmap::Compact lay = rptlightmap::compact(piece, irr, ao);
    size_t scan_bytes = 0;
    double *c_point = nullptr, *c_normal = nullptr, *c_irr = nullptr, *c_ao = nullptr;
    uint32_t* c_ids = nullptr;
    if (gather) {
      // (one scratch for every piece: what the full piece asks for and, should rocPRIM ever ask more for fewer items,
      // what the shorter last piece asks for)
      size_t tail_bytes = 0;
      HIP_TRY(rptlightmap::scan_bytes(piece, &scan_bytes));
      if (n % piece) HIP_TRY(rptlightmap::scan_bytes(n % piece, &tail_bytes));
      scan_bytes = std::max(scan_bytes, tail_bytes);
      h->lm_scan_tmp.alloc(scan_bytes);
      h->lm_scan.alloc(piece);
      h->lm_compact.alloc(lay.words);
      c_point = h->lm_compact.p + lay.point; c_normal = h->lm_compact.p + lay.normal;
      c_ids = (uint32_t*)(h->lm_compact.p + lay.ids);
      if (irr) c_irr = h->lm_compact.p + lay.irradiance;
      if (ao) c_ao = h->lm_compact.p + lay.ao;
    }
    RptProbeQuery pq{};
    pq.struct_size = sizeof(RptProbeQuery); pq.kind = RPT_PROBE_IRRADIANCE; pq.samples = q->samples; pq.max_bounces = max_bounces;
    pq.seed = q->seed; pq.sample_index_base = q->sample_index_base; pq.precision_mode = q->precision_mode; pq.flags = q->flags;
    RptAoQuery aq{};
    aq.struct_size = sizeof(RptAoQuery); aq.samples = q->samples; aq.seed = q->seed; aq.sample_index_base = q->sample_index_base;
    aq.max_distance = q->max_distance; aq.precision_mode = q->precision_mode;
    aq.flags = q->flags & ~(uint32_t)RPT_FLAG_RAYS_PERSISTENT; // (the AO gather has no persistent form: the same bits)
    RptDirectQuery dq{};
    dq.struct_size = sizeof(RptDirectQuery); dq.samples = q->samples; dq.seed = q->seed; dq.sample_index_base = q->sample_index_base;
    dq.precision_mode = q->precision_mode; dq.flags = q->flags & ~(uint32_t)RPT_FLAG_RAYS_PERSISTENT;
    const rptlightmap::RawOut raw{map.at<int32_t>(rptlightmap::R_OWNER), map.at<double>(rptlightmap::R_BARYCENTRIC),
                                  map.at<double>(rptlightmap::R_POSITION), map.at<double>(rptlightmap::R_NORMAL)};
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)rptlightmap::piece_len(base, n, piece);
      if (gather) HIP_TRY(rptlightmap::scan_owned(st, h->lm_owner.p, base, m, h->lm_scan.p, h->lm_scan_tmp.p, scan_bytes));
      HIP_TRY(rptlightmap::texels(st, tris, W, H, q->offset, q->stream_base, h->lm_owner.p, base, m, raw,
                                  gather ? h->lm_scan.p : nullptr, c_point, c_normal, c_ids));
      if (!gather) continue;
      uint32_t owned = 0; // the piece's owned texels: the scan's last entry
      HIP_TRY(hipMemcpyAsync(&owned, h->lm_scan.p + (m - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (owned) {
        if (direct) overflow |= enqueue_direct(h, owned, c_point, c_normal, c_ids, &dq, c_irr, true);
        else if (irr) overflow |= enqueue_probes(h, owned, c_point, c_normal, c_ids, &pq, c_irr, true);
        if (ao) overflow |= enqueue_ao(h, owned, c_point, c_normal, c_ids, &aq, c_ao, nullptr, true);
      }
      if (irr) HIP_TRY(rptlightmap::scatter(st, h->lm_owner.p, base, m, h->lm_scan.p, c_irr, 3, map_irr));
      if (ao) HIP_TRY(rptlightmap::scatter(st, h->lm_owner.p, base, m, h->lm_scan.p, c_ao, 1, map_ao));
    }

    // 3. the gutters
    // (after max(W, H) rounds every texel of a map with an owner is filled, and a round over a full map, or over one
    // without an owner, changes nothing: more rounds than that are the same bits)
    const uint32_t rounds = std::min(q->dilate, std::max(W, H));
    if (gather && rounds) {
      h->lm_filled.alloc(2 * n);
      h->lm_pong.alloc(((irr ? 3 : 0) + (ao ? 1 : 0)) * n);
      HIP_TRY(rptlightmap::filled_from_owner(st, h->lm_owner.p, n, h->lm_filled.p));
      dilate_map(h, W, H, rounds, map_irr, map_ao, h->lm_filled.p);
    }
    if (!on_device) {
      copy_out(rptlightmap::ROWS, map, theirs, ch, n, st);
      HIP_TRY(hipStreamSynchronize(st));
    }
    return overflow;
  });
}

// on_device: positions, normals, uvs and out's arrays are device pointers (user_stream: the stream their producer ran on)
int bake_lightmap(rptgpu_scene* h, uint64_t n_tris, const double* positions, const double* normals, const double* uvs,
                  const RptLightmapQuery* q, const RptLightmapArrays* out, bool on_device, hipStream_t user_stream) {
  // (the query first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_lightmap_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_channel_arrays(out, RPT_ARRAYS_TEXTS(RptLightmapArrays), rptlightmap::ROWS, q->channels))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const int rc = bad_lightmap_call(h, n_tris, positions, uvs)) return rc;
  return run_lightmap(h, n_tris, positions, normals, uvs, q, q->channels, ptrs_at(rptlightmap::ROWS, out, q->channels, 0), false, on_device,
                      user_stream);
}

} // namespace

// what is wrong with the RptLightmapQuery of rptgpu_bake_lightmap_direct, which reads neither channels nor max_bounces nor
// max_distance (nullptr: nothing)
static const char* bad_lightmap_direct_query(const RptLightmapQuery* q) {
  if (!q) return "null RptLightmapQuery";
  if (q->struct_size != sizeof(RptLightmapQuery)) return "RptLightmapQuery: struct_size is not sizeof(RptLightmapQuery)";
  if (!q->width || !q->height) return "RptLightmapQuery: width == 0 or height == 0";
  if (!rptlightmap::streams_fit(q->width, q->height, q->stream_base))
    return "RptLightmapQuery: width * height + stream_base > 2^32 (a texel's stream id has 32 bits)";
  if (!q->samples) return "RptLightmapQuery: samples == 0";
  if (!std::isfinite(q->offset)) return "RptLightmapQuery: offset is not finite";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a lightmap's direct light runs the "
           "wavefront pipeline's shadow-ray query only";
  return nullptr;
}

int bake_lightmap_direct(rptgpu_scene* h, uint64_t n_tris, const double* positions, const double* normals, const double* uvs,
                         const RptLightmapQuery* q, double* direct, bool on_device, hipStream_t user_stream) {
  if (const char* why = bad_lightmap_direct_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!direct) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null out");
  if (const int rc = bad_lightmap_call(h, n_tris, positions, uvs)) return rc;
  ChannelPtrs theirs{};
  theirs.p[rptlightmap::R_IRRADIANCE] = (char*)direct;
  return run_lightmap(h, n_tris, positions, normals, uvs, q, RPT_LIGHTMAP_IRRADIANCE, theirs, true, on_device, user_stream);
}

} // namespace rptapi

extern "C" {

int rptgpu_bake_lightmap(rptgpu_scene* h, uint64_t n_tris, const double* positions, const double* normals, const double* uvs,
                         const RptLightmapQuery* q, const RptLightmapArrays* out) {
  return bake_lightmap(h, n_tris, positions, normals, uvs, q, out, false, nullptr);
}

int rptgpu_bake_lightmap_device(rptgpu_scene* h, uint64_t n_tris, const void* d_positions, const void* d_normals, const void* d_uvs,
                                const RptLightmapQuery* q, const RptLightmapArrays* d_out, void* stream) {
  return bake_lightmap(h, n_tris, (const double*)d_positions, (const double*)d_normals, (const double*)d_uvs, q, d_out, true,
                       (hipStream_t)stream);
}

} // extern "C"
