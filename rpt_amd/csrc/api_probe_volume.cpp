// api_probe_volume.cpp — rptgpu_sample_probe_volume[_device], rptgpu_lookup_probe_volume[_device] and
// rptgpu_render_views_probe_lit[_device]: a grid of baked SH9 probes read at the caller's points, at the first hits of the
// caller's rays and in views shaded from lightmaps where bound (include/rpt_gpu_probe_volume.h; see
// api_internal.h).  Points: one kernel per piece, rpt_probe_volume_sample.  Rays: per piece rptgpu_first_hits' own query for T,
// OBJECT, NORMAL and POSITION (api_hits.cpp plan_hit_pieces / hit_piece), unchanged, into arrays the handle keeps, then
// rpt_probe_volume_lookup, one lane per ray (kernels/probe_volume.inc).  Views: rptgpu_render_views_lightmapped's own driver
// (api_lightmap_lookup.cpp render_views_lit) with a volume: NORMAL and POSITION added to the query's channels and
// rpt_views_probe_lit_merge (kernels/probe_volume_views.inc) in front of the fold.  The checks of a volume's numbers, the pieces and the sizes — a
// piece's arrays, a host caller's staging — and RptVolumeArrays' channel table are probe_volume_plan.h's.
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t VOLUME_ALL = RPT_VOLUME_T | RPT_VOLUME_OBJECT | RPT_VOLUME_POSITION | RPT_VOLUME_NORMAL | RPT_VOLUME_VALUE |
                                RPT_VOLUME_COVERED | RPT_VOLUME_INSIDE;
static_assert(rptvolume::CH_T == RPT_VOLUME_T && rptvolume::CH_OBJECT == RPT_VOLUME_OBJECT && rptvolume::CH_POSITION == RPT_VOLUME_POSITION &&
              rptvolume::CH_NORMAL == RPT_VOLUME_NORMAL && rptvolume::CH_VALUE == RPT_VOLUME_VALUE &&
              rptvolume::CH_COVERED == RPT_VOLUME_COVERED && rptvolume::CH_INSIDE == RPT_VOLUME_INSIDE && rptvolume::CH_ALL == VOLUME_ALL,
              "probe_volume_plan.h restates the header's channel bits");

namespace {

// what is wrong with an RptVolumeQuery of a call that knows the channels `known` / with an RptProbeVolume (nullptr: nothing)
const char* bad_volume_query(const RptVolumeQuery* q, uint32_t known) {
  if (const char* why = bad_channel_query(q, RPT_QUERY_TEXTS(RptVolumeQuery, RPT_VOLUME), VOLUME_ALL)) return why;
  if (q->channels & ~known)
    return "RptVolumeQuery: channels names a channel of the ray form (a point has VALUE, COVERED and INSIDE only)";
  if (!std::isfinite(q->normal_bias)) return "RptVolumeQuery: normal_bias is not finite";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a probe volume is read at points or "
           "behind the closest-hit query only";
  return nullptr;
}
const char* bad_volume(const RptProbeVolume* v) {
  if (!v) return "null RptProbeVolume";
  if (v->struct_size != sizeof(RptProbeVolume)) return "RptProbeVolume: struct_size is not sizeof(RptProbeVolume)";
  if (v->reserved) return "RptProbeVolume: reserved != 0";
  if (const char* why = rptvolume::bad_grid(v->nx, v->ny, v->nz, v->origin, v->spacing)) return why;
  if (!v->coeffs) return "RptProbeVolume: coeffs is NULL";
  bool fits;
  (void)rptvolume::probe_count(v->nx, v->ny, v->nz, fits);
  if (!fits) return "RptProbeVolume: nx * ny * nz probes do not fit: no allocation holds their coefficients";
  return nullptr;
}

} // namespace

// the volume as the kernels read it (bad_volume passed): a device caller's arrays as they are, a host caller's staged whole
rptvolume::Volume upload_volume(rptgpu_scene* h, const RptProbeVolume& v, double normal_bias, bool on_device) {
  rptvolume::Volume d{};
  d.nx = v.nx; d.ny = v.ny; d.nz = v.nz;
  for (int a = 0; a < 3; a++) { d.origin[a] = v.origin[a]; d.spacing[a] = v.spacing[a]; }
  d.normal_bias = normal_bias;
  if (on_device) {
    d.coeffs = v.coeffs; d.valid = v.valid;
    return d;
  }
  bool fits;
  const rptvolume::Staged s = rptvolume::stage_volume(rptvolume::probe_count(v.nx, v.ny, v.nz, fits), v.valid != nullptr);
  h->pv_stage.alloc(s.words);
  double* base = h->pv_stage.p;
  HIP_TRY(hipMemcpyAsync(base + s.coeffs, v.coeffs, s.coeff_words * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (v.valid) HIP_TRY(hipMemcpyAsync(base + s.valid, v.valid, s.valid_bytes, hipMemcpyHostToDevice, h->stream));
  d.coeffs = base + s.coeffs;
  d.valid = v.valid ? (const uint8_t*)(base + s.valid) : nullptr;
  return d;
}

uint64_t asked_volume_piece() { // tests: pieces of a few points
  if (const char* e = std::getenv("RPTGPU_VOLUME_PIECE")) return std::strtoull(e, nullptr, 10);
  return 0;
}

namespace {

// rays == false: a, b are the points and their directions; true: the rays' origins and directions.
// on_device: a, b, out's arrays and the volume's coeffs / valid are device pointers
int read_probe_volume(rptgpu_scene* h, bool rays, uint64_t n, const double* a, const double* b, const RptProbeVolume* volume,
                      const RptVolumeQuery* q, const RptVolumeArrays* out, bool on_device, hipStream_t user_stream) {
  // (the query, the volume, the arrays: refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_volume_query(q, rays ? VOLUME_ALL : rptvolume::CH_POINT)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_volume(volume)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_channel_arrays(out, RPT_ARRAYS_TEXTS(RptVolumeArrays), rptvolume::ROWS, q->channels))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!a || !b)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const uint32_t ch = q->channels;
    const KernelTable* kt = nullptr;
    HitPieces hp{};
    uint64_t piece;
    if (rays) {
      kt = table_for(q->precision_mode, h->ext_shapes);
      hp = plan_hit_pieces(h, n, q->flags, "RPTGPU_VOLUME_PIECE");
      piece = hp.piece;
    } else {
      piece = rptvolume::piece(n, asked_volume_piece(), rptvolume::POINTS_PIECE);
    }
    const bool prof = (q->flags & RPT_FLAG_PROFILE_KERNELS) != 0;
    const rptvolume::Layout lay = rptvolume::layout(piece, ch, rays, on_device);
    h->pv_piece.alloc(lay.words);
    const ChannelPtrs mine = ptrs_in(h->pv_piece.p, lay);
    if (!on_device) { h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); }
    const rptvolume::Volume dv = upload_volume(h, *volume, q->normal_bias, on_device);
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const double *d_a = a + 3 * base, *d_b = b + 3 * base;
      using namespace rptvolume; // (the rows of ROWS)
      const ChannelPtrs theirs = ptrs_at(ROWS, out, ch, base);
      if (!on_device) stage_rays(h, d_a, d_b, m);
      // where this piece's results go on the device: the caller's arrays (device callers), else the handle's
      const ChannelPtrs& dev = on_device ? theirs : mine;
      if (rays) {
        // 1. rptgpu_first_hits' query for T | OBJECT | NORMAL | POSITION, into the handle's arrays
        rptdev::HitOut ho{};
        ho.channels = RPT_HIT_T | RPT_HIT_OBJECT | RPT_HIT_NORMAL | RPT_HIT_POSITION;
        ho.t = mine.at<double>(R_T); ho.object = mine.at<int32_t>(R_OBJECT);
        ho.normal = mine.at<double>(R_NORMAL); ho.position = mine.at<double>(R_POSITION);
        hit_piece(h, kt, hp, d_a, d_b, m, ho, prof);
        // 2. the facing, the rule, the named channels (a host caller's four hit channels: in place)
        rptvolume::Hits r{};
        r.dirs = d_b; r.t = ho.t; r.object = ho.object; r.normal = ho.normal; r.position = ho.position;
        r.fallback[0] = q->fallback[0]; r.fallback[1] = q->fallback[1]; r.fallback[2] = q->fallback[2];
        r.channels = ch;
        r.o_t = dev.at<double>(R_T); r.o_object = dev.at<int32_t>(R_OBJECT);
        r.o_position = dev.at<double>(R_POSITION); r.o_normal = dev.at<double>(R_NORMAL);
        r.o_value = dev.at<double>(R_VALUE); r.o_covered = dev.at<uint8_t>(R_COVERED); r.o_inside = dev.at<uint8_t>(R_INSIDE);
        HIP_TRY(rptvolume::lookup(st, m, dv, r));
      } else {
        rptvolume::Points p{};
        p.positions = d_a; p.normals = d_b;
        p.fallback[0] = q->fallback[0]; p.fallback[1] = q->fallback[1]; p.fallback[2] = q->fallback[2];
        p.channels = ch;
        p.value = dev.at<double>(R_VALUE); p.covered = dev.at<uint8_t>(R_COVERED); p.inside = dev.at<uint8_t>(R_INSIDE);
        HIP_TRY(rptvolume::sample(st, m, dv, p));
      }
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_out(ROWS, mine, theirs, ch, m, st);
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return rays && h->has_deep && h->gen_overflow.p;
  });
}

// what is wrong with an RptViewsProbeLitQuery (nullptr: nothing)
const char* bad_views_probe_lit_query(const RptViewsProbeLitQuery* q) {
  if (!q) return "null RptViewsProbeLitQuery";
  if (q->struct_size != sizeof(RptViewsProbeLitQuery)) return "RptViewsProbeLitQuery: struct_size is not sizeof(RptViewsProbeLitQuery)";
  if (q->filter != RPT_LOOKUP_NEAREST && q->filter != RPT_LOOKUP_BILINEAR)
    return "RptViewsProbeLitQuery: filter is neither RPT_LOOKUP_NEAREST nor RPT_LOOKUP_BILINEAR";
  if (!std::isfinite(q->normal_bias)) return "RptViewsProbeLitQuery: normal_bias is not finite";
  return nullptr;
}

// rptgpu_render_views_lightmapped's driver (api_lightmap_lookup.cpp render_views_lit) with the volume's step: this call's own
// refusals — its query, then the volume — stand where that call's query's stand
int render_views_probe_lit(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* qv, uint32_t n_bindings,
                           const RptLightmapBinding* bindings, const RptProbeVolume* volume, const RptViewsProbeLitQuery* q,
                           double* out, bool on_device, hipStream_t user_stream) {
  const char* why = bad_views_probe_lit_query(q);
  if (!why) why = bad_volume(volume);
  ViewsLit lit{};
  if (!why) { lit.filter = q->filter; lit.unbound = q->unbound_irradiance; lit.volume = volume; lit.normal_bias = q->normal_bias; }
  return render_views_lit(h, n_views, views, qv, n_bindings, bindings, why, lit, out, on_device, user_stream);
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_sample_probe_volume(rptgpu_scene* h, uint64_t n, const double* positions, const double* normals,
                               const RptProbeVolume* volume, const RptVolumeQuery* q, const RptVolumeArrays* out) {
  return read_probe_volume(h, false, n, positions, normals, volume, q, out, false, nullptr);
}

int rptgpu_sample_probe_volume_device(rptgpu_scene* h, uint64_t n, const void* d_positions, const void* d_normals,
                                      const RptProbeVolume* d_volume, const RptVolumeQuery* q, const RptVolumeArrays* d_out, void* stream) {
  return read_probe_volume(h, false, n, (const double*)d_positions, (const double*)d_normals, d_volume, q, d_out, true, (hipStream_t)stream);
}

int rptgpu_lookup_probe_volume(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, const RptProbeVolume* volume,
                               const RptVolumeQuery* q, const RptVolumeArrays* out) {
  return read_probe_volume(h, true, n, origins, dirs, volume, q, out, false, nullptr);
}

int rptgpu_lookup_probe_volume_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs,
                                      const RptProbeVolume* d_volume, const RptVolumeQuery* q, const RptVolumeArrays* d_out, void* stream) {
  return read_probe_volume(h, true, n, (const double*)d_origins, (const double*)d_dirs, d_volume, q, d_out, true, (hipStream_t)stream);
}

int rptgpu_render_views_probe_lit(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                  uint32_t n_bindings, const RptLightmapBinding* bindings, const RptProbeVolume* volume,
                                  const RptViewsProbeLitQuery* q, double* out) {
  return render_views_probe_lit(h, n_views, views, q_views, n_bindings, bindings, volume, q, out, false, nullptr);
}

int rptgpu_render_views_probe_lit_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                         uint32_t n_bindings, const RptLightmapBinding* d_bindings, const RptProbeVolume* d_volume,
                                         const RptViewsProbeLitQuery* q, void* d_out, void* stream) {
  return render_views_probe_lit(h, n_views, views, q_views, n_bindings, d_bindings, d_volume, q, (double*)d_out, true, (hipStream_t)stream);
}

} // extern "C"
