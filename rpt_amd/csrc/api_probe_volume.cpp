// api_probe_volume.cpp — rptgpu_sample_probe_volume[_device], rptgpu_lookup_probe_volume[_device] and
// rptgpu_render_views_probe_lit[_device]: a grid of baked SH9 probes read at the caller's points, at the first hits of the
// caller's rays and in views shaded from lightmaps where bound (include/rpt_gpu_probe_volume.h; see
// api_internal.h).  Points: one kernel per piece, rpt_probe_volume_sample.  Rays: per piece rptgpu_first_hits' own query for T,
// OBJECT, NORMAL and POSITION (api_hits.cpp plan_hit_pieces / hit_piece), unchanged, into arrays the handle keeps, then
// rpt_probe_volume_lookup, one lane per ray (kernels/probe_volume.inc).  Views: rptgpu_render_views_lightmapped's own driver
// (api_lightmap_lookup.cpp render_views_lit) with a volume: NORMAL and POSITION added to the query's channels and
// rpt_views_probe_lit_merge (kernels/probe_volume_views.inc) in front of the fold.  The checks of a volume's numbers, the pieces and the sizes — a
// piece's arrays, a host caller's staging — are probe_volume_plan.h's.
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t VOLUME_ALL = RPT_VOLUME_T | RPT_VOLUME_OBJECT | RPT_VOLUME_POSITION | RPT_VOLUME_NORMAL | RPT_VOLUME_VALUE |
                                RPT_VOLUME_COVERED | RPT_VOLUME_INSIDE;
static_assert(rptvolume::CH_T == RPT_VOLUME_T && rptvolume::CH_OBJECT == RPT_VOLUME_OBJECT && rptvolume::CH_POSITION == RPT_VOLUME_POSITION &&
              rptvolume::CH_NORMAL == RPT_VOLUME_NORMAL && rptvolume::CH_VALUE == RPT_VOLUME_VALUE &&
              rptvolume::CH_COVERED == RPT_VOLUME_COVERED && rptvolume::CH_INSIDE == RPT_VOLUME_INSIDE && rptvolume::CH_ALL == VOLUME_ALL,
              "probe_volume_plan.h restates the header's channel bits");

namespace {

// what is wrong with an RptVolumeQuery of a call that knows the channels `known` / with an RptProbeVolume / with the
// RptVolumeArrays of a call that names `channels` (nullptr: nothing)
const char* bad_volume_query(const RptVolumeQuery* q, uint32_t known) {
  if (!q) return "null RptVolumeQuery";
  if (q->struct_size != sizeof(RptVolumeQuery)) return "RptVolumeQuery: struct_size is not sizeof(RptVolumeQuery)";
  if (!q->channels) return "RptVolumeQuery: channels == 0 (name at least one RPT_VOLUME_* channel)";
  if (q->channels & ~VOLUME_ALL) return "RptVolumeQuery: channels names an unknown RPT_VOLUME_* bit";
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
const char* bad_volume_arrays(const RptVolumeArrays* o, uint32_t channels) {
  if (!o) return "null RptVolumeArrays";
  if (o->struct_size != sizeof(RptVolumeArrays)) return "RptVolumeArrays: struct_size is not sizeof(RptVolumeArrays)";
  if (o->reserved) return "RptVolumeArrays: reserved != 0";
  if ((channels & RPT_VOLUME_T) && !o->t) return "RptVolumeArrays: RPT_VOLUME_T is named but t is NULL";
  if ((channels & RPT_VOLUME_OBJECT) && !o->object) return "RptVolumeArrays: RPT_VOLUME_OBJECT is named but object is NULL";
  if ((channels & RPT_VOLUME_POSITION) && !o->position) return "RptVolumeArrays: RPT_VOLUME_POSITION is named but position is NULL";
  if ((channels & RPT_VOLUME_NORMAL) && !o->normal) return "RptVolumeArrays: RPT_VOLUME_NORMAL is named but normal is NULL";
  if ((channels & RPT_VOLUME_VALUE) && !o->value) return "RptVolumeArrays: RPT_VOLUME_VALUE is named but value is NULL";
  if ((channels & RPT_VOLUME_COVERED) && !o->covered) return "RptVolumeArrays: RPT_VOLUME_COVERED is named but covered is NULL";
  if ((channels & RPT_VOLUME_INSIDE) && !o->inside) return "RptVolumeArrays: RPT_VOLUME_INSIDE is named but inside is NULL";
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

// the arrays of a piece on the device, and the caller's
struct PieceArrays {
  double* t;
  int32_t* object;
  double* position;
  double* normal;
  double* value;
  uint8_t* covered;
  uint8_t* inside;
};
PieceArrays volume_arrays_at(const RptVolumeArrays& a, uint32_t ch, uint64_t base) {
  PieceArrays p{};
  if (ch & RPT_VOLUME_T) p.t = a.t + base;
  if (ch & RPT_VOLUME_OBJECT) p.object = a.object + base;
  if (ch & RPT_VOLUME_POSITION) p.position = a.position + 3 * base;
  if (ch & RPT_VOLUME_NORMAL) p.normal = a.normal + 3 * base;
  if (ch & RPT_VOLUME_VALUE) p.value = a.value + 3 * base;
  if (ch & RPT_VOLUME_COVERED) p.covered = a.covered + base;
  if (ch & RPT_VOLUME_INSIDE) p.inside = a.inside + base;
  return p;
}
PieceArrays volume_arrays_in(double* base, const rptvolume::Layout& l) {
  PieceArrays p{};
  if (l.has & RPT_VOLUME_T) p.t = base + l.t;
  if (l.has & RPT_VOLUME_OBJECT) p.object = (int32_t*)(base + l.object);
  if (l.has & RPT_VOLUME_POSITION) p.position = base + l.position;
  if (l.has & RPT_VOLUME_NORMAL) p.normal = base + l.normal;
  if (l.has & RPT_VOLUME_VALUE) p.value = base + l.value;
  if (l.has & RPT_VOLUME_COVERED) p.covered = (uint8_t*)(base + l.covered);
  if (l.has & RPT_VOLUME_INSIDE) p.inside = (uint8_t*)(base + l.inside);
  return p;
}
void copy_volume_out(const PieceArrays& src, const PieceArrays& dst, uint32_t ch, uint64_t m, hipStream_t st) {
  if (ch & RPT_VOLUME_T) HIP_TRY(hipMemcpyAsync(dst.t, src.t, m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_VOLUME_OBJECT) HIP_TRY(hipMemcpyAsync(dst.object, src.object, m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (ch & RPT_VOLUME_POSITION) HIP_TRY(hipMemcpyAsync(dst.position, src.position, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_VOLUME_NORMAL) HIP_TRY(hipMemcpyAsync(dst.normal, src.normal, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_VOLUME_VALUE) HIP_TRY(hipMemcpyAsync(dst.value, src.value, 3 * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ch & RPT_VOLUME_COVERED) HIP_TRY(hipMemcpyAsync(dst.covered, src.covered, m, hipMemcpyDeviceToHost, st));
  if (ch & RPT_VOLUME_INSIDE) HIP_TRY(hipMemcpyAsync(dst.inside, src.inside, m, hipMemcpyDeviceToHost, st));
}

// a piece of a host caller's points or rays into the handle's pair -> where the piece lies on the device
void stage_inputs(rptgpu_scene* h, const double*& a, const double*& b, uint32_t m) {
  HIP_TRY(hipMemcpyAsync(h->rays_o.p, a, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->rays_d.p, b, 3 * (uint64_t)m * sizeof(double), hipMemcpyHostToDevice, h->stream));
  a = h->rays_o.p; b = h->rays_d.p;
}

// rays == false: a, b are the points and their directions; true: the rays' origins and directions.
// on_device: a, b, out's arrays and the volume's coeffs / valid are device pointers
int read_probe_volume(rptgpu_scene* h, bool rays, uint64_t n, const double* a, const double* b, const RptProbeVolume* volume,
                      const RptVolumeQuery* q, const RptVolumeArrays* out, bool on_device, hipStream_t user_stream) {
  // (the query, the volume, the arrays: refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_volume_query(q, rays ? VOLUME_ALL : rptvolume::CH_POINT)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_volume(volume)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_volume_arrays(out, q->channels)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
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
    const PieceArrays mine = volume_arrays_in(h->pv_piece.p, lay);
    if (!on_device) { h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); }
    const rptvolume::Volume dv = upload_volume(h, *volume, q->normal_bias, on_device);
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const double *d_a = a + 3 * base, *d_b = b + 3 * base;
      const PieceArrays theirs = volume_arrays_at(*out, ch, base);
      if (!on_device) stage_inputs(h, d_a, d_b, m);
      // where this piece's results go on the device: the caller's arrays (device callers), else the handle's
      const PieceArrays dev = on_device ? theirs : mine;
      if (rays) {
        // 1. rptgpu_first_hits' query for T | OBJECT | NORMAL | POSITION, into the handle's arrays
        rptdev::HitOut ho{};
        ho.channels = RPT_HIT_T | RPT_HIT_OBJECT | RPT_HIT_NORMAL | RPT_HIT_POSITION;
        ho.t = mine.t; ho.object = mine.object; ho.normal = mine.normal; ho.position = mine.position;
        hit_piece(h, kt, hp, d_a, d_b, m, ho, prof);
        // 2. the facing, the rule, the named channels (a host caller's four hit channels: in place)
        rptvolume::Hits r{};
        r.dirs = d_b; r.t = mine.t; r.object = mine.object; r.normal = mine.normal; r.position = mine.position;
        r.fallback[0] = q->fallback[0]; r.fallback[1] = q->fallback[1]; r.fallback[2] = q->fallback[2];
        r.channels = ch;
        r.o_t = dev.t; r.o_object = dev.object; r.o_position = dev.position; r.o_normal = dev.normal;
        r.o_value = dev.value; r.o_covered = dev.covered; r.o_inside = dev.inside;
        HIP_TRY(rptvolume::lookup(st, m, dv, r));
      } else {
        rptvolume::Points p{};
        p.positions = d_a; p.normals = d_b;
        p.fallback[0] = q->fallback[0]; p.fallback[1] = q->fallback[1]; p.fallback[2] = q->fallback[2];
        p.channels = ch;
        p.value = dev.value; p.covered = dev.covered; p.inside = dev.inside;
        HIP_TRY(rptvolume::sample(st, m, dv, p));
      }
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_volume_out(mine, theirs, ch, m, st);
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
