// api_lightmap_lookup.cpp — rptgpu_lookup_lightmap[_device]: a baked lightmap read back at the first hits of the caller's rays
// (include/rpt_gpu_lightmap_lookup.h; see api_internal.h).  Per piece: rptgpu_first_hits' own query for T and
// OBJECT (api_hits.cpp plan_hit_pieces / hit_piece) and rptgpu_hit_surface's resolve walk for PRIMITIVE and BARYCENTRIC
// (api_surface.cpp surface_walk_piece), both unchanged, into arrays the handle keeps; then rpt_lightmap_lookup
// (kernels/lightmap_lookup.inc), one lane per ray.  The binding records and the object-to-binding table are made here per
// call; the sizes — a piece's arrays, a host caller's staging — and RptLookupArrays' channel table are lightmap_lookup_plan.h's.
// rptgpu_render_views_lightmapped[_device]: the same three steps per sample over rptgpu_render_views' own rays
// (rpt_raygen_views[_seeded], unchanged, then rpt_views_rays_gather), and rpt_views_lightmapped_fold into the frame
// (kernels/lightmap_views.inc).
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t LOOKUP_ALL = RPT_LOOKUP_T | RPT_LOOKUP_OBJECT | RPT_LOOKUP_BINDING | RPT_LOOKUP_COVERED | RPT_LOOKUP_UV | RPT_LOOKUP_VALUE;
static_assert(rptlookup::CH_T == RPT_LOOKUP_T && rptlookup::CH_OBJECT == RPT_LOOKUP_OBJECT && rptlookup::CH_BINDING == RPT_LOOKUP_BINDING &&
              rptlookup::CH_COVERED == RPT_LOOKUP_COVERED && rptlookup::CH_UV == RPT_LOOKUP_UV && rptlookup::CH_VALUE == RPT_LOOKUP_VALUE &&
              rptlookup::CH_ALL == LOOKUP_ALL && rptlookup::FILTER_NEAREST == RPT_LOOKUP_NEAREST &&
              rptlookup::FILTER_BILINEAR == RPT_LOOKUP_BILINEAR && !(LOOKUP_ALL & (rptlookup::IN_PRIMITIVE | rptlookup::IN_BARYCENTRIC)),
              "lightmap_lookup_plan.h restates the header's channel bits and filters");

namespace {

// what is wrong with an RptLookupQuery (nullptr: nothing)
const char* bad_lookup_query(const RptLookupQuery* q) {
  if (const char* why = bad_channel_query(q, RPT_QUERY_TEXTS(RptLookupQuery, RPT_LOOKUP), LOOKUP_ALL)) return why;
  if (q->filter != RPT_LOOKUP_NEAREST && q->filter != RPT_LOOKUP_BILINEAR)
    return "RptLookupQuery: filter is neither RPT_LOOKUP_NEAREST nor RPT_LOOKUP_BILINEAR";
  if (q->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  if (q->flags & RPT_FLAG_PERSISTENT)
    return "RPT_FLAG_PERSISTENT — the persistent kernel makes its rays from a camera; a lightmap lookup runs the closest-hit "
           "query, a resolve walk and a fetch only";
  return nullptr;
}
} // namespace

// (the bindings' checks and uploads are rptgpu_render_views_probe_lit's too: api_internal.h, api_probe_volume.cpp)
// what is wrong with the bindings by themselves (empty: nothing)
std::string bad_bindings(uint32_t n_bindings, const RptLightmapBinding* b) {
  if (n_bindings && !b) return "null bindings with n_bindings > 0";
  std::vector<uint32_t> objects;
  for (uint32_t k = 0; k < n_bindings; k++) {
    const std::string who = "binding " + std::to_string(k) + ": ";
    if (b[k].struct_size != sizeof(RptLightmapBinding)) return who + "struct_size is not sizeof(RptLightmapBinding)";
    if (b[k].reserved) return who + "reserved != 0";
    if (!b[k].width || !b[k].height) return who + "width or height is 0";
    if (b[k].components != 1 && b[k].components != 3) return who + "components is neither 1 nor 3";
    if (!b[k].uvs) return who + "uvs is NULL";
    if (!b[k].map) return who + "map is NULL";
    objects.push_back(b[k].object);
  }
  std::sort(objects.begin(), objects.end());
  const auto twice = std::adjacent_find(objects.begin(), objects.end());
  if (twice != objects.end()) return "two bindings name object " + std::to_string(*twice);
  return "";
}
// ... and against the handle's scene
std::string bad_bindings_for(const rptgpu_scene* h, uint32_t n_bindings, const RptLightmapBinding* b) {
  const size_t count = h->obj_geom.size();
  for (uint32_t k = 0; k < n_bindings; k++) {
    const std::string who = "binding " + std::to_string(k) + ": object " + std::to_string(b[k].object);
    if (b[k].object >= count) return who + " is out of range (the scene has " + std::to_string(count) + ")";
    const rptdev::Inst& in = h->top_insts[b[k].object];
    if (in.kind != RPT_SHAPE_MESH) return who + " is not a top-level mesh (shape kind " + std::to_string(in.kind) + ")";
    const uint64_t tris = h->host_trees[(size_t)in.tree].num_prims;
    if (b[k].n_tris != tris)
      return who + ": n_tris = " + std::to_string(b[k].n_tris) + " differs from the mesh's triangle count (" + std::to_string(tris) + ")";
  }
  return "";
}

// the call's binding records and object-to-binding table on the device (a host caller's arrays staged whole), into `rays`.
// table and recs are the caller's: the uploads read them until the call's last synchronisation
void upload_bindings(rptgpu_scene* h, uint32_t n_bindings, const RptLightmapBinding* bindings, bool on_device,
                     const std::vector<rptlookup::Staged>& staged, uint64_t stage_words, std::vector<int32_t>& table,
                     std::vector<rptlookup::Binding>& recs, rptlookup::Rays& rays) {
  hipStream_t st = h->stream;
  if (!on_device) h->lk_stage.alloc(stage_words);
  for (uint32_t k = 0; k < n_bindings; k++) {
    const RptLightmapBinding& b = bindings[k];
    rptlookup::Binding& r = recs[k];
    r.n_tris = b.n_tris; r.width = b.width; r.height = b.height; r.components = b.components;
    if (on_device) {
      r.uvs = b.uvs; r.map = b.map; r.valid = b.valid;
    } else {
      const rptlookup::Staged& s = staged[k];
      double* base = h->lk_stage.p;
      if (s.uv_words) HIP_TRY(hipMemcpyAsync(base + s.uvs, b.uvs, s.uv_words * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(base + s.map, b.map, s.map_words * sizeof(double), hipMemcpyHostToDevice, st));
      if (b.valid) HIP_TRY(hipMemcpyAsync(base + s.valid, b.valid, s.valid_bytes, hipMemcpyHostToDevice, st));
      r.uvs = base + s.uvs; r.map = base + s.map;
      r.valid = b.valid ? (const uint8_t*)(base + s.valid) : nullptr;
    }
    table[b.object] = (int32_t)k;
  }
  h->lk_table.upload(table, st);
  h->lk_bindings.upload(recs, st);
  rays.binding_of = h->lk_table.p;
  rays.bindings = h->lk_bindings.p;
  rays.num_objects = (uint32_t)table.size();
}
// a host caller's bindings' arrays inside one allocation -> the words, or ~0 when no allocation holds them
uint64_t stage_bindings(uint32_t n_bindings, const RptLightmapBinding* bindings, bool on_device, std::vector<rptlookup::Staged>& staged) {
  uint64_t words = 0;
  staged.assign(n_bindings, rptlookup::Staged{});
  if (!on_device)
    for (uint32_t k = 0; k < n_bindings; k++) {
      const RptLightmapBinding& b = bindings[k];
      staged[k] = rptlookup::stage_binding(words, b.n_tris, b.width, b.height, b.components, b.valid != nullptr);
      if (!staged[k].ok) return ~0ull;
      words = staged[k].end;
    }
  return words;
}

namespace {
constexpr const char* TOO_LARGE = BINDINGS_TOO_LARGE;

// on_device: origins, dirs, out's arrays and every binding's uvs / map / valid are device pointers
int lookup_lightmap(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, uint32_t n_bindings,
                    const RptLightmapBinding* bindings, const RptLookupQuery* q, const RptLookupArrays* out, bool on_device,
                    hipStream_t user_stream) {
  // (the query, the arrays, the bindings by themselves: refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_lookup_query(q)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_channel_arrays(out, RPT_ARRAYS_TEXTS(RptLookupArrays), rptlookup::ROWS, q->channels))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (n && (!origins || !dirs)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  {
    const std::string why = bad_bindings(n_bindings, bindings);
    if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  }
  std::vector<rptlookup::Staged> staged;
  const uint64_t stage_words = stage_bindings(n_bindings, bindings, on_device, staged);
  if (stage_words == ~0ull) return fail(h, RPTGPU_E_INVALID_ARGUMENT, TOO_LARGE);
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  {
    const std::string why = bad_bindings_for(h, n_bindings, bindings);
    if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  }
  REFUSE_IF_ABANDONED(h);
  if (!n) return RPTGPU_OK;
  // (these outlive the call's last synchronisation: the uploads read them)
  std::vector<int32_t> table(h->obj_geom.size(), -1);
  std::vector<rptlookup::Binding> recs(n_bindings);
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(q->precision_mode, h->ext_shapes);
    const bool prof = (q->flags & RPT_FLAG_PROFILE_KERNELS) != 0;
    const uint32_t ch = q->channels;
    const bool fetch = rptlookup::needs_lookup(ch);
    const HitPieces hp = plan_hit_pieces(h, n, q->flags, "RPTGPU_LOOKUP_PIECE");
    const uint64_t piece = hp.piece;
    const rptlookup::Layout lay = rptlookup::layout(piece, ch, on_device);
    h->lk_piece.alloc(lay.words);
    const ChannelPtrs mine = ptrs_in(h->lk_piece.p, lay);
    if (!on_device) { h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece); }
    GenericStack gs{};
    bool from_inf = false;
    rptlookup::Rays rays{};
    if (fetch) {
      gs = ensure_surface_columns(h, piece);
      from_inf = group_holds_monomial(h);
      upload_bindings(h, n_bindings, bindings, on_device, staged, stage_words, table, recs, rays);
      rays.filter = q->filter;
      rays.fallback[0] = q->fallback[0]; rays.fallback[1] = q->fallback[1]; rays.fallback[2] = q->fallback[2];
      rays.channels = ch & rptlookup::CH_KERNEL;
    }
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const double *d_o = origins + 3 * base, *d_d = dirs + 3 * base;
      const ChannelPtrs theirs = ptrs_at(rptlookup::ROWS, out, ch, base);
      if (!on_device) stage_rays(h, d_o, d_d, m);
      // where this piece's results lie on the device: the caller's arrays (device callers), else the handle's — the
      // kernels' structs from the arrays of rptlookup::ROWS
      const ChannelPtrs& dev = on_device ? theirs : mine;
      double* const t = (lay.has & RPT_LOOKUP_T ? mine : dev).at<double>(rptlookup::R_T);
      int32_t* const object = (lay.has & RPT_LOOKUP_OBJECT ? mine : dev).at<int32_t>(rptlookup::R_OBJECT);
      rptdev::SurfaceOut so{};
      so.t = t; so.object = object;
      so.primitive = mine.at<int32_t>(rptlookup::R_PRIMITIVE); so.barycentric = mine.at<double>(rptlookup::R_BARYCENTRIC);
      so.channels = RPT_SURFACE_PRIMITIVE | RPT_SURFACE_BARYCENTRIC;
      // 1. rptgpu_first_hits' query for T | OBJECT — what the caller named of the two, and both where the fetch follows
      rptdev::HitOut ho{};
      if (t) { ho.channels |= RPT_HIT_T; ho.t = t; }
      if (object) { ho.channels |= RPT_HIT_OBJECT; ho.object = object; }
      hit_piece(h, kt, hp, d_o, d_d, m, ho, prof);
      if (fetch) {
        // 2. rptgpu_hit_surface's resolve walk for PRIMITIVE | BARYCENTRIC
        surface_walk_piece(h, d_o, d_d, m, so, gs, from_inf);
        // 3. the fetch
        rays.object = object; rays.primitive = so.primitive; rays.barycentric = so.barycentric;
        rays.binding = dev.at<int32_t>(rptlookup::R_BINDING); rays.covered = dev.at<uint8_t>(rptlookup::R_COVERED);
        rays.uv = dev.at<double>(rptlookup::R_UV); rays.value = dev.at<double>(rptlookup::R_VALUE);
        HIP_TRY(rptlookup::lookup(st, m, rays));
      }
      if (!on_device) { // the staging arrays are the next piece's, too
        copy_out(rptlookup::ROWS, mine, theirs, ch, m, st);
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return (fetch || h->has_deep) && h->gen_overflow.p;
  });
}

// what is wrong with an RptViewsLightmapQuery (nullptr: nothing)
const char* bad_views_lightmap_query(const RptViewsLightmapQuery* q) {
  if (!q) return "null RptViewsLightmapQuery";
  if (q->struct_size != sizeof(RptViewsLightmapQuery)) return "RptViewsLightmapQuery: struct_size is not sizeof(RptViewsLightmapQuery)";
  if (q->filter != RPT_LOOKUP_NEAREST && q->filter != RPT_LOOKUP_BILINEAR)
    return "RptViewsLightmapQuery: filter is neither RPT_LOOKUP_NEAREST nor RPT_LOOKUP_BILINEAR";
  return nullptr;
}

} // namespace

// The one driver behind rptgpu_render_views_lightmapped[_device] and rptgpu_render_views_probe_lit[_device] (api_internal.h).
// on_device: out, every binding's uvs / map / valid and the volume's coeffs / valid are device pointers; views and the structs
// are host memory either way.  lit.volume == nullptr: the lightmapped call, as it always ran.  With a volume: the first-hit
// query also writes NORMAL and POSITION (into the handle's pv_piece), rpt_views_probe_lit_merge stands in front of the fold,
// and without bindings the resolve walk and the lookup are not run
int render_views_lit(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* qv, uint32_t n_bindings,
                     const RptLightmapBinding* bindings, const char* bad_own_query, const ViewsLit& lit, double* out, bool on_device,
                     hipStream_t user_stream) {
  if (const char* why = bad_view_query(qv)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (bad_own_query) return fail(h, RPTGPU_E_INVALID_ARGUMENT, bad_own_query);
  if (!out) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null out");
  if (n_views && !views) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  const uint64_t npix = (uint64_t)qv->width * qv->height;
  if (n_views > (1ull << 58) / npix) // (3 values of 8 bytes per index: an array's size in bytes fits 64 bits)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "n_views * width * height does not fit: the frames would not fit any memory");
  for (uint64_t v = 0; v < n_views; v++)
    if (const char* why = bad_view(views[v], *qv)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  {
    const std::string why = bad_bindings(n_bindings, bindings);
    if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  }
  std::vector<rptlookup::Staged> staged;
  const uint64_t stage_words = stage_bindings(n_bindings, bindings, on_device, staged);
  if (stage_words == ~0ull) return fail(h, RPTGPU_E_INVALID_ARGUMENT, BINDINGS_TOO_LARGE);
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  {
    const std::string why = bad_bindings_for(h, n_bindings, bindings);
    if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  }
  REFUSE_IF_ABANDONED(h);
  if (!n_views) return RPTGPU_OK;
  // (these outlive the call's last synchronisation: the uploads read them)
  std::vector<int32_t> table(h->obj_geom.size(), -1);
  std::vector<rptlookup::Binding> recs(n_bindings);
  std::vector<rptdev::View> view_recs(n_views);
  const std::vector<uint64_t> seed_list = view_seed_list(n_views, *qv, nullptr);
  return device_call(h, user_stream, [&]() {
    hipStream_t st = h->stream;
    const KernelTable* kt = table_for(qv->precision_mode, h->ext_shapes);
    const bool prof = (qv->flags & RPT_FLAG_PROFILE_KERNELS) != 0;
    const bool with_volume = lit.volume != nullptr;
    const bool fetch = !with_volume || n_bindings != 0; // (a volume without bindings: no ray is covered by a lightmap)
    // the views' device records: the camera constants by the host function a render uses (as rptgpu_render_views)
    for (uint64_t v = 0; v < n_views; v++) {
      view_recs[v].cam = make_camera(views[v].camera);
      view_recs[v].projection = views[v].projection;
      view_recs[v].ortho_scale = views[v].ortho_scale;
    }
    h->view_recs.upload(view_recs, st);
    const bool per_view = !seed_list.empty();
    if (per_view) h->view_seeds.upload(seed_list, st);
    // the piece: consecutive (view, pixel) indices, at most what a pass and the first-hit query hold; one sample per pass
    const uint64_t n = n_views * npix;
    uint64_t asked = 0; // tests: pieces of a few pixels
    if (const char* e = std::getenv("RPTGPU_VIEWS_PIECE")) asked = std::strtoull(e, nullptr, 10);
    uint64_t piece = rptplan::views_piece(n, asked, piece_pass_target(h, 1, 0));
    HitPieces hp = plan_hit_pieces(h, piece, qv->flags, "RPTGPU_LOOKUP_PIECE");
    piece = std::min(piece, hp.piece);
    if (with_volume) piece = rptvolume::piece(piece, asked_volume_piece(), piece); // (RPTGPU_VOLUME_PIECE caps it too)
    ensure_workspace(h, piece, 1); // rpt_raygen_views' columns (the per-tree query's own, where that route runs)
    const rptdev::PathState ps = path_state(h);
    if (hp.by_object) hp.ps = ps;
    h->ray_ids.alloc(piece);
    if (per_view) h->ray_seeds.alloc(piece);
    h->rays_o.alloc(3 * piece); h->rays_d.alloc(3 * piece);
    if (!on_device) h->rays_out.alloc(3 * piece);
    constexpr uint32_t CH = RPT_LOOKUP_VALUE | RPT_LOOKUP_COVERED;
    const rptlookup::Layout lay = rptlookup::layout(piece, CH, false);
    h->lk_piece.alloc(lay.words);
    const ChannelPtrs mine = ptrs_in(h->lk_piece.p, lay);
    int32_t* const primitive = mine.at<int32_t>(rptlookup::R_PRIMITIVE);
    double *const barycentric = mine.at<double>(rptlookup::R_BARYCENTRIC), *const value = mine.at<double>(rptlookup::R_VALUE);
    uint8_t* const covered = mine.at<uint8_t>(rptlookup::R_COVERED);
    // the first hit's record: T and OBJECT in the lookup's arrays — with a volume all four of the query's in the volume's
    rptdev::HitOut ho{};
    ho.channels = RPT_HIT_T | RPT_HIT_OBJECT; ho.t = mine.at<double>(rptlookup::R_T); ho.object = mine.at<int32_t>(rptlookup::R_OBJECT);
    if (with_volume) {
      const rptvolume::Layout vlay = rptvolume::layout(piece, 0, true, true);
      h->pv_piece.alloc(vlay.words);
      const ChannelPtrs vol = ptrs_in(h->pv_piece.p, vlay);
      ho.channels |= RPT_HIT_NORMAL | RPT_HIT_POSITION;
      ho.t = vol.at<double>(rptvolume::R_T); ho.object = vol.at<int32_t>(rptvolume::R_OBJECT);
      ho.normal = vol.at<double>(rptvolume::R_NORMAL); ho.position = vol.at<double>(rptvolume::R_POSITION);
    }
    GenericStack gs{};
    bool from_inf = false;
    rptlookup::Rays rays{};
    if (fetch) {
      gs = ensure_surface_columns(h, piece);
      from_inf = group_holds_monomial(h);
      upload_bindings(h, n_bindings, bindings, on_device, staged, stage_words, table, recs, rays);
      rays.filter = lit.filter;
      rays.channels = CH;
      rays.object = ho.object; rays.primitive = primitive; rays.barycentric = barycentric;
      rays.covered = covered; rays.value = value;
    }
    rptvolume::Volume dv{};
    rptvolumeviews::Merge mg{};
    if (with_volume) {
      dv = upload_volume(h, *lit.volume, lit.normal_bias, on_device);
      mg.dirs = h->rays_d.p; mg.object = ho.object; mg.normal = ho.normal; mg.position = ho.position;
      mg.lightmaps = fetch ? 1u : 0u;
      mg.covered = covered; mg.value = value;
    }
    rptlookupviews::Sample smp{};
    smp.object = ho.object; smp.dirs = h->rays_d.p; smp.covered = covered; smp.value = value;
    smp.unbound[0] = lit.unbound[0]; smp.unbound[1] = lit.unbound[1]; smp.unbound[2] = lit.unbound[2];
    smp.iterations = (double)qv->iterations;
    smp.ev_scale = std::pow(2.0, qv->exposure_value);
    for (uint64_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      double* frame = on_device ? out + 3 * base : h->rays_out.p;
      rptdev::Frame fr{};
      fr.width = m; fr.height = 1; fr.npix = m; fr.pixels = h->ray_ids.p;
      fr.seed = per_view ? 0 : qv->seed;
      for (uint32_t s = 0; s < qv->iterations; s++) { // ascending: an index's additions happen in sample order
        fr.sample_base = qv->sample_index_base + s;
        // 1. rptgpu_render_views' own first step, then its rays interleaved
        if (per_view)
          kt->raygen_views_seeded(st, fr, h->view_recs.p, qv->width, qv->height, base, h->ray_ids.p, h->view_seeds.p, h->ray_seeds.p, 0, m, ps, m);
        else kt->raygen_views(st, fr, h->view_recs.p, qv->width, qv->height, base, h->ray_ids.p, ps, m);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rptlookupviews::gather_rays(st, ps.ray, ps.cap, m, h->rays_o.p, h->rays_d.p));
        // 2. the ray form's steps: the first hit, the surface element, the fetch
        hit_piece(h, kt, hp, h->rays_o.p, h->rays_d.p, m, ho, prof);
        if (fetch) {
          rptdev::SurfaceOut so{};
          so.t = ho.t; so.object = ho.object; so.primitive = primitive; so.barycentric = barycentric;
          so.channels = RPT_SURFACE_PRIMITIVE | RPT_SURFACE_BARYCENTRIC;
          surface_walk_piece(h, h->rays_o.p, h->rays_d.p, m, so, gs, from_inf);
          HIP_TRY(rptlookup::lookup(st, m, rays));
        }
        // ... and the volume where no lightmap covers the hit, into the lookup's arrays
        if (with_volume) HIP_TRY(rptvolumeviews::merge(st, m, dv, mg));
        // 3. the sample into the frame's sums
        smp.first = s == 0; smp.last = s + 1 == qv->iterations;
        HIP_TRY(rptlookupviews::fold(st, h->dscene, m, smp, frame));
      }
      if (!on_device) { // the staging array is the next piece's, too
        HIP_TRY(hipMemcpyAsync(out + 3 * base, frame, 3 * (uint64_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
    }
    return (fetch || h->has_deep) && h->gen_overflow.p;
  });
}

namespace {

int render_views_lightmapped(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* qv, uint32_t n_bindings,
                             const RptLightmapBinding* bindings, const RptViewsLightmapQuery* q, double* out, bool on_device,
                             hipStream_t user_stream) {
  const char* why = bad_views_lightmap_query(q);
  ViewsLit lit{};
  if (!why) { lit.filter = q->filter; lit.unbound = q->unbound_irradiance; }
  return render_views_lit(h, n_views, views, qv, n_bindings, bindings, why, lit, out, on_device, user_stream);
}

} // namespace
} // namespace rptapi

extern "C" {

int rptgpu_lookup_lightmap(rptgpu_scene* h, uint64_t n, const double* origins, const double* dirs, uint32_t n_bindings,
                           const RptLightmapBinding* bindings, const RptLookupQuery* q, const RptLookupArrays* out) {
  return lookup_lightmap(h, n, origins, dirs, n_bindings, bindings, q, out, false, nullptr);
}

int rptgpu_lookup_lightmap_device(rptgpu_scene* h, uint64_t n, const void* d_origins, const void* d_dirs, uint32_t n_bindings,
                                  const RptLightmapBinding* d_bindings, const RptLookupQuery* q, const RptLookupArrays* d_out,
                                  void* stream) {
  return lookup_lightmap(h, n, (const double*)d_origins, (const double*)d_dirs, n_bindings, d_bindings, q, d_out, true,
                         (hipStream_t)stream);
}

int rptgpu_render_views_lightmapped(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                    uint32_t n_bindings, const RptLightmapBinding* bindings, const RptViewsLightmapQuery* q, double* out) {
  return render_views_lightmapped(h, n_views, views, q_views, n_bindings, bindings, q, out, false, nullptr);
}

int rptgpu_render_views_lightmapped_device(rptgpu_scene* h, uint64_t n_views, const RptView* views, const RptViewQuery* q_views,
                                           uint32_t n_bindings, const RptLightmapBinding* d_bindings, const RptViewsLightmapQuery* q,
                                           void* d_out, void* stream) {
  return render_views_lightmapped(h, n_views, views, q_views, n_bindings, d_bindings, q, (double*)d_out, true, (hipStream_t)stream);
}

} // extern "C"
