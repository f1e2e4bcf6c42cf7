// api_aov.cpp — rptgpu_render_aov: first-hit feature buffers (include/rpt_gpu.h; see api_internal.h).
// Argument checks, the route (one fused kernel, or raygen + closest-hit query + fold in passes), the device arrays of the
// requested channels (RptAovBuffers' table: render_plan.h AOV_ROWS, channel_plan.h), one copy per channel and one
// synchronisation.  The kernels: kernels/aov.inc.
// The device half (aov_arrays, aov_enqueue, then drain_call) writes into arrays it is handed: rptgpu_render_aov hands it
// the handle's own and copies them out (copy_aov_out), rptgpu_buffer_features (api_buffer.cpp) hands it arrays the buffer
// keeps.
#include "api_internal.h"

namespace rptapi {

constexpr uint32_t AOV_ALL = RPT_AOV_DEPTH | RPT_AOV_NORMAL | RPT_AOV_ALBEDO | RPT_AOV_POSITION | RPT_AOV_OBJECT;

// what is wrong with an RptAovBuffers (nullptr: nothing)
const char* bad_aov(const RptAovBuffers* o) {
  if (!o) return "null RptAovBuffers";
  if (o->struct_size != sizeof(RptAovBuffers)) return "RptAovBuffers: struct_size is not sizeof(RptAovBuffers)";
  if (o->channels & ~AOV_ALL) return "RptAovBuffers: channels names an unknown RPT_AOV_* bit";
  if (!o->hits) return rptplan::AOV_ROWS[rptplan::AOV_R_HITS].null_text; // (in front of the channels, whatever its row's bit)
  const rptchan::Row* r = rptchan::first_null(rptplan::AOV_ROWS, o->channels, o);
  return r ? r->null_text : nullptr;
}
// ... and with the fields of RptRenderParams this call reads (max_bounces, exposure_value and collective are ignored)
const char* bad_aov_params(const RptRenderParams* p) {
  if (!p) return "null params";
  if (!p->iterations) return "iterations == 0";
  if (!p->width || !p->height) return "width * height == 0";
  if ((uint64_t)p->width * p->height >= (1ull << 31)) return "frame too large";
  if (p->part_count && p->part_index >= p->part_count) return "part_index >= part_count";
  if (p->precision_mode != RPT_PRECISION_F64_STRICT) return BAD_MODE;
  return nullptr;
}

// the kernels' struct from the arrays of rptplan::AOV_ROWS (a channel that is not named: nullptr), and back
rptdev::AovOut aov_out(const ChannelPtrs& p, uint32_t channels) {
  rptdev::AovOut ao{};
  ao.channels = channels;
  ao.depth = p.at<double>(rptplan::AOV_R_DEPTH); ao.normal = p.at<double>(rptplan::AOV_R_NORMAL);
  ao.albedo = p.at<double>(rptplan::AOV_R_ALBEDO); ao.position = p.at<double>(rptplan::AOV_R_POSITION);
  ao.hits = p.at<uint32_t>(rptplan::AOV_R_HITS); ao.object = p.at<int32_t>(rptplan::AOV_R_OBJECT);
  return ao;
}
static ChannelPtrs aov_rows(const rptdev::AovOut& ao) {
  ChannelPtrs p{};
  p.p[rptplan::AOV_R_DEPTH] = (char*)ao.depth; p.p[rptplan::AOV_R_NORMAL] = (char*)ao.normal;
  p.p[rptplan::AOV_R_ALBEDO] = (char*)ao.albedo; p.p[rptplan::AOV_R_POSITION] = (char*)ao.position;
  p.p[rptplan::AOV_R_HITS] = (char*)ao.hits; p.p[rptplan::AOV_R_OBJECT] = (char*)ao.object;
  return p;
}

// the device arrays of `channels` and hits for n pixels inside `arrays` (rptplan::AOV_ROWS' layout)
rptdev::AovOut aov_arrays(DevBuf<double>& arrays, hipStream_t st, uint64_t n, uint32_t channels) {
  const rptchan::Layout lay = rptchan::layout(rptplan::AOV_ROWS, channels | rptplan::AOV_HITS, n);
  arrays.alloc(lay.words);
  const rptdev::AovOut ao = aov_out(ptrs_in(arrays.p, lay), channels);
  // every sum starts at +0.0 and every count at 0 (also where the part has no pixel); object = -1
  const uint64_t sums_and_hits = lay.off[rptplan::AOV_R_HITS] + rptchan::row_words(rptplan::AOV_ROWS[rptplan::AOV_R_HITS], n);
  HIP_TRY(hipMemsetAsync(arrays.p, 0, sums_and_hits * sizeof(double), st));
  if (ao.object) HIP_TRY(hipMemsetAsync(ao.object, 0xff, n * sizeof(int32_t), st));
  return ao;
}

namespace {

// Scenes with deep trees (and RPT_FLAG_WAVEFRONT): per pass rpt_raygen into the workspace's ray columns, the depth-0
// closest-hit query of a render (run_pass, api_render.cpp), rpt_aov_fold.  Passes are sample-major and run in ascending
// sample order, so a pixel's additions happen in sample order whatever the pass size; a camera ray reaches depth 0
// only, hence one record column per path for the planner.
void aov_wavefront(rptgpu_scene* h, const KernelTable* kt, const RptRenderParams& p, rptdev::Frame fr, const rptdev::Camera& cam,
                   const rptdev::AovOut& ao) {
  hipStream_t st = h->stream;
  const uint32_t npix = fr.npix;
  rptplan::PassInput in{};
  in.npix = npix; in.iterations = p.iterations;
  in.per_slot = rptplan::wavefront_slot_bytes(h->dscene.num_lights, h->has_deep, h->sort_rays, h->path_reorder);
  in.target_paths = h->opt.target_paths; in.budget_bytes = h->opt.workspace_bytes;
  in.free_percent = RPT_WS_FREE_PERCENT;
  in.rec_ratio = 1.0; in.ratio = 1.0;
  const bool by_object = h->has_deep && (!(p.flags & RPT_FLAG_GENERAL_TRAVERSAL) || h->tree_kids);
  const bool generic_all = h->has_deep && (h->gen_all || h->dscene.force_general);
  for (uint32_t s0 = 0; s0 < p.iterations;) {
    in.remaining = p.iterations - s0;
    in.free_bytes = in.target_paths ? -1 : free_memory();
    in.held_slots = h->ws_cap; in.held_cols = h->ws_rec_cols;
    in.fail_paths = h->ws_fail_paths;
    const rptplan::PassPlan pp = size_pass(h, in, npix, generic_all);
    const uint32_t n_paths = npix * pp.s_chunk;
    fr.sample_base = p.sample_index_base + s0;
    const rptdev::PathState ps = path_state(h);
    if (h->has_deep) reset_tree_counters(h);
    kt->raygen(st, fr, cam, ps, n_paths);
    if (by_object)
      query_closest(h, kt, ps, n_paths, nullptr);
    else
      kt->extend(st, h->dscene, ps, nullptr, n_paths);
    kt->aov_fold(st, h->dscene, fr, ps, ao, pp.s_chunk, s0 == 0);
    HIP_TRY(hipGetLastError());
    s0 += pp.s_chunk;
  }
}

} // namespace

// The route and the kernels of one call into the zeroed arrays `ao`, enqueued on the handle's stream; -> whether
// rpt_tree_generic's overflow flag has to be read with the call's synchronisation (drain_call)
bool aov_enqueue(rptgpu_scene* h, const RptCamera& camera, const RptRenderParams& p, const rptdev::AovOut& ao) {
  hipStream_t st = h->stream;
  const KernelTable* kt = table_for(p.precision_mode, h->ext_shapes);
  const bool wavefront = use_wavefront(h, p.flags, h->has_deep);
  h->dscene.force_general = (p.flags & RPT_FLAG_GENERAL_TRAVERSAL) ? 1 : 0;
  if (h->npix) {
    rptdev::Frame fr{};
    fr.width = p.width; fr.height = p.height; fr.npix = h->npix; fr.pixels = h->pixels.p;
    fr.seed = p.seed; fr.sample_base = p.sample_index_base;
    const rptdev::Camera cam = make_camera(camera);
    if (wavefront) aov_wavefront(h, kt, p, fr, cam, ao);
    else kt->aov(st, h->dscene, fr, cam, ao, p.iterations);
  }
  HIP_TRY(hipGetLastError());
  return wavefront && h->has_deep && h->gen_overflow.p;
}

void copy_aov_out(const rptdev::AovOut& src, uint32_t channels, const ChannelPtrs& dst, uint64_t n, hipStream_t st) {
  copy_out(rptplan::AOV_ROWS, aov_rows(src), dst, rptplan::AOV_HITS, n, st); // hits first
  copy_out(rptplan::AOV_ROWS, aov_rows(src), dst, channels, n, st);
}

} // namespace rptapi

extern "C" int rptgpu_render_aov(rptgpu_scene* h, const RptCamera* camera, const RptRenderParams* p, const RptAovBuffers* out) {
  // (the buffers first: a bad RptAovBuffers is refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_aov(out)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_aov_params(p)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!camera) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null camera");
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  if (h->abandoned)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, "an aborted batch's device work never drained on this handle: destroy it");
  return guarded(h, h->device, [&]() -> int {
    hipStream_t st = h->stream;
    ensure_partition(h, *p);
    const uint64_t n = (uint64_t)p->width * p->height;
    const rptdev::AovOut ao = aov_arrays(h->aov_out, st, n, out->channels);
    const bool read_overflow = aov_enqueue(h, *camera, *p, ao);
    copy_aov_out(ao, out->channels, ptrs_at(rptplan::AOV_ROWS, out, out->channels | rptplan::AOV_HITS, 0), n, st);
    return drain_call(h, read_overflow);
  });
}
