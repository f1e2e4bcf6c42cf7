// api_aov.cpp — rptgpu_render_aov: first-hit feature buffers (include/rpt_gpu.h; see api_internal.h).
// Argument checks, the route (one fused kernel, or raygen + closest-hit query + fold in passes), the device arrays of the
// requested channels, one copy per channel and one synchronisation.  The kernels: kernels/aov.inc.
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
  if (!o->hits) return "RptAovBuffers: hits is NULL (it is always written)";
  if ((o->channels & RPT_AOV_DEPTH) && !o->depth) return "RptAovBuffers: RPT_AOV_DEPTH is named but depth is NULL";
  if ((o->channels & RPT_AOV_NORMAL) && !o->normal) return "RptAovBuffers: RPT_AOV_NORMAL is named but normal is NULL";
  if ((o->channels & RPT_AOV_ALBEDO) && !o->albedo) return "RptAovBuffers: RPT_AOV_ALBEDO is named but albedo is NULL";
  if ((o->channels & RPT_AOV_POSITION) && !o->position) return "RptAovBuffers: RPT_AOV_POSITION is named but position is NULL";
  if ((o->channels & RPT_AOV_OBJECT) && !o->object) return "RptAovBuffers: RPT_AOV_OBJECT is named but object is NULL";
  return nullptr;
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

// the device arrays: the f64 channels first, then hits and object, each 16-byte aligned inside `arrays`
rptdev::AovOut aov_arrays(DevBuf<double>& arrays, hipStream_t st, uint64_t n, uint32_t channels) {
  const uint64_t words = (n + 3) / 4 * 2; // doubles that hold n 32-bit values, rounded up to 16 bytes
  uint64_t off = 0, off_depth = 0, off_normal = 0, off_albedo = 0, off_position = 0, off_object = 0;
  if (channels & RPT_AOV_DEPTH) { off_depth = off; off += (n + 1) / 2 * 2; }
  if (channels & RPT_AOV_NORMAL) { off_normal = off; off += (3 * n + 1) / 2 * 2; }
  if (channels & RPT_AOV_ALBEDO) { off_albedo = off; off += (3 * n + 1) / 2 * 2; }
  if (channels & RPT_AOV_POSITION) { off_position = off; off += (3 * n + 1) / 2 * 2; }
  const uint64_t off_hits = off;
  off += words;
  if (channels & RPT_AOV_OBJECT) { off_object = off; off += words; }
  arrays.alloc(off);
  double* base = arrays.p;
  rptdev::AovOut ao{};
  ao.channels = channels;
  ao.hits = (uint32_t*)(base + off_hits);
  if (channels & RPT_AOV_DEPTH) ao.depth = base + off_depth;
  if (channels & RPT_AOV_NORMAL) ao.normal = base + off_normal;
  if (channels & RPT_AOV_ALBEDO) ao.albedo = base + off_albedo;
  if (channels & RPT_AOV_POSITION) ao.position = base + off_position;
  if (channels & RPT_AOV_OBJECT) ao.object = (int32_t*)(base + off_object);
  // every sum starts at +0.0 and every count at 0 (also where the part has no pixel); object = -1
  HIP_TRY(hipMemsetAsync(base, 0, (off_hits + words) * sizeof(double), st));
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

void copy_aov_out(const rptdev::AovOut& src, uint32_t channels, const RptAovBuffers& dst, uint64_t n, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(dst.hits, src.hits, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (channels & RPT_AOV_DEPTH) HIP_TRY(hipMemcpyAsync(dst.depth, src.depth, n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (channels & RPT_AOV_NORMAL) HIP_TRY(hipMemcpyAsync(dst.normal, src.normal, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (channels & RPT_AOV_ALBEDO) HIP_TRY(hipMemcpyAsync(dst.albedo, src.albedo, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (channels & RPT_AOV_POSITION) HIP_TRY(hipMemcpyAsync(dst.position, src.position, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (channels & RPT_AOV_OBJECT) HIP_TRY(hipMemcpyAsync(dst.object, src.object, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
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
    copy_aov_out(ao, out->channels, *out, n, st);
    return drain_call(h, read_overflow);
  });
}
