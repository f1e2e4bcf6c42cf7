// api_lightmap_filter.cpp — rptgpu_filter_lightmap[_device]: a baked lightmap through the geometry-guided a-trous filter
// (include/rpt_gpu_lightmap_filter.h; see api_internal.h).  The call: rpt_lightmap_filter_prepare lays the
// caller's guides down as columns with the validity bytes, the prefiltered variance and the values in the first of two
// column sets; rpt_lightmap_filter_level once per level from one set into the other; rpt_lightmap_filter_finish into the
// caller's layout; then the gutters, rptgpu_bake_lightmap's own rounds (rptlightmap::dilate) between `out` and a second copy
// that lies in the columns the filter is done with.  The sizes and the launch geometry: lightmap_filter_plan.h.  A device
// caller's arrays are read and written where they lie; a host caller's are staged whole in an array the handle keeps.
// Nothing of the handle's scene is read.
#include "api_internal.h"

namespace rptapi {

static bool good_sigma(double s) { return std::isfinite(s) && s > 0.0; }

// what is wrong with an RptLightmapFilter (sigma_color apart: bad_filter_color) / with its arrays (nullptr: nothing)
static const char* bad_filter(const RptLightmapFilter* f) {
  if (!f) return "null RptLightmapFilter";
  if (f->struct_size != sizeof(RptLightmapFilter)) return "RptLightmapFilter: struct_size is not sizeof(RptLightmapFilter)";
  if (!f->width || !f->height) return "RptLightmapFilter: width == 0 or height == 0";
  if (!rptlightmapfilter::map_fits(f->width, f->height)) return "RptLightmapFilter: width * height > 2^32";
  if (!rptlightmapfilter::words_ok(f->words)) return "RptLightmapFilter: words is neither 1 nor 3";
  if (f->levels > rptlightmapfilter::LEVELS_MAX) return "RptLightmapFilter: levels > 8";
  if (!good_sigma(f->sigma_normal)) return "RptLightmapFilter: sigma_normal is not finite and > 0";
  if (!good_sigma(f->sigma_plane)) return "RptLightmapFilter: sigma_plane is not finite and > 0";
  if (!good_sigma(f->sigma_distance)) return "RptLightmapFilter: sigma_distance is not finite and > 0";
  return nullptr;
}
static const char* bad_filter_arrays(const RptLightmapFilterArrays* a) {
  if (!a) return "null RptLightmapFilterArrays";
  if (a->struct_size != sizeof(RptLightmapFilterArrays))
    return "RptLightmapFilterArrays: struct_size is not sizeof(RptLightmapFilterArrays)";
  if (a->reserved) return "RptLightmapFilterArrays: reserved != 0";
  if (!a->owner) return "RptLightmapFilterArrays: owner is NULL";
  if (!a->position) return "RptLightmapFilterArrays: position is NULL";
  if (!a->normal) return "RptLightmapFilterArrays: normal is NULL";
  if (!a->values) return "RptLightmapFilterArrays: values is NULL";
  if (!a->out) return "RptLightmapFilterArrays: out is NULL";
  if (a->out_variance && !a->variance) return "RptLightmapFilterArrays: out_variance without variance";
  return nullptr;
}
// (sigma_color is read only with a variance: it is checked behind the arrays)
static const char* bad_filter_color(const RptLightmapFilter* f, const RptLightmapFilterArrays* a) {
  if (a->variance && !good_sigma(f->sigma_color)) return "RptLightmapFilter: sigma_color is not finite and > 0 (variance is given)";
  return nullptr;
}

namespace {

// on_device: a's arrays are device pointers (user_stream: the stream their producer ran on)
int filter_lightmap(rptgpu_scene* h, const RptLightmapFilter* f, const RptLightmapFilterArrays* a, bool on_device,
                    hipStream_t user_stream) {
  // (the filter first, then the arrays: both are refused whatever else is wrong, also without a handle or a device)
  if (const char* why = bad_filter(f)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_filter_arrays(a)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (const char* why = bad_filter_color(f, a)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, why);
  if (!h) return fail(h, RPTGPU_E_INVALID_ARGUMENT, "null handle");
  REFUSE_IF_ABANDONED(h);
  return device_call(h, user_stream, [&]() {
    namespace lf = rptlightmapfilter;
    hipStream_t st = h->stream;
    const uint32_t W = f->width, H = f->height, words = f->words;
    const uint64_t n = lf::texels(W, H);
    const bool variance = a->variance != nullptr;

    // where the caller's arrays lie on the device: where they are, or the handle's staging
    lf::Inputs in{a->owner, a->position, a->normal, a->values, a->variance};
    double *out = a->out, *out_variance = a->out_variance;
    if (!on_device) {
      const lf::Stage s = lf::stage(n, words, variance, out_variance != nullptr);
      h->lf_stage.alloc(s.words);
      double* d = h->lf_stage.p;
      HIP_TRY(hipMemcpyAsync(d + s.owner, a->owner, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d + s.position, a->position, 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d + s.normal, a->normal, 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d + s.values, a->values, words * n * sizeof(double), hipMemcpyHostToDevice, st));
      if (variance) HIP_TRY(hipMemcpyAsync(d + s.variance, a->variance, n * sizeof(double), hipMemcpyHostToDevice, st));
      in = lf::Inputs{(const int32_t*)(d + s.owner), d + s.position, d + s.normal, d + s.values, variance ? d + s.variance : nullptr};
      out = d + s.out;
      out_variance = out_variance ? d + s.out_variance : nullptr;
    }

    // the columns
    const lf::Workspace ws = lf::workspace(n, words, variance);
    h->lf_ws.alloc(ws.words);
    double* base = h->lf_ws.p;
    uint8_t* valid = (uint8_t*)(base + ws.valid);
    const lf::Guides g{base + ws.position, base + ws.normal, valid, n, W, H};
    double* c[2] = {base + ws.c[0], base + ws.c[1]};
    double* v[2] = {variance ? base + ws.v[0] : nullptr, variance ? base + ws.v[1] : nullptr};
    const lf::Sigmas sg{f->sigma_normal, f->sigma_plane, f->sigma_distance, variance ? f->sigma_color : 0.0};

    HIP_TRY(lf::prepare(st, in, words, g, c[0], v[0]));
    for (uint32_t l = 0; l < f->levels; l++) {
      const uint32_t s = lf::source_set(l);
      HIP_TRY(lf::level(st, g, words, c[s], v[s], c[1 - s], v[1 - s], lf::step(l), sg));
    }
    const uint32_t r = lf::result_set(f->levels);
    HIP_TRY(lf::finish(st, n, words, c[r], v[r], out, out_variance));

    // the gutters: rptgpu_bake_lightmap's rounds with FILLED = valid, between `out` and a second copy over the columns,
    // which nobody reads any more; the second set of flags over the position columns
    const uint32_t rounds = lf::rounds(f->dilate, W, H);
    double *src = out, *dst = base + ws.pong;
    uint8_t* flags[2] = {valid, (uint8_t*)(base + ws.flags2)};
    for (uint32_t k = 0; k < rounds; k++) {
      HIP_TRY(rptlightmap::dilate(st, W, H, words, src, flags[k % 2], dst, flags[(k + 1) % 2]));
      std::swap(src, dst);
    }
    if (src != out) HIP_TRY(hipMemcpyAsync(out, src, words * n * sizeof(double), hipMemcpyDeviceToDevice, st));

    if (!on_device) {
      HIP_TRY(hipMemcpyAsync(a->out, out, words * n * sizeof(double), hipMemcpyDeviceToHost, st));
      if (out_variance) HIP_TRY(hipMemcpyAsync(a->out_variance, out_variance, n * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    return false; // (no tree walk: nothing to read behind the call)
  });
}

} // namespace

} // namespace rptapi

extern "C" {

int rptgpu_filter_lightmap(rptgpu_scene* h, const RptLightmapFilter* f, const RptLightmapFilterArrays* a) {
  return rptapi::filter_lightmap(h, f, a, false, nullptr);
}

int rptgpu_filter_lightmap_device(rptgpu_scene* h, const RptLightmapFilter* f, const RptLightmapFilterArrays* d_a, void* stream) {
  return rptapi::filter_lightmap(h, f, d_a, true, (hipStream_t)stream);
}

} // extern "C"
