// kernels/aov.inc — first-hit feature buffers (rptgpu_render_aov, DESIGN.md §11): per pixel the f64 SUMS of depth,
// shading normal, albedo and world position over the hits of the call's camera rays, the hit count, and the object of
// the call's first sample.  Part of kernels.inc (inside namespace RPT_NS).
//
// The contract fixes the order of every addition — a pixel's samples in ascending order, each sum starting at +0.0 — so
// both kernels give ONE LANE a pixel and let it walk that pixel's samples: no atomics, no tree of partial sums.  The
// sums live in the full-frame output arrays (zeroed by the host; pixels outside the caller's part are never touched):
// rpt_aov adds each hit to what the samples before it left there, rpt_aov_fold a pass's hits to what the passes before it
// left there: either way the same sequence of additions.  The channel mask is a kernel argument
// (wave-uniform): a channel that is not asked for is neither added nor stored, and its pointer is never read.

// one hit into the sums (contract step 3); o, d: the ray the hit belongs to
RPT_DEV void aov_add(const Scene& sc, uint32_t ch, D3 o, D3 d, double t, D3 nrm, int obj, uint32_t& hits, double& depth,
                     D3& normal, D3& albedo, D3& position) {
  hits += 1u;
  if (ch & RPT_AOV_DEPTH) depth += t;
  if (ch & RPT_AOV_NORMAL) normal = normal + nrm;
  if (ch & RPT_AOV_ALBEDO) {
    const Material& mat = sc.materials[sc.insts[obj].material];
    albedo = albedo + mk(mat.color[0], mat.color[1], mat.color[2]);
  }
  if (ch & RPT_AOV_POSITION) position = position + (o + t * d); // Ray::at (shape.rs:59-61): one multiply, one add
}

RPT_DEV void aov_store(const AovOut& out, uint32_t pixel, uint32_t hits, double depth, D3 normal, D3 albedo, D3 position) {
  const uint32_t ch = out.channels;
  const uint64_t p3 = 3ull * pixel;
  out.hits[pixel] = hits;
  if (ch & RPT_AOV_DEPTH) out.depth[pixel] = depth;
  if (ch & RPT_AOV_NORMAL) { out.normal[p3] = normal.x; out.normal[p3 + 1] = normal.y; out.normal[p3 + 2] = normal.z; }
  if (ch & RPT_AOV_ALBEDO) { out.albedo[p3] = albedo.x; out.albedo[p3 + 1] = albedo.y; out.albedo[p3 + 2] = albedo.z; }
  if (ch & RPT_AOV_POSITION) { out.position[p3] = position.x; out.position[p3 + 1] = position.y; out.position[p3 + 2] = position.z; }
}

// In-kernel scenes: camera ray, closest hit and the fold in one kernel; the ray never leaves registers.  One lane per
// pixel of the part, `iterations` samples each, in rpt_extend's shape (256-thread blocks, the kd stack's first levels in
// LDS).  fr.sample_base is the call's sample_index_base.  Between two samples the sums rest in the pixel's own words of
// the output arrays (L2-resident, touched by this lane alone) instead of 21 registers that would be live across the
// traversal: closest_hit<> fills rpt_extend's 168-register budget by itself, and what does not fit is spilled wherever
// the allocator likes — here the round trip stands outside the traversal loop by construction.
__global__ void __launch_bounds__(256, RPT_WF_WAVES) rpt_aov(Scene sc, Frame fr, Camera cam, AovOut out, uint32_t iterations) {
  __shared__ KdLdsW kd_lds;
  const uint32_t p_local = blockIdx.x * blockDim.x + threadIdx.x;
  if (p_local >= fr.npix) return;
  const uint32_t pixel = fr.pixels[p_local];
  const uint32_t ch = out.channels;
  const double dim = (double)max(fr.width, fr.height);
  uint32_t hits = 0u;
  for (uint32_t s = 0; s < iterations; s++) {
    D3 o, d, nrm;
    Rng rng;
    camera_ray(fr, cam, dim, pixel, s, o, d, rng);
    double t;
    const int obj = closest_hit<KdLdsW>(sc, o, d, t, nrm, &kd_lds);
    if (s == 0u && (ch & RPT_AOV_OBJECT)) out.object[pixel] = obj;
    if (obj < 0) continue;
    double depth = 0.0;
    D3 normal = mk(0, 0, 0), albedo = mk(0, 0, 0), position = mk(0, 0, 0);
    if (hits) { // (the first hit adds to +0.0: the host has zeroed the arrays, nothing to read)
      const uint64_t p3 = 3ull * pixel;
      if (ch & RPT_AOV_DEPTH) depth = out.depth[pixel];
      if (ch & RPT_AOV_NORMAL) normal = mk(out.normal[p3], out.normal[p3 + 1], out.normal[p3 + 2]);
      if (ch & RPT_AOV_ALBEDO) albedo = mk(out.albedo[p3], out.albedo[p3 + 1], out.albedo[p3 + 2]);
      if (ch & RPT_AOV_POSITION) position = mk(out.position[p3], out.position[p3 + 1], out.position[p3 + 2]);
    }
    aov_add(sc, ch, o, d, t, nrm, obj, hits, depth, normal, albedo, position);
    aov_store(out, pixel, hits, depth, normal, albedo, position);
  }
}

// Scenes with deep trees: one pass's hits (rpt_raygen's rays, the depth-0 closest-hit query's records; slot =
// s_local * npix + p_local) added to the running sums, one lane per pixel over the pass's `spp` samples in ascending
// order.  The ray is re-read from the origin / direction columns, not drawn again.  first: the pass holds the call's
// first sample (the sums start at +0.0 — the host has zeroed the arrays — and `object` is that sample's).
__global__ void __launch_bounds__(256) rpt_aov_fold(Scene sc, Frame fr, PathState ps, AovOut out, uint32_t spp, int first) {
  const uint32_t p_local = blockIdx.x * blockDim.x + threadIdx.x;
  if (p_local >= fr.npix) return;
  const uint32_t pixel = fr.pixels[p_local];
  const uint32_t ch = out.channels;
  const uint64_t p3 = 3ull * pixel;
  uint32_t hits = 0u;
  double depth = 0.0;
  D3 normal = mk(0, 0, 0), albedo = mk(0, 0, 0), position = mk(0, 0, 0);
  if (!first) {
    hits = out.hits[pixel];
    if (ch & RPT_AOV_DEPTH) depth = out.depth[pixel];
    if (ch & RPT_AOV_NORMAL) normal = mk(out.normal[p3], out.normal[p3 + 1], out.normal[p3 + 2]);
    if (ch & RPT_AOV_ALBEDO) albedo = mk(out.albedo[p3], out.albedo[p3 + 1], out.albedo[p3 + 2]);
    if (ch & RPT_AOV_POSITION) position = mk(out.position[p3], out.position[p3 + 1], out.position[p3 + 2]);
  }
  for (uint32_t s = 0; s < spp; s++) {
    const uint64_t slot = (uint64_t)s * fr.npix + p_local;
    const int obj = ps.hit_obj[slot];
    if (s == 0u && first && (ch & RPT_AOV_OBJECT)) out.object[pixel] = obj;
    if (obj < 0) continue;
    const double t = ps.hit[slot];
    D3 nrm = mk(0, 0, 0), o = mk(0, 0, 0), d = mk(0, 0, 0);
    if (ch & RPT_AOV_NORMAL) nrm = ld_soa3(ps.hit + ps.cap, ps.cap, slot);
    if (ch & RPT_AOV_POSITION) {
      o = ld_soa3(ps.ray, ps.cap, slot);
      d = ld_soa3(ps.ray + 3 * ps.cap, ps.cap, slot);
    }
    aov_add(sc, ch, o, d, t, nrm, obj, hits, depth, normal, albedo, position);
  }
  aov_store(out, pixel, hits, depth, normal, albedo, position);
}
