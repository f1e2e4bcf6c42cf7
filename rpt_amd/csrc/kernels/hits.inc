// kernels/hits.inc — first-hit records for the caller: rptgpu_first_hits and rptgpu_render_views_aov (include/rpt_gpu.h,
// DESIGN.md §17).  The closest-hit query is a render's own — closest_hit<KdLdsW> as rpt_extend calls it, or the per-tree query
// behind rpt_raygen_rays / rpt_raygen_views (api_hits.cpp) —; these kernels only carry its record into the caller's layout:
// rpt_first_hits (fused: ray in, record out, nothing through the path state), rpt_hits_store (the record from the path
// state), rpt_views_aov_fold (rpt_aov_fold's sequence of additions, addressed by the piece's index).  The channel mask is
// a kernel argument (wave-uniform): a channel that is not asked for is neither computed nor stored, and its pointer is
// never read.  Part of kernels.inc (inside namespace RPT_NS).

// ray i's record into the named channels; o, d: the ray the record belongs to.  A hit is obj >= 0 (a NaN time is one)
RPT_DEV void hit_store(const Scene& sc, const HitOut& out, uint32_t i, D3 o, D3 d, double t, D3 nrm, int obj) {
  const uint32_t ch = out.channels;
  const uint64_t i3 = 3ull * i;
  if (ch & RPT_HIT_T) out.t[i] = t;
  if (ch & RPT_HIT_NORMAL) { out.normal[i3] = nrm.x; out.normal[i3 + 1] = nrm.y; out.normal[i3 + 2] = nrm.z; }
  if (ch & RPT_HIT_OBJECT) out.object[i] = obj;
  if (ch & RPT_HIT_POSITION) {
    D3 p = mk(0, 0, 0);
    if (obj >= 0) p = o + t * d; // Ray::at (shape.rs:59-61): one multiply, one add — aov_add's expression
    out.position[i3] = p.x; out.position[i3 + 1] = p.y; out.position[i3 + 2] = p.z;
  }
  if (ch & RPT_HIT_ALBEDO) {
    D3 a = mk(0, 0, 0);
    if (obj >= 0) {
      const Material& mat = sc.materials[sc.insts[obj].material];
      a = mk(mat.color[0], mat.color[1], mat.color[2]);
    }
    out.albedo[i3] = a.x; out.albedo[i3 + 1] = a.y; out.albedo[i3 + 2] = a.z;
  }
}

// In-kernel scenes: the caller's ray ([n][3] f64, already offset to the piece, used as given), the closest hit and the
// record's channels in one kernel, in rpt_extend's shape (256-thread blocks, the kd stack's first levels in LDS)
__global__ void __launch_bounds__(256, RPT_WF_WAVES) rpt_first_hits(Scene sc, const double* __restrict__ origins,
                                                                    const double* __restrict__ dirs, uint32_t n, HitOut out) {
  __shared__ KdLdsW kd_lds;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  D3 o = ld3(origins + 3 * (uint64_t)i), d = ld3(dirs + 3 * (uint64_t)i);
  double t;
  D3 nrm;
  int obj = closest_hit<KdLdsW>(sc, o, d, t, nrm, &kd_lds);
  hit_store(sc, out, i, o, d, t, nrm, obj);
}

// Scenes with deep trees: the records of the n rays rpt_raygen_rays laid into the path state (one sample: slot = the ray's
// position in the piece) after the closest-hit query; the ray is re-read from the origin / direction columns
__global__ void __launch_bounds__(256) rpt_hits_store(Scene sc, PathState ps, uint32_t n, HitOut out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t ch = out.channels;
  const int obj = ps.hit_obj[i];
  const double t = ps.hit[i];
  D3 nrm = mk(0, 0, 0), o = mk(0, 0, 0), d = mk(0, 0, 0);
  if (ch & RPT_HIT_NORMAL) nrm = ld_soa3(ps.hit + ps.cap, ps.cap, i);
  if ((ch & RPT_HIT_POSITION) && obj >= 0) {
    o = ld_soa3(ps.ray, ps.cap, i);
    d = ld_soa3(ps.ray + 3 * ps.cap, ps.cap, i);
  }
  hit_store(sc, out, i, o, d, t, nrm, obj);
}

// rptgpu_render_views_aov: one pass's hits (rpt_raygen_views' rays, the closest-hit query's records; slot = s_local * n + j)
// added to the running sums of index j of the piece, one lane per j over the pass's `spp` samples in ascending order —
// rpt_aov_fold's sequence of additions, with the sums at j of `out` (the arrays offset to the piece) instead of at a pixel
// of a frame.  first: the pass holds the call's first sample (the sums start at +0.0 here and `object` is that sample's);
// every j of the piece is stored, so nothing has to be zeroed beforehand.
__global__ void __launch_bounds__(256) rpt_views_aov_fold(Scene sc, PathState ps, AovOut out, uint32_t n, uint32_t spp, int first) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t ch = out.channels;
  const uint64_t j3 = 3ull * j;
  uint32_t hits = 0u;
  double depth = 0.0;
  D3 normal = mk(0, 0, 0), albedo = mk(0, 0, 0), position = mk(0, 0, 0);
  if (!first) {
    hits = out.hits[j];
    if (ch & RPT_AOV_DEPTH) depth = out.depth[j];
    if (ch & RPT_AOV_NORMAL) normal = mk(out.normal[j3], out.normal[j3 + 1], out.normal[j3 + 2]);
    if (ch & RPT_AOV_ALBEDO) albedo = mk(out.albedo[j3], out.albedo[j3 + 1], out.albedo[j3 + 2]);
    if (ch & RPT_AOV_POSITION) position = mk(out.position[j3], out.position[j3 + 1], out.position[j3 + 2]);
  }
  for (uint32_t s = 0; s < spp; s++) {
    const uint64_t slot = (uint64_t)s * n + j;
    const int obj = ps.hit_obj[slot];
    if (s == 0u && first && (ch & RPT_AOV_OBJECT)) out.object[j] = obj;
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
  aov_store(out, j, hits, depth, normal, albedo, position);
}
