// kernels/occlusion.inc — visibility for the caller: rptgpu_occluded and rptgpu_bake_ao (include/rpt_gpu.h, DESIGN.md §16).
// These kernels only lay rays where a depth's shadow rays lie — origin in ps.ray, direction and stop in column 0 of ps.shadow
// (SHADOW_FIELDS: wi[3], dist), the identity in light 0's queue with its length on the device — and read the answers back:
// the query between them is a render's own, rpt_shadow_rays or the per-tree query (api_occlusion.cpp), and its record times
// come back in srt's column 0: -inf / +inf from rpt_shadow_rays, the record's time (a hit, +inf, NaN) from the per-tree
// kernels.  Both are read the way rpt_shadow_sum reads them: visible = srt > light_stop(dist), false for a NaN record.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

RPT_DEV bool occ_visible(const PathState& ps, const double* __restrict__ srt, uint64_t slot) {
  return srt[slot] > light_stop(ps.shadow[3 * ps.cap + slot]);
}

// a piece of the caller's rays ([n][3] f64, already offset to the piece; max_t may be null: +inf), used as given
__global__ void __launch_bounds__(256) rpt_occ_load(const double* __restrict__ origins, const double* __restrict__ dirs,
                                                    const double* __restrict__ max_t, PathState ps, uint32_t* __restrict__ sq,
                                                    uint32_t* __restrict__ sq_count, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_soa3(ps.ray, ps.cap, i, ld3(origins + 3 * (uint64_t)i));
  st_soa3(ps.shadow, ps.cap, i, ld3(dirs + 3 * (uint64_t)i));
  ps.shadow[3 * ps.cap + i] = max_t ? max_t[i] : INF;
  sq[i] = i;
  if (i == 0) *sq_count = n;
}

// The same for ambient occlusion: slot = s_local * npix + p_local (rpt_raygen_probes' order) is direction fr.sample_base +
// s_local of point p_local of the piece, RPT_PROBE_IRRADIANCE's direction from draw 0 of its stream; the stream id is
// ids[p_local] (the caller's, offset to the piece) or id_base + p_local.  Every ray stops at max_distance.
__global__ void __launch_bounds__(256) rpt_raygen_ao(Frame fr, const double* __restrict__ positions, const double* __restrict__ normals,
                                                     const uint32_t* __restrict__ ids, uint32_t id_base, double max_distance,
                                                     PathState ps, uint32_t* __restrict__ sq, uint32_t* __restrict__ sq_count,
                                                     uint32_t n_slots) {
  uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_slots) return;
  uint32_t s_local = slot / fr.npix, p_local = slot - s_local * fr.npix;
  const uint32_t id = ids ? ids[p_local] : id_base + p_local;
  Rng rng = rng_make(fr.seed, id, fr.sample_base + s_local, 0);
  const D3 dir = probe_direction(RPT_PROBE_IRRADIANCE, ld3(normals + 3 * (uint64_t)p_local), rng);
  st_soa3(ps.ray, ps.cap, slot, ld3(positions + 3 * (uint64_t)p_local));
  st_soa3(ps.shadow, ps.cap, slot, dir);
  ps.shadow[3 * ps.cap + slot] = max_distance;
  sq[slot] = slot;
  if (slot == 0) *sq_count = n_slots;
}

// rptgpu_occluded's answers: one byte per ray of the piece, 1 = occluded
__global__ void __launch_bounds__(256) rpt_occ_store(PathState ps, const double* __restrict__ srt, uint32_t n, uint8_t* __restrict__ out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = occ_visible(ps, srt, i) ? (uint8_t)0 : (uint8_t)1;
}

// rpt_resolve_probes' step for ambient occlusion: one thread per point of the piece, the pass's n_samples directions in
// ascending order into the point's running sums — the count of visible directions (an integer in an f64) and their sum —
// which rest in fr.accum between the passes of a piece, SoA ([4][npix]); `first`: the sums start at +0.0 here, `last`: they
// leave divided by the call's S (out_bent may be null) instead of being stored
__global__ void __launch_bounds__(256) rpt_ao_fold(Frame fr, PathState ps, const double* __restrict__ srt, uint32_t n_samples,
                                                   int first, int last, uint32_t samples, double* __restrict__ out_ao,
                                                   double* __restrict__ out_bent) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= fr.npix) return;
  double count = first ? 0.0 : fr.accum[p];
  D3 acc = first ? mk(0, 0, 0) : ld_soa3(fr.accum + fr.npix, fr.npix, p);
  for (uint32_t s = 0; s < n_samples; s++) {
    const uint64_t slot = (uint64_t)s * fr.npix + p;
    if (occ_visible(ps, srt, slot)) {
      count = count + 1.0;
      acc = acc + ld_soa3(ps.shadow, ps.cap, slot);
    }
  }
  if (!last) {
    fr.accum[p] = count;
    st_soa3(fr.accum + fr.npix, fr.npix, p, acc);
    return;
  }
  const double S = (double)samples;
  out_ao[p] = count / S;
  if (out_bent) {
    out_bent[3 * (uint64_t)p] = acc.x / S;
    out_bent[3 * (uint64_t)p + 1] = acc.y / S;
    out_bent[3 * (uint64_t)p + 2] = acc.z / S;
  }
}
