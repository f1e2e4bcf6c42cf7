// kernels/direct.inc — direct light at the caller's points: rptgpu_bake_direct and the lightmap form (include/rpt_gpu_direct.h,
// DESIGN.md §23).  sample_lights (renderer.rs:177-204) without a hit in front of it: rpt_raygen_direct does for a (sample,
// point) slot what rpt_shade does for a hit — illuminate() light after light on the slot's stream, each light's wi, dist and
// contribution into its column of ps.shadow (SHADOW_FIELDS), the slot into the queues of the lights that can add something —
// with `I * cos` where rpt_shade has `bsdf * I * cos`; the query between the two kernels is a render's own (api_direct.cpp);
// rpt_direct_fold reads the columns and srt the way rpt_shadow_sum reads them.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// slot = s_local * npix + p_local (rpt_raygen_ao's order) is light sample fr.sample_base + s_local of point p_local of the
// piece, from draw 0 of its stream; the stream id is ids[p_local] (the caller's, offset to the piece) or id_base + p_local.
// counters: [2 + l] the length of light l's queue (sq + l * cap), cleared by the driver before the launch.
// A wave takes DIRECT_GROUPS runs of 64 consecutive slots and appends to a light's queue ONCE for all of them: one atomic on
// one address per wave and run was 262 144 atomics per light for a pass of 16 Mi slots, and at the ~88 per microsecond a single
// address takes (wf_state.inc) that was 3 ms per light — the whole kernel's time, twelve times rpt_raygen_ao's.  The
// contributions are read back from the columns the lanes just wrote (each lane reads its own stores)
constexpr uint32_t DIRECT_GROUPS = 16;
__global__ void __launch_bounds__(256) rpt_raygen_direct(Scene sc, Frame fr, const double* __restrict__ positions,
                                                         const double* __restrict__ normals, const uint32_t* __restrict__ ids,
                                                         uint32_t id_base, PathState ps, uint32_t* __restrict__ sq,
                                                         uint32_t* __restrict__ counters, uint32_t n_slots) {
  const uint32_t lane = __lane_id();
  // the wave's first slot (the grid covers n_slots / DIRECT_GROUPS threads, rounded up: launch_raygen_direct)
  const uint64_t first = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x - lane) * DIRECT_GROUPS + lane;
  for (uint32_t j = 0; j < DIRECT_GROUPS; j++) {
    const uint64_t slot = first + (uint64_t)j * 64u;
    if (slot >= n_slots) break; // (slots ascend with j: nothing of this lane's is left)
    const uint32_t s_local = (uint32_t)slot / fr.npix, p_local = (uint32_t)slot - s_local * fr.npix;
    const uint32_t id = ids ? ids[p_local] : id_base + p_local;
    Rng rng = rng_make(fr.seed, id, fr.sample_base + s_local, 0);
    const D3 pos = ld3(positions + 3 * (uint64_t)p_local);
    const D3 nn = normalize(ld3(normals + 3 * (uint64_t)p_local));
    st_soa3(ps.ray, ps.cap, slot, pos); // the origin of every light's shadow ray
    for (int l = 0; l < sc.num_lights; l++) {
      CLight& light = clight(sc, l);
      if (light.kind == RPT_LIGHT_AMBIENT) continue; // no draw, no ray (its queue stays empty)
      D3 intensity, wi;
      double dist;
      illuminate(sc, light, pos, rng, intensity, wi, dist); // (draws whether or not the light faces the point)
      const double cosv = dot(wi, nn);
      const D3 c = cosv > 0.0 ? intensity * cosv : mk(0, 0, 0); // (false for NaN: +0.0, which is never queued)
      double* sh = ps.shadow + (uint64_t)l * SHADOW_FIELDS * ps.cap;
      st_soa3(sh, ps.cap, slot, wi);
      sh[3 * ps.cap + slot] = dist;
      st_soa3(sh + 4 * ps.cap, ps.cap, slot, c);
    }
  }
  // the appends, light by light (wave-uniform from here on: every lane of the wave walks every run).  A ray that can add
  // only zero is not traced (null_contribution, wf_state.inc); the order of a queue is scheduling only
  for (int l = 0; l < sc.num_lights; l++) {
    if (clight(sc, l).kind == RPT_LIGHT_AMBIENT) continue;
    const double* sh = ps.shadow + (uint64_t)l * SHADOW_FIELDS * ps.cap;
    uint64_t masks[DIRECT_GROUPS];
    uint32_t total = 0;
#pragma unroll
    for (uint32_t j = 0; j < DIRECT_GROUPS; j++) {
      const uint64_t slot = first + (uint64_t)j * 64u;
      masks[j] = __ballot(slot < n_slots && !null_contribution(ld_soa3(sh + 4 * ps.cap, ps.cap, slot < n_slots ? slot : 0)));
      total += (uint32_t)__popcll(masks[j]);
    }
    if (!total) continue;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counters + 2 + l, total);
    base = __shfl(base, 0);
    uint32_t* __restrict__ q = sq + (uint64_t)l * ps.cap;
#pragma unroll
    for (uint32_t j = 0; j < DIRECT_GROUPS; j++) {
      if (masks[j] >> lane & 1ull) q[base + (uint32_t)__popcll(masks[j] & ((1ull << lane) - 1ull))] = (uint32_t)(first + (uint64_t)j * 64u);
      base += (uint32_t)__popcll(masks[j]);
    }
  }
}

// rpt_ao_fold's step for direct light: one thread per point of the piece, the pass's n_samples samples in ascending order
// (outer) and the lights in scene order (inner) into the point's running sum, which rests in fr.accum between the passes of a
// piece, SoA ([3][npix]); `first`: the sum starts at +0.0 here, `last`: it leaves divided by the call's S instead of being
// stored.  A contribution that is exactly zero was never queued and its srt entry is stale: adding it would change nothing
// (rpt_shadow_sum's argument: the sum starts at +0.0 and is never -0.0)
__global__ void __launch_bounds__(256) rpt_direct_fold(Scene sc, Frame fr, PathState ps, const double* __restrict__ srt,
                                                       uint32_t n_samples, int first, int last, uint32_t samples,
                                                       double* __restrict__ out) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= fr.npix) return;
  D3 acc = first ? mk(0, 0, 0) : ld_soa3(fr.accum, fr.npix, p);
  for (uint32_t s = 0; s < n_samples; s++) {
    const uint64_t slot = (uint64_t)s * fr.npix + p;
    for (int l = 0; l < sc.num_lights; l++) {
      if (clight(sc, l).kind == RPT_LIGHT_AMBIENT) continue;
      const double* sh = ps.shadow + (uint64_t)l * SHADOW_FIELDS * ps.cap;
      const D3 c = ld_soa3(sh + 4 * ps.cap, ps.cap, slot);
      if (null_contribution(c)) continue;
      if (srt[(uint64_t)l * ps.cap + slot] > light_stop(sh[3 * ps.cap + slot])) acc = acc + c; // renderer.rs:197 (false for a NaN hit)
    }
  }
  if (!last) {
    st_soa3(fr.accum, fr.npix, p, acc);
    return;
  }
  const double S = (double)samples;
  out[3 * (uint64_t)p] = acc.x / S;
  out[3 * (uint64_t)p + 1] = acc.y / S;
  out[3 * (uint64_t)p + 2] = acc.z / S;
}
