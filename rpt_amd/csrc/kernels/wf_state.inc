// kernels/wf_state.inc — what the wavefront pipeline's kernels share: access to the SoA path state and the depth records,
// null_contribution, and the queue appends (one wave's, one block's, several queues of one block at once).
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ state access
RPT_DEV D3 ld_soa3(const double* base, uint64_t cap, uint64_t slot) {
  return {base[slot], base[cap + slot], base[2 * cap + slot]};
}
RPT_DEV void st_soa3(double* base, uint64_t cap, uint64_t slot, D3 v) {
  base[slot] = v.x;
  base[cap + slot] = v.y;
  base[2 * cap + slot] = v.z;
}
RPT_DEV double pack_u32(uint32_t a, uint32_t b) { return __longlong_as_double((long long)((uint64_t)a | ((uint64_t)b << 32))); }
RPT_DEV void unpack_u32(double v, uint32_t& a, uint32_t& b) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  a = (uint32_t)u; b = (uint32_t)(u >> 32);
}
// depth records: fields f .. f + 2 of column c (PathState::rec).  A column is ONE 64-byte row — A[3], f[3], 1/pdf, |wi.n|
// side by side: rpt_shade's lanes write neighbouring rows (as coalesced as a field-major layout), and rpt_resolve, which
// walks a path's records along their parent links — anywhere in the pool once the paths of a depth are re-ordered —
// touches one 64-byte sector per record instead of eight.
RPT_DEV D3 ld_rec3(const PathState& ps, int f, uint64_t c) { const double* r = ps.rec + c * REC_FIELDS + f; return {r[0], r[1], r[2]}; }
RPT_DEV void st_rec3(const PathState& ps, int f, uint64_t c, D3 v) { double* r = ps.rec + c * REC_FIELDS + f; r[0] = v.x; r[1] = v.y; r[2] = v.z; }

// A shadow ray whose light would add exactly zero — bsdf = 0 because the light is below an opaque surface
// (material.rs:130-133), or a light sample facing away (light.rs:38-40) — cannot change the pixel whether it is
// occluded or not: sample_lights adds `bsdf * intensity * cos` (renderer.rs:199) to a sum that starts at +0, and
// x + (+-0) = x for every x that sum can hold (it is never -0).  The reference still traces it; rpt_shade leaves it
// out of the light's shadow-ray queue, so no kernel ever sees it, and rpt_shadow_sum may add its zero or not.  NaN
// or infinite contributions are not zero and are traced.  On closed meshes about half of the hit points face away
// from a given light: the queues hold 50-70 % of the reference's shadow rays.
RPT_DEV bool null_contribution(D3 c) { return c.x == 0.0 && c.y == 0.0 && c.z == 0.0; }

// append `slot` to a queue: one 64-bit ballot + one atomic per wave (wave64)
RPT_DEV void queue_push(bool pred, uint32_t slot, uint32_t* __restrict__ q, uint32_t* __restrict__ count) {
  uint64_t mask = __ballot(pred);
  if (mask == 0) return;
  uint32_t lane = __lane_id();
  uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(mask));
  base = __shfl(base, (int)leader);
  if (pred) q[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = slot;
}

// The same for a whole 1024-thread block: ONE global atomic per block (and one more for an optional second counter).
// A single address takes ~88 atomics per microsecond on this chip; with one atomic per wave the compaction kernels of a
// 60-Mi-ray depth spent milliseconds queueing on the counter (rpt_shade 6.6 ms, rpt_tree_enter 2.9 ms per launch).
// Every thread of the block must call this (no early returns before it).
constexpr int PUSH_BLOCK = 1024; // rpt_tree_enter: a light streaming kernel, the fewer atomics the better
constexpr int SHADE_BLOCK = 256; // rpt_shade: heavy lanes; 256 / 512 / 1024 -> 104 / 121 / 120 ms on the fractal spheres
// three waves per SIMD (168 VGPRs): the kernel streams scattered path state and waits half of its cycles.  Round 3's
// build happened to need exactly 168; round 4's sample_f needed 170 and silently ran at two waves (rpt_shade +10 %,
// 1-1.5 % of a C3 / C4 / C5 frame) until the bound was written down
#ifndef RPT_SHADE_WAVES
#define RPT_SHADE_WAVES 3
#endif
                                 // (a whole block waits at the two barriers for its slowest wave)
// q2 / v2: a second array that gets v2 at the same position (the ray sort's keys beside the queue's entries)
RPT_DEV void block_queue_push(bool pred, uint32_t slot, uint32_t* __restrict__ q, uint32_t* __restrict__ count,
                              bool pred2 = false, uint32_t* __restrict__ count2 = nullptr,
                              uint32_t* __restrict__ q2 = nullptr, uint32_t v2 = 0u) {
  __shared__ uint32_t s_cnt[PUSH_BLOCK / 64], s_cnt2[PUSH_BLOCK / 64], s_off[PUSH_BLOCK / 64];
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6, nw = (blockDim.x + 63u) >> 6;
  const uint64_t mask = __ballot(pred), mask2 = __ballot(pred2);
  if (lane == 0) { s_cnt[wave] = (uint32_t)__popcll(mask); s_cnt2[wave] = (uint32_t)__popcll(mask2); }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0, total2 = 0;
    for (uint32_t w = 0; w < nw; w++) { s_off[w] = total; total += s_cnt[w]; total2 += s_cnt2[w]; }
    uint32_t base = total ? atomicAdd(count, total) : 0u;
    for (uint32_t w = 0; w < nw; w++) s_off[w] += base;
    if (count2 && total2) atomicAdd(count2, total2);
  }
  __syncthreads();
  if (pred && q) {
    const uint32_t pos = s_off[wave] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    q[pos] = slot;
    if (q2) q2[pos] = v2;
  }
}

// Several queue appends of a SHADE_BLOCK-thread block at the price of one: queue q (q < nq <= 32) gets `slot` of every
// thread whose bit q of `bits` is set; one pair of barriers and one global atomic per queue and block, whatever nq is.
// q = 0: the next depth's path queue, q = 1: the hit counter (no queue behind it), q = 2 + k: the shadow-ray queue of
// light first_light + k.  Every thread of the block must call this.
// Returns the calling thread's position in queue 0 (the next depth's paths) when its bit 0 is set: with dense path state
// nothing is stored for that queue — the position IS where the thread writes its path's next state.
RPT_DEV uint32_t block_multi_push(uint32_t bits, int nq, uint32_t slot, uint32_t* __restrict__ counters,
                                  uint32_t* __restrict__ sq, uint64_t cap, int first_light) {
  constexpr int NW = SHADE_BLOCK / 64;
  __shared__ uint32_t s_cnt[32][NW], s_off[32][NW];
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  for (int q = 0; q < nq; q++) {
    const uint64_t mask = __ballot((bits >> q) & 1u);
    if (lane == 0) s_cnt[q][wave] = (uint32_t)__popcll(mask);
  }
  __syncthreads();
  if ((int)threadIdx.x < nq) { // one thread per queue: scan the waves' counts, reserve the block's range
    const int q = (int)threadIdx.x;
    uint32_t total = 0;
    for (int w = 0; w < NW; w++) { s_off[q][w] = total; total += s_cnt[q][w]; }
    uint32_t* ctr = q < 2 ? counters + q : counters + 2 + first_light + (q - 2);
    const uint32_t base = total ? atomicAdd(ctr, total) : 0u;
    for (int w = 0; w < NW; w++) s_off[q][w] += base;
  }
  __syncthreads();
  uint32_t pos0 = 0;
  for (int q = 0; q < nq; q++) {
    if (q == 1) continue; // the hit counter has no queue
    const bool mine = (bits >> q) & 1u;
    const uint64_t mask = __ballot(mine);
    if (mine) {
      const uint32_t pos = s_off[q][wave] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (q == 0) pos0 = pos;
      else (sq + (uint64_t)(first_light + q - 2) * cap)[pos] = slot;
    }
  }
  return pos0;
}
