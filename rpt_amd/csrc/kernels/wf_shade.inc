// kernels/wf_shade.inc — rpt_shade and rpt_shade_seeded: ONE text, included twice by wavefront.inc, with RPT_WF_SEEDED 0
// and 1 (why not a template: wf_raygen_views.inc).
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// trace_ray's body for one depth (renderer.rs:147-168).
// The stream's seed is fr.seed (rpt_shade) — or seeds[p_local], what rpt_raygen_views_seeded wrote for the path's index of
// the piece (rpt_shade_seeded; fr.seed is not read).  Nothing else in the depth loop reads a seed.
// sq / counters[2 + l]: per light, the queue of the paths that cast a shadow ray towards it at this depth ([light][cap])
// and its length: every hit whose light could add something (see null_contribution).  The visibility queries of the
// depth run over these queues, not over the path queue.
#if RPT_WF_SEEDED
#define RPT_WF_KERNEL(name) name##_seeded
#else
#define RPT_WF_KERNEL(name) name
#endif
__global__ void __launch_bounds__(SHADE_BLOCK, RPT_SHADE_WAVES) RPT_WF_KERNEL(rpt_shade)(Scene sc, Frame fr, PathState ps, const uint32_t* __restrict__ queue,
                                                 uint32_t n, uint32_t depth, uint32_t* __restrict__ next_queue,
                                                 uint32_t* __restrict__ counters /* [0]=next count, [1]=hits, [2+l]=shadow rays of light l */,
                                                 uint32_t* __restrict__ sq, uint32_t* __restrict__ zero_next, uint32_t zero_n,
                                                 uint32_t rec_off /* first record column of this depth: path i of the queue writes column rec_off + i */
#if RPT_WF_SEEDED
                                                 , const uint64_t* __restrict__ seeds /* [fr.npix]: the seed of each index of the piece */
#endif
                                                 ) {
  constexpr int FAST_LIGHTS = 30; // lights whose queue bit fits the one combined append (bits 2..31)
  // the NEXT depth's counters — the other of two sets (api_render.cpp): the host has read them back (it waits for every
  // depth's counts) before this launch, and nothing touches them until the next depth's rpt_shade.  One memset per depth less.
  if (blockIdx.x == 0 && zero_next) for (uint32_t k = threadIdx.x; k < zero_n; k += blockDim.x) zero_next[k] = 0u;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool active = i < n;
  const uint32_t slot = i; // dense state: the path's position at this depth (`queue` is the identity, kept for the signature)
  (void)queue;
  (void)next_queue;
  uint32_t bits = 0; // bit 0: the path continues, bit 1: it hit something, bit 2 + l: it casts a shadow ray to light l
  uint32_t path = 0, next_draw = 0;
  D3 next_o = mk(0, 0, 0), next_d = mk(0, 0, 0);
  const uint64_t col = (uint64_t)rec_off + i; // this path's record of this depth; linked to its record one depth up
  if (active) {
    path = ps.pid[slot];
    ps.rec_parent[col] = depth ? ps.col[slot] : REC_NONE;
    D3 o = ld_soa3(ps.ray, ps.cap, slot);
    D3 d = ld_soa3(ps.ray + 3 * ps.cap, ps.cap, slot);
    int obj = ps.hit_obj[slot];
    // the hit record, the stream position and the pixel (rpt_shade_seeded: and the path's seed) are requested together with
    // the ray, before the hit / miss branch: one round trip to the path state instead of three
    const double t = ps.hit[slot];
    const D3 nrm = ld_soa3(ps.hit + ps.cap, ps.cap, slot);
    const uint32_t s_local = path / fr.npix, p_local = path - s_local * fr.npix;
    const uint32_t pixel = fr.pixels[p_local], draw0 = ps.draw[slot];
#if RPT_WF_SEEDED
    // (as two words: loaded as one u64 and taken apart by rng_make, the key wants an aligned register pair of its own for
    // the whole hit branch — 8 VGPRs spilled at RPT_SHADE_WAVES' 168 where this form spills none, DESIGN.md §15.1)
    const uint2 key = reinterpret_cast<const uint2*>(seeds)[p_local];
    const uint64_t seed = ((uint64_t)key.y << 32) | key.x;
#else
    const uint64_t seed = fr.seed;
#endif
    if (obj < 0) { // renderer.rs:147
      D3 e = env_color(sc, d);
      st_rec3(ps, 0, col, e);
    } else {
      bits |= 2u;
      Rng rng = rng_make(seed, pixel, fr.sample_base + s_local, draw0);
      D3 world_pos = o + t * d;                  // renderer.rs:149
      const Material& mat = sc.materials[sc.insts[obj].material];
      D3 wo = -normalize(d);                     // renderer.rs:151
      D3 emit = mat.emittance * ld3(mat.color);  // renderer.rs:153
      st_rec3(ps, 0, col, emit);
      // sample_lights (renderer.rs:177-204): everything except the visibility test
      for (int l = 0; l < sc.num_lights; l++) {
        CLight& light = clight(sc, l);
        double* sh = ps.shadow + (uint64_t)l * SHADOW_FIELDS * ps.cap;
        if (light.kind == RPT_LIGHT_AMBIENT) {
          st_soa3(sh + 4 * ps.cap, ps.cap, slot, cmul(ld3(light.color), ld3(mat.color)));
        } else {
          D3 intensity, wi;
          double dist;
          illuminate(sc, light, world_pos, rng, intensity, wi, dist);
          D3 f = bsdf(mat, nrm, wo, wi);
          const D3 contrib = cmul(f, intensity) * dot(wi, nrm); // renderer.rs:199
          st_soa3(sh, ps.cap, slot, wi);
          sh[3 * ps.cap + slot] = dist;
          st_soa3(sh + 4 * ps.cap, ps.cap, slot, contrib);
          if (l < FAST_LIGHTS && !null_contribution(contrib)) bits |= 4u << l;
        }
      }
      st_soa3(ps.ray, ps.cap, slot, world_pos); // origin of the shadow rays and of the next ray
      if (depth < fr.max_bounces) {             // renderer.rs:155
        D3 wi;
        double pdf;
        if (sample_f(mat, nrm, wo, rng, wi, pdf)) {
          D3 f = bsdf(mat, nrm, wo, wi);
          st_rec3(ps, 3, col, f);
          ps.rec[col * REC_FIELDS + 6] = 1.0 / pdf;
          ps.rec[col * REC_FIELDS + 7] = fabs(dot(wi, nrm));
          next_o = world_pos; next_d = wi;
          bits |= 1u;
        }
      }
      next_draw = rng.draw;
    }
    if (!(bits & 1u)) ps.last_col[path] = (uint32_t)col; // the path ends with this record: where rpt_resolve starts
  }
  const uint32_t j = block_multi_push(bits, 2 + min(sc.num_lights, FAST_LIGHTS), slot, counters, sq, ps.cap, 0);
  if (bits & 1u) { // the survivor's state, at its position in the next depth
    if (ps.next_rows) {
      // in-kernel-traversal scenes (path re-order): one 64-byte row, and the key the re-order sorts by while the ray is
      // in registers
      double* row = ps.next_rows + (uint64_t)j * 8u;
      row[0] = next_o.x; row[1] = next_o.y; row[2] = next_o.z; row[3] = next_d.x; row[4] = next_d.y; row[5] = next_d.z;
      row[6] = pack_u32(next_draw, path);
      row[7] = pack_u32((uint32_t)col, 0u);
      SceneBox box;
#pragma unroll
      for (int k = 0; k < 6; k++) box.bounds[k] = ps.key_bounds[k];
      ps.sort_keys[j] = ray_sort_key(box, next_o, next_d, 0.0);
      ps.sort_vals[j] = j;
    } else {
      st_soa3(ps.ray_next, ps.cap, j, next_o);
      st_soa3(ps.ray_next + 3 * ps.cap, ps.cap, j, next_d);
      ps.draw_next[j] = next_draw;
      ps.pid_next[j] = path;
      ps.col_next[j] = (uint32_t)col;
    }
  }
  // scenes with more lights than one append holds: the rest in further appends, from the stored contributions
  for (int l0 = FAST_LIGHTS; l0 < sc.num_lights; l0 += FAST_LIGHTS) {
    const int nl = min(sc.num_lights - l0, FAST_LIGHTS);
    uint32_t more = 0;
    if (bits & 2u)
      for (int k = 0; k < nl; k++) {
        const double* sh = ps.shadow + (uint64_t)(l0 + k) * SHADOW_FIELDS * ps.cap;
        if (clight(sc, l0 + k).kind != RPT_LIGHT_AMBIENT && !null_contribution(ld_soa3(sh + 4 * ps.cap, ps.cap, slot))) more |= 4u << k;
      }
    (void)block_multi_push(more, 2 + nl, slot, counters, sq, ps.cap, l0);
  }
}
#undef RPT_WF_KERNEL
