// kernels/paths.inc — the persistent path kernel rpt_paths<KdLds|KdFlat>: contract, work hand-out, record ring, parked lookups,
// ray stash, the fused kernels' wave-level pool of pre-traced hits, the loop; rpt_sum_samples.  (Its flat-scene queries, tables and fast shading: paths_flat / _consts / _shade.inc.)
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ persistent path kernel
// The MI355X-first form of Renderer::sample (renderer.rs:117-129).  A work item is a run of
// `chunk` consecutive samples of one pixel; a lane owns one item at a time and waves are
// persistent: a lane that finished its item pulls the next one from a global counter (through its
// wave's pool of claimed items: fetch_item), the GPU analogue of rayon's per-row work stealing at a granularity fine
// enough that the tail of a launch is a few samples, not a whole pixel (this matters when a GPU
// owns few pixels per lane: small frames, or 1/8 of a frame under the multi-GPU partition).
// The whole path lives in registers; per-path memory traffic is the depth record (A, f, 1/pdf,
// |wi.n|) needed to fold the nested firefly clamp back to front (renderer.rs:162-167), laid out
// [thread][depth][field] (one 64-byte record per lane and depth: the lanes of a wave are at different
// depths, so a lane's own records are what is contiguous), plus one
// 24-byte store of the finished sample's radiance into lbuf[sample][channel][pixel];
// rpt_sum_samples then adds a pixel's samples in sample order, which is the reference's
// `color += ...` loop (renderer.rs:136-140) without atomics and independent of the schedule.
// Every loop iteration runs the same phases for every lane (generate if needed -> closest hit ->
// shade + shadow rays -> fold if the path ended), so lanes at different depths and samples stay
// converged.
//
// The nested clamp is folded by a per-lane WALKER, one depth level per loop iteration (round 4).  trace_ray's
// recursion unwinds back to front — L_k = A_k + min(1/pdf_k * (f_k . L_{k+1}) * |wi_k.n_k|, 100), renderer.rs:162-167 —
// so a path that ends D bounces deep owes D dependent steps.  Run on the spot, that loop kept the ~6 lanes whose
// paths had just ended busy while the other 58 waited (11 % of the kernel on C2).  Now an ended path only leaves
// its terminal radiance behind, the lane starts its next sample in the next iteration, and every iteration ends
// with ONE fold step for every lane that owes one: about 50 lanes per step, and the record's trip through global
// memory is paid once per iteration instead of once per level.  Depth records and the headers of paths that wait
// for the walker live in a per-lane ring of 64-byte slots, [thread][slot][field]: a path takes slot b for its
// header and b+1.. for its records.  Per path the same operations in the same order as before, hence the same bits.
// Ring size: let U = records not yet folded, C = records of the running path.  An iteration adds at most one
// record and, whenever U > 0, folds one, so U + C <= max_bounces (+1 inside an iteration).  Slots between the
// walker's path and the write position: the walker's own path (<= max_bounces + 1, part of it already folded),
// the waiting paths' records and headers (each waits with >= 1 record: <= 2 U), the running path (C + 1)
// — <= 3 max_bounces + 2 = rpt_fold_ring_slots() (launch_limits.h; api_render.cpp sizes the buffer with it).
// With pre-traced camera rays (PRETRACE below) a lane can end two paths in one iteration: the one whose ray escaped, at
// the swap, and the stashed one it takes — but that one starts at depth 0 in this iteration, so it either ends there
// (no record, no header: its sample goes straight to lbuf) or writes its level-0 record.  Still at most one record per
// iteration, every header written (path_ended) before the fold step of the same iteration, and the bound above stands
// (tests/test_ray_stash_swap_model.py).
// With the fused query (FUSE below) an iteration runs: take the hit (the previous iteration's bounce result, or the
// stashed one: a path whose bounce ray escaped ends here, at the swap, as above) -> shade it and write the record's f,
// 1/pdf and |wi.n| -> the two-ray query -> the record's A, or the path's end -> one fold step.  The record of level
// `depth` is the only one written in the iteration, and into the slot it had before, so per lane and iteration the ring
// sees the same events in the same order as above: at most one record, the headers before the fold step; the bound
// stands.
// With the wave-level pool of pre-traced hits (POOL below, RPT_HIT_POOL: the fused kernels) the pop takes the swap's place:
// a lane whose bounce ray escaped ends that path when it pops a hit, and the popped path starts at depth 0 in the same
// iteration — by whichever lane generated it, which the ring, private to the lane that RUNS a path, never sees.  Still at
// most one record per lane and iteration and every header before the fold step: rpt_fold_ring_slots() and
// tests/test_ray_stash_swap_model.py hold as they are.
//
// Environment lookups are PARKED (round 5; flat scenes whose environment is a texture).  A ray that escapes ends its
// path with Hdri::get_color (environment.rs:25-52: atan2, acos, four texels) — one round of it per loop iteration for
// the lanes whose ray just escaped while the others wait: in a scene of mostly escaping rays (glass.rs) a fifth of the
// kernel at 40 of 64 lanes.  Here a lane leaves (direction, depth, header slot, sample, pixel) in its queue of
// RPT_PARK_K entries in LDS and takes its next ray at once.  The wave DRAINS the queues together — when RPT_PARK_FLUSH
// requests wait, or when a lane must have its queue empty: it is full and the lane's ray escaped again, its path
// ended otherwise (paths leave a lane in the order they entered it: the walker takes headers in ring order), it ran
// out of work, or the running path's records and the parked ones' together would exceed max_bounces (which keeps
// unfolded + parked + running records <= max_bounces and with it the ring bound above: a parked path counts as a
// waiting one).  A drain numbers the requests through the wave (prefix sums of the lanes' counts), lane j of round r
// looks up request 64 r + j — whoever owns it — and leaves the colour where the direction was; then every lane ends
// its parked paths in order.  Rounds of 64 lookups instead of 40: the same lookups on the same directions, the same
// folds, the same bits.
#ifndef RPT_PARK_FLUSH
#define RPT_PARK_FLUSH 160
#endif
struct ParkLds { // the lanes' queues, [entry][field][lane]
  double d[RPT_PARK_K][3][64];   // the escaped ray's direction; after a drain's rounds the looked-up colour
  uint32_t u[RPT_PARK_K][4][64]; // depth, header slot, sample, pixel of its path
  uint8_t list[RPT_PARK_K * 64]; // a drain's requests in (lane, entry) order: lane | entry << 6
};
static_assert(sizeof(ParkLds) == RPT_PATHS_PARK_LDS, "kernels.h sizes the wave's LDS budget with it");
static_assert(RPT_PARK_K >= 1 && RPT_PARK_K <= 4, "two bits for the entry in ParkLds::list, three for a lane's count");
struct PersistArgs {
  uint32_t* work_counter; // next work item
  double* rec;            // [nthreads][ring][REC_FIELDS]: depth records and waiting paths' headers
  unsigned long long* ray_counters; // [0] closest-hit rays, [1] shadow rays
  double* lbuf;           // [spp][3][npix] radiance of every sample of this launch
  uint32_t spp;           // samples per pixel in this launch
  uint32_t chunk;         // samples per work item
  uint32_t n_items;       // npix * ceil(spp / chunk); item i = (chunk i / npix, pixel i % npix)
  uint32_t nthreads;
  uint32_t ring;          // slots per thread in rec: fold_ring_slots(max_bounces)
  uint32_t batch;         // work items a wave claims at a time (fetch_item)
  uint32_t park_off;      // byte offset of the lanes' parked environment lookups (ParkLds) in the dynamic LDS; ~0u = lookups on the spot
  FlatLayout flat;        // flat instantiations: what goes where in the wave's dynamic LDS
};

#ifndef RPT_PATHS_WAVES
#define RPT_PATHS_WAVES 2
#endif
template <class LDS> struct PathsLds { using type = LDS; };
template <> struct PathsLds<KdFlat> { struct type { int unused; }; };
// KdFlatG: the same kernel with the triangles (vertex normals, light sampling) left in GLOBAL memory, for flat scenes
// whose intersection records fit the wave's LDS share but not together with the 144-byte triangles (a room of 23
// polygons).  A second instantiation rather than a run-time switch: a pointer that is LDS or global by a flag turns
// every access through it into a flat load, which cost C2 1.3 %.
struct KdFlatG { static constexpr int levels = 0; };
template <> struct PathsLds<KdFlatG> { struct type { int unused; }; };
// KdFlatF: KdFlatG behind the object filter (flat_query_filtered).  A third instantiation for the same reason: with
// the filtered query as a run-time branch of the one kernel C2 lost 0.9 % (966 against 974 Msamples/s).
struct KdFlatF { static constexpr int levels = 0; };
template <> struct PathsLds<KdFlatF> { struct type { int unused; }; };
// camera ray of sample `smp` of `pix` (renderer.rs:132-139, camera.rs:64-81): Renderer::get_color's jitter, Camera::cast_ray
RPT_DEV void camera_ray(const Frame& fr, const Camera& cam, double dim, uint32_t pix, uint32_t smp, D3& ro, D3& rd, Rng& rr) {
  uint32_t y = pix / fr.width, x = pix - y * fr.width;
  double xn = ((double)(2 * x + 1) - (double)fr.width) / dim;
  double yn = ((double)(2 * (fr.height - y) - 1) - (double)fr.height) / dim;
  rr = rng_make(fr.seed, pix, fr.sample_base + smp, 0);
  double dx = gen_range(rr, -1.0 / dim, 1.0 / dim);
  double dy = gen_range(rr, -1.0 / dim, 1.0 / dim);
  double px = xn + dx, py = yn + dy;
  D3 direction = ld3(cam.direction), up = ld3(cam.up), right = ld3(cam.right);
  ro = ld3(cam.eye);
  D3 new_dir = cam.d * direction + px * right + py * up;
  if (cam.aperture > 0.0) {
    D3 focal_point = ro + normalize(new_dir) * cam.focal_distance;
    double a, b;
    unit_disc(rr, a, b);
    ro = ro + (a * right + b * up) * cam.aperture;
    new_dir = focal_point - ro;
  }
  rd = normalize(new_dir);
}
// work hand-out, the persistent-thread fetch: the lanes of `want` each take the next work item; false = no item left.
// The wave keeps a POOL of items it has already claimed (round 5): one atomic on the global counter claims a batch,
// later requests are served from the pool with a ballot and a prefix count alone.  Before, every iteration in which a
// lane of the wave needed an item was an atomic on ONE address shared by the whole grid — in a scene of short paths
// (glass.rs: most rays escape at once) nearly every iteration of 2 048 waves, and the counter's L2 channel, not the
// arithmetic, set the kernel's pace (glass.rs 4 590 -> 7 500 Msamples/s, the 23-polygon room 671 -> 745).  A claim is
// pa.batch items — the host's choice, 1/32 of a wave's share of the launch within [16, 256]: a short launch (basic.rs,
// 4 ms) loses 4 % to pools of 128, a long one still gains from 128 -> 256 — and guided towards the end: never more than
// 1 / (4 x waves) of the items the wave last saw left, never less than what the asking lanes need, so the launch's tail
// stays about one item long.  Items claimed past the end are dead (every lane asks at most once past the end, and by
// then the claims are of the askers' size: at most 64 + 256 per wave, which the host's bound on n_items leaves room for).
struct ItemPool { uint32_t next, end, seen; }; // wave-uniform; seen: the counter after this wave's last claim
RPT_DEV bool fetch_item(const PersistArgs& pa, const Frame& fr, uint32_t lane, bool want, ItemPool& pool, uint32_t& f_p_local,
                        uint32_t& f_pixel, uint32_t& f_s, uint32_t& f_s_end) {
  bool got = false;
  const uint64_t need_mask = __ballot(want);
  if (need_mask) {
    const uint32_t n = (uint32_t)__popcll(need_mask), rank = (uint32_t)__popcll(need_mask & ((1ull << lane) - 1ull));
    const uint32_t avail = pool.end - pool.next;
    uint32_t idx = pool.next + rank;
    if (n > avail) { // (wave-uniform)
      const uint32_t left = pa.n_items - min(pa.n_items, pool.seen);
      const uint32_t more = max(n - avail, min(pa.batch, left / (pa.nthreads >> 4)));
      uint32_t base = 0;
      if (lane == (uint32_t)__ffsll((long long)need_mask) - 1u) base = atomicAdd(pa.work_counter, more);
      base = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(base, __ffsll((long long)need_mask) - 1));
      if (rank >= avail) idx = base + (rank - avail);
      pool.next = base + (n - avail);
      pool.end = base + more;
      pool.seen = pool.end;
    } else {
      pool.next += n;
    }
    if (want && idx < pa.n_items) {
      uint32_t c = idx / fr.npix;
      f_p_local = idx - c * fr.npix;
      f_pixel = fr.pixels[f_p_local];
      f_s = c * pa.chunk;
      f_s_end = min(f_s + pa.chunk, pa.spp);
      got = true;
    }
  }
  return got;
}
// ring arithmetic (top of this file): a path with header slot b keeps level k in slot b + 1 + k, and the next path's
// header comes behind its `depth` records; the running path's header slot is the high half of fold_st
RPT_DEV uint32_t next_header_slot(uint32_t b, uint32_t depth, uint32_t ring) {
  uint32_t nb = b + depth + 1u;
  if (nb >= ring) nb -= ring;
  return nb;
}
RPT_DEV uint32_t rec_slot(uint32_t fold_st, uint32_t depth, uint32_t ring) { // of level `depth` of the running path
  return next_header_slot(fold_st >> 16, depth, ring);
}
// a record's f, 1/pdf and |wi.n| (its A is r[0..2])
RPT_DEV void rec_store_bsdf(double* r, const D3& f, double inv_pdf, double abscos) {
  r[3] = f.x; r[4] = f.y; r[5] = f.z; r[6] = inv_pdf; r[7] = abscos;
}
// a path of `depth` levels ended with radiance A: the sample itself (depth 0), or the walker's next job — from
// registers if it is idle, else as a header in the path's slot b (the walker gets there in ring order)
RPT_DEV void path_ended(const PersistArgs& pa, const Frame& fr, double* __restrict__ rec, double (*fold_l)[64],
                        uint32_t (*fold_u)[64], uint32_t lane, uint32_t& fold_st, const D3& A, uint32_t depth, uint32_t b,
                        uint32_t s, uint32_t p_local) {
  if (depth == 0) { // nothing to fold: the sample is A
    double* lb = pa.lbuf + (uint64_t)s * 3 * fr.npix + p_local; // summed by rpt_sum_samples
    lb[0] = A.x;
    lb[fr.npix] = A.y;
    lb[2 * (uint64_t)fr.npix] = A.z;
  } else if ((fold_st & 0xffffu) == 0u) { // the walker is idle (so nothing waits either): it takes this path from registers
    fold_l[0][lane] = A.x; fold_l[1][lane] = A.y; fold_l[2][lane] = A.z;
    fold_u[0][lane] = depth; fold_u[1][lane] = b; fold_u[2][lane] = s; fold_u[3][lane] = p_local;
    fold_st |= depth;
  } else { // the path waits for the walker: its header goes into slot b
    double* r = rec + b * REC_FIELDS;
    r[0] = A.x; r[1] = A.y; r[2] = A.z;
    r[3] = __longlong_as_double((long long)((uint64_t)s | ((uint64_t)p_local << 32)));
    r[4] = __longlong_as_double((long long)depth);
  }
}
// an escaped ray's lookup joins the lane's queue (pcnt < RPT_PARK_K); its path keeps its header slot and records in
// the ring, so the next path's header comes after them
RPT_DEV void park_push(ParkLds& park, uint32_t lane, uint32_t& pcnt, uint32_t& park_hd, uint32_t& park_recs, uint32_t& fold_st,
                       uint32_t ring, const D3& d, uint32_t depth, uint32_t s, uint32_t p_local) {
  const uint32_t k = pcnt, b = fold_st >> 16;
  park.d[k][0][lane] = d.x; park.d[k][1][lane] = d.y; park.d[k][2][lane] = d.z;
  park.u[k][0][lane] = depth; park.u[k][1][lane] = b; park.u[k][2][lane] = s; park.u[k][3][lane] = p_local;
  if (depth != 0u) {
    if (park_hd == 0xffffffffu) park_hd = b; // the oldest parked header: where the walker stops
    park_recs += depth;
    fold_st = (fold_st & 0xffffu) | (next_header_slot(b, depth, ring) << 16);
  }
  pcnt = k + 1u;
}
// RPT_RAY_STASH (kernels.h): rpt_paths<KdFlat>'s next camera ray generated ahead (1), and traced ahead as well (2)
struct RayStash { // per lane, [field][lane]: origin, direction, the stream's cached half; work item, sample, draw counter
  double v[7][64];
  uint32_t u[5][64];
};
static_assert(sizeof(RayStash) == RPT_PATHS_STASH_LDS, "kernels.h sizes the wave's LDS budget with it");
// the pre-traced form (rpt_paths<KdFlat, false> under RPT_RAY_STASH=2): RayStash's fields, where v[0..2] holds the hit
// point o + t d once the ray is traced; v[7..9] the hit's normal, or the environment's colour if the ray escaped; u[5]
// the object hit (-1: escaped)
struct RayStashHit {
  double v[10][64];
  uint32_t u[6][64];
};
static_assert(sizeof(RayStashHit) == RPT_PATHS_STASH_HIT_LDS, "kernels.h sizes the wave's LDS budget with it");
// the stash's traffic, for either form (S = RayStash | RayStashHit): a ray (origin, direction)
template <class S> RPT_DEV void stash_put_pos(S& st, uint32_t lane, const D3& o) {
  st.v[0][lane] = o.x; st.v[1][lane] = o.y; st.v[2][lane] = o.z;
}
template <class S> RPT_DEV void stash_put_dir(S& st, uint32_t lane, const D3& d) {
  st.v[3][lane] = d.x; st.v[4][lane] = d.y; st.v[5][lane] = d.z;
}
template <class S> RPT_DEV void stash_put_ray(S& st, uint32_t lane, const D3& o, const D3& d) {
  stash_put_pos(st, lane, o);
  stash_put_dir(st, lane, d);
}
template <class S> RPT_DEV void stash_take_ray(const S& st, uint32_t lane, D3& o, D3& d) {
  o = mk(st.v[0][lane], st.v[1][lane], st.v[2][lane]);
  d = mk(st.v[3][lane], st.v[4][lane], st.v[5][lane]);
}
// the two-pass pre-trace: the stashed ray into (o, d), the running one into its slots meanwhile
template <class S> RPT_DEV void stash_swap_ray(S& st, uint32_t lane, D3& o, D3& d) {
  D3 so, sd;
  stash_take_ray(st, lane, so, sd);
  stash_put_ray(st, lane, o, d);
  o = so; d = sd;
}
// a path's identity (work item, sample) and its Philox position after camera_ray's draws
template <class S> RPT_DEV void stash_put_path(S& st, uint32_t lane, uint32_t p_local, uint32_t pixel, uint32_t s, uint32_t s_end, const Rng& r) {
  st.v[6][lane] = __longlong_as_double((long long)r.hi);
  st.u[0][lane] = p_local; st.u[1][lane] = pixel; st.u[2][lane] = s; st.u[3][lane] = s_end;
  st.u[4][lane] = r.draw;
}
template <class S> RPT_DEV void stash_take_path(const S& st, uint32_t lane, const Frame& fr, uint32_t& p_local, uint32_t& pixel, uint32_t& s,
                             uint32_t& s_end, Rng& r) {
  p_local = st.u[0][lane]; pixel = st.u[1][lane]; s = st.u[2][lane]; s_end = st.u[3][lane];
  r = rng_make(fr.seed, pixel, fr.sample_base + s, 0);
  r.draw = st.u[4][lane];
  r.hi = (uint64_t)__double_as_longlong(st.v[6][lane]);
}
// a traced ray's hit in place of its origin: the point, the normal (or the environment's colour), the object (-1: escaped)
RPT_DEV void stash_put_hit(RayStashHit& st, uint32_t lane, const D3& pos, const D3& nrm, int obj) {
  stash_put_pos(st, lane, pos);
  st.v[7][lane] = nrm.x; st.v[8][lane] = nrm.y; st.v[9][lane] = nrm.z;
  st.u[5][lane] = (uint32_t)obj;
}
RPT_DEV void stash_take_hit(const RayStashHit& st, uint32_t lane, D3& pos, D3& d, D3& nrm, int& obj) {
  stash_take_ray(st, lane, pos, d);
  nrm = mk(st.v[7][lane], st.v[8][lane], st.v[9][lane]);
  obj = (int)st.u[5][lane];
}
// RPT_HIT_POOL (kernels.h; the fused kernels): the wave's FIFO of pre-traced camera hits, [field][slot] — consecutive
// ranks of a push or a pop touch consecutive slots, as the lanes of the stash do.  An entry is all a lane needs to go on
// with the sample: v[0..2] the hit point, v[3..5] the incoming direction, v[6] the stream's cached half, v[7..9] the
// normal, or the environment's colour if the ray escaped; u: the object (-1: escaped), the work item's p_local, its
// pixel, the sample, the stream's draw counter.  Head and count are wave-uniform (hit_pool.h has the arithmetic)
struct HitPool {
  double v[10][RPT_POOL_CAP];
  uint32_t u[5][RPT_POOL_CAP];
};
static_assert(sizeof(HitPool) == RPT_PATHS_POOL_LDS, "kernels.h sizes the wave's LDS budget with it");
RPT_DEV void pool_put(HitPool& hp, uint32_t slot, const D3& pos, const D3& d, const D3& nrm, int obj, uint32_t p_local,
                      uint32_t pixel, uint32_t s, const Rng& r) {
  hp.v[0][slot] = pos.x; hp.v[1][slot] = pos.y; hp.v[2][slot] = pos.z;
  hp.v[3][slot] = d.x; hp.v[4][slot] = d.y; hp.v[5][slot] = d.z;
  hp.v[6][slot] = __longlong_as_double((long long)r.hi);
  hp.v[7][slot] = nrm.x; hp.v[8][slot] = nrm.y; hp.v[9][slot] = nrm.z;
  hp.u[0][slot] = (uint32_t)obj; hp.u[1][slot] = p_local; hp.u[2][slot] = pixel; hp.u[3][slot] = s; hp.u[4][slot] = r.draw;
}
RPT_DEV void pool_take(const HitPool& hp, uint32_t slot, const Frame& fr, D3& pos, D3& d, D3& nrm, int& obj, uint32_t& p_local,
                       uint32_t& s, Rng& r) {
  pos = mk(hp.v[0][slot], hp.v[1][slot], hp.v[2][slot]);
  d = mk(hp.v[3][slot], hp.v[4][slot], hp.v[5][slot]);
  nrm = mk(hp.v[7][slot], hp.v[8][slot], hp.v[9][slot]);
  obj = (int)hp.u[0][slot]; p_local = hp.u[1][slot]; s = hp.u[3][slot];
  r = rng_make(fr.seed, hp.u[2][slot], fr.sample_base + s, 0);
  r.draw = hp.u[4][slot];
  r.hi = (uint64_t)__double_as_longlong(hp.v[6][slot]);
}
#ifndef RPT_STASH_REFILL_MIN
#define RPT_STASH_REFILL_MIN 32 // RayStashHit: the wave also refills once this many lanes have an empty stash
#endif
// a path that ends at `depth` with radiance A (path_ended) and the next path's header slot behind its records
RPT_DEV void end_path(const PersistArgs& pa, const Frame& fr, double* __restrict__ rec, double (*fold_l)[64],
                      uint32_t (*fold_u)[64], uint32_t lane, uint32_t& fold_st, uint32_t ring, const D3& A, uint32_t depth,
                      uint32_t s, uint32_t p_local) {
  const uint32_t b = fold_st >> 16;
  path_ended(pa, fr, rec, fold_l, fold_u, lane, fold_st, A, depth, b, s, p_local);
  if (depth != 0u) fold_st = (fold_st & 0xffffu) | (next_header_slot(b, depth, ring) << 16);
}
// one step of the walker, for a lane that owes one (fold_st's low half): L = A_k + min(1/pdf * (f . L) * |wi.n|, 100)
// (renderer.rs:162-167), k = the deepest level not yet folded of the oldest path that ended
template <bool PARK>
RPT_DEV void walker_step(const PersistArgs& pa, const Frame& fr, const double* __restrict__ rec, double (*fold_l)[64],
                         uint32_t (*fold_u)[64], uint32_t lane, uint32_t& fold_st, uint32_t ring, uint32_t park_hd,
                         double probe_chk /* -DRPT_PROBE_NO_RING builds only */) {
  const uint32_t wk = fold_st & 0xffffu, cb = fold_st >> 16;
  const uint32_t wD = fold_u[0][lane], wb = fold_u[1][lane];
  uint32_t pos = wb + wk; // level wk - 1 of the walker's path
  if (pos >= ring) pos -= ring;
  const uint32_t nh = next_header_slot(wb, wD, ring); // header slot of the path behind it; == cb when no path waits
  const bool last = wk == 1u, more = last && nh != cb && (!PARK || nh != park_hd); // (a parked path's header is not written yet)
  double v[REC_FIELDS], hd[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#ifdef RPT_PROBE_NO_RING
  (void)pos; // (the headers of waiting paths — 40 B per path that waits, against 64 B per SEGMENT — stay real: the
             // walker's bookkeeping needs their depth)
#pragma unroll
  for (int q = 0; q < REC_FIELDS; q++) v[q] = probe_chk * (double)(q + 1);
#else
  {
    const double* r = rec + pos * REC_FIELDS;
#pragma unroll
    for (int q = 0; q < REC_FIELDS; q++) v[q] = r[q];
  }
#endif
  if (more) { // requested together with the record: one round trip
    const double* r = rec + nh * REC_FIELDS;
#pragma unroll
    for (int q = 0; q < 5; q++) hd[q] = r[q];
  }
  D3 L = mk(fold_l[0][lane], fold_l[1][lane], fold_l[2][lane]);
  D3 Ak = mk(v[0], v[1], v[2]);
  D3 f = mk(v[3], v[4], v[5]);
  D3 indirect = v[6] * cmul(f, L) * v[7];
  L = mk(Ak.x + fmin(indirect.x, FIREFLY_CLAMP), Ak.y + fmin(indirect.y, FIREFLY_CLAMP),
         Ak.z + fmin(indirect.z, FIREFLY_CLAMP));
  if (!last) {
    fold_l[0][lane] = L.x; fold_l[1][lane] = L.y; fold_l[2][lane] = L.z;
    fold_st -= 1u;
  } else { // level 0 folded: L is the sample (summed by rpt_sum_samples)
    double* lb = pa.lbuf + (uint64_t)fold_u[2][lane] * 3 * fr.npix + fold_u[3][lane];
    lb[0] = L.x;
    lb[fr.npix] = L.y;
    lb[2 * (uint64_t)fr.npix] = L.z;
    uint32_t nk = 0u;
    if (more) { // on to the oldest waiting path
      const uint64_t sp = (uint64_t)__double_as_longlong(hd[3]);
      nk = (uint32_t)__double_as_longlong(hd[4]);
      fold_l[0][lane] = hd[0]; fold_l[1][lane] = hd[1]; fold_l[2][lane] = hd[2];
      fold_u[0][lane] = nk; fold_u[1][lane] = nh; fold_u[2][lane] = (uint32_t)sp; fold_u[3][lane] = (uint32_t)(sp >> 32);
    }
    fold_st = (cb << 16) | nk;
  }
}
// the loop itself: kernels/paths_loop.inc, one text for rpt_paths (a camera's frame), rpt_paths_views (a piece of a batch of
// views, kernels/paths_views.inc) and rpt_paths_rays (a piece of the caller's rays or probes, kernels/paths_rays.inc), the last
// two in translation units of their own
#define RPT_PATHS_FORM RPT_PATHS_FORM_CAMERA
#include "paths_loop.inc"
#undef RPT_PATHS_FORM

#ifndef RPT_FORM_TU // (a form's translation unit compiles that form's kernels alone)
// color += trace_ray(...) over the launch's samples in sample order (renderer.rs:136-140); `first`
// starts the pixel's sum at zero, later launches of the same batch continue it
__global__ void __launch_bounds__(256) rpt_sum_samples(Frame fr, const double* __restrict__ lbuf, uint32_t spp, int first) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= fr.npix) return;
  D3 acc = first ? mk(0, 0, 0) : ld3(fr.accum + 3 * (uint64_t)p);
  const double* lb = lbuf + p;
  for (uint32_t s = 0; s < spp; s++) {
    D3 L = mk(lb[0], lb[fr.npix], lb[2 * (uint64_t)fr.npix]);
    acc = acc + L;
    lb += 3 * (uint64_t)fr.npix;
  }
  fr.accum[3 * (uint64_t)p] = acc.x;
  fr.accum[3 * (uint64_t)p + 1] = acc.y;
  fr.accum[3 * (uint64_t)p + 2] = acc.z;
}
#endif
