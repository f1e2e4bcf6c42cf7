// kernels/paths_loop.inc — the persistent path kernel's loop: ONE text, included once per form (RPT_PATHS_FORM, kernels.inc).
// RPT_PATHS_FORM_CAMERA (paths.inc): rpt_paths, whose work items are pixels of one camera's frame.
// RPT_PATHS_FORM_VIEWS (paths_views.inc): rpt_paths_views, whose work items are indices of a piece of a batch of views
// (rptgpu_render_views under RPT_FLAG_VIEWS_PERSISTENT, DESIGN.md §15.2): item p_local is index j = the piece's base + p_local
// of the call, fr.pixels[p_local] its pixel in its view — the stream id, as for a frame — and vr.view_of[p_local] its view,
// counted from the piece's first.  The camera ray is views_camera_ray's (rpt_raygen_views' ray, expression for expression)
// and the stream's key is the view's seed, taken at ray generation and again wherever a path comes back from the stash or
// the pool (views_rekey): the key is per lane.
// RPT_PATHS_FORM_RAYS (paths_rays.inc): rpt_paths_rays, whose work items are rays or light probes of a piece of the caller's
// (rptgpu_trace_rays / rptgpu_bake_probes under RPT_FLAG_RAYS_PERSISTENT, DESIGN.md §13.1): item p_local is ray or probe
// p_local of the piece, fr.pixels[p_local] its stream id, the key the Frame's seed as for a render; the ray is caller_ray's —
// read where the caller left it, or drawn as a probe's direction — behind all three hand-out forms.
// RPT_PATHS_FORM_VERTICES (paths_vertices.inc): rpt_paths_vertices, rpt_paths_rays over the caller's rays (never probes) with
// one argument more, the vertex sink (rptgpu_trace_vertices under RPT_FLAG_VERTICES_PERSISTENT, DESIGN.md §19.1): every value
// a vertex holds is written where the loop has it in a register — the hit behind the closest-hit query (vertex_hit), a
// record's values where they go to the ring (vertex_record), the last vertex's radiance and the path's length where the path
// ends (vertex_end).  The plain hand-out only: its translation units compile with the ray stash off.
// Everything else is the same text.  The forms differ by the preprocessor, not by a template parameter, and are compiled
// in different translation units (kernels.inc, RPT_VIEWS_TU / RPT_RAYS_TU / RPT_VERTICES_TU): rpt_paths' instantiations keep
// their names, their instructions and their place in their code object (DESIGN.md §15.2 has what sharing one cost).
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).
// the ray of sample smp of work item pl (stream id px) into (ro, rd), its stream behind the ray's draws into rr
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VIEWS
#define RPT_PATHS_RAY(pl, px, smp, ro, rd, rr) views_camera_ray(fr, vr, pl, px, smp, ro, rd, rr)
#elif RPT_PATHS_FORM == RPT_PATHS_FORM_RAYS || RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
#define RPT_PATHS_RAY(pl, px, smp, ro, rd, rr) caller_ray(fr, cr, pl, px, smp, ro, rd, rr)
#else
#define RPT_PATHS_RAY(pl, px, smp, ro, rd, rr) camera_ray(fr, cam, dim, px, smp, ro, rd, rr)
#endif
template <class LDS, bool PARK /* environment lookups parked per lane (pa.park_off) */,
          bool FUSE = false /* a hit's shadow ray and bounce ray in one query (FUSE below) */,
          bool CONSTS = false /* FUSE with a hit's scene constants in the wave's tables (SceneConsts, paths_consts.inc) */>
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VIEWS
__global__ void __launch_bounds__(64, RPT_PATHS_WAVES) rpt_paths_views(Scene sc, Frame fr, ViewRays vr, PersistArgs pa) {
#elif RPT_PATHS_FORM == RPT_PATHS_FORM_RAYS
__global__ void __launch_bounds__(64, RPT_PATHS_WAVES) rpt_paths_rays(Scene sc, Frame fr, CallerRays cr, PersistArgs pa) {
#elif RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
__global__ void __launch_bounds__(64, RPT_PATHS_WAVES) rpt_paths_vertices(Scene sc, Frame fr, CallerRays cr, VertexOut vo, PersistArgs pa) {
#else
__global__ void __launch_bounds__(64, RPT_PATHS_WAVES) rpt_paths(Scene sc, Frame fr, Camera cam, PersistArgs pa) {
#endif
  extern __shared__ __attribute__((aligned(16))) unsigned char flat_smem[]; // KdFlat only (dynamic size)
  __shared__ typename PathsLds<LDS>::type kd_store; // KdLds: the wave's traversal stack (15 KB); KdFlat: unused
  LDS* kd_ldsp = reinterpret_cast<LDS*>(&kd_store);
  constexpr bool FILTERED = std::is_same<LDS, KdFlatF>::value;
  constexpr bool IS_FLAT = std::is_same<LDS, KdFlat>::value || std::is_same<LDS, KdFlatG>::value || FILTERED;
  constexpr bool TRIS_IN_LDS = std::is_same<LDS, KdFlat>::value;
  FlatLds fl{};
  if constexpr (IS_FLAT) {
    const FlatLayout& lay = pa.flat;
    const uint32_t l = threadIdx.x;
    TriX* l_lrec = reinterpret_cast<TriX*>(flat_smem);
    Tri* l_tris = reinterpret_cast<Tri*>(flat_smem + lay.off_tris);
    uint32_t* l_refs = reinterpret_cast<uint32_t*>(flat_smem + lay.off_refs);
    Material* l_mat = reinterpret_cast<Material*>(flat_smem + lay.off_mat);
    uint32_t(*l_leaf)[4] = reinterpret_cast<uint32_t(*)[4]>(flat_smem + lay.off_leaf);
    const double* src = reinterpret_cast<const double*>(sc.lrec);
    double* dst = reinterpret_cast<double*>(l_lrec);
    for (uint32_t i = l; i < lay.n_refs * (uint32_t)(sizeof(TriX) / 8); i += 64) dst[i] = src[i];
    if constexpr (TRIS_IN_LDS) { // (KdFlatG: they stay in global memory — vertex normals of accepted hits, light sampling)
      src = reinterpret_cast<const double*>(sc.tris);
      dst = reinterpret_cast<double*>(l_tris);
      for (uint32_t i = l; i < lay.n_tris * (uint32_t)(sizeof(Tri) / 8); i += 64) dst[i] = src[i];
    }
    for (uint32_t i = l; i < lay.n_refs; i += 64) l_refs[i] = sc.refs[i];
    for (uint32_t i = l; i < (uint32_t)sc.num_objects * (uint32_t)(sizeof(Material) / 8); i += 64) {
      uint32_t ob = i / (uint32_t)(sizeof(Material) / 8), w = i - ob * (uint32_t)(sizeof(Material) / 8);
      reinterpret_cast<double*>(l_mat)[i] = reinterpret_cast<const double*>(sc.materials + sc.insts[ob].material)[w];
    }
    for (uint32_t ob = l; ob < (uint32_t)sc.num_objects; ob += 64) {
      const Inst& in = sc.insts[ob];
      uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
      if (in.kind == RPT_SHAPE_MESH) {
        const Tree& tr = sc.trees[in.tree];
        e0 = tr.ref_base; e1 = tr.prim_base; e2 = tr.root_first; e3 = tr.root_leaf - 1u;
      }
      l_leaf[ob][0] = e0; l_leaf[ob][1] = e1; l_leaf[ob][2] = e2; l_leaf[ob][3] = e3;
      if constexpr (FILTERED) {
        l_leaf[ob][3] = e3 | ((uint32_t)in.kind << 8) | (in.has_xf ? 1u << 16 : 0u);
        double* ob6 = reinterpret_cast<double*>(flat_smem + lay.off_obox) + 6u * ob;
        for (int k = 0; k < 6; k++) ob6[k] = in.bounds[k];
      }
    }
    if constexpr (CONSTS) {
      static_assert(FUSE, "the tables serve the fused form");
      scene_consts_fill(sc, sc.tris, l, flat_smem + lay.off_consts);
      fl.consts = flat_smem + lay.off_consts;
    }
    __syncthreads();
    sc.lrec = l_lrec;
    if constexpr (TRIS_IN_LDS) sc.tris = l_tris;
    sc.refs = l_refs;
    fl.lrec = l_lrec; fl.tris = sc.tris; fl.refs = l_refs; fl.obj_mat = l_mat; fl.obj_leaf = l_leaf;
    fl.qtab = reinterpret_cast<double*>(flat_smem + lay.off_qtab);
    fl.plane_vals = lay.plane_vals;
    fl.plane_cnt = lay.plane_cnt;
    if constexpr (FILTERED) {
      fl.obox = reinterpret_cast<const double*>(flat_smem + lay.off_obox);
      fl.obj_box = lay.obj_box; fl.obj_grid = lay.obj_grid; fl.obj_always = lay.obj_always;
    }
  }
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = __lane_id();
  // one lane's records are contiguous: [thread][depth][field], 64 B per depth.  Lanes of a wave sit at different
  // depths, so a [depth][field][thread] layout makes every store and every fold load a scattered 8-byte access
  double* __restrict__ rec = pa.rec + (uint64_t)tid * pa.ring * REC_FIELDS;
  // the walker's state (see the top of this file): L so far, its path's depth, header slot and sample — in LDS, so
  // that the registers of the main phases do not carry it; what stays in a register is fold_st = levels the walker
  // still owes (low half) | header slot of the running path (high half)
  __shared__ double fold_l[3][64];
  __shared__ uint32_t fold_u[4][64]; // depth D, header slot b, sample s, pixel p_local of the walker's path
  uint32_t fold_st = 0;
  const uint32_t ring = pa.ring;
  uint32_t p_local = 0, pixel = 0, s = 0, s_end = 0, depth = 0;
  bool done = false, in_path = false;
  D3 o = mk(0, 0, 0), d = mk(0, 0, 1);
  Rng rng = rng_make(fr.seed, 0, 0, 0);
  uint32_t n_ext = 0, n_sh = 0;
#ifdef RPT_PROBE_NO_RING
  double probe_chk = 0.0;
#else
  constexpr double probe_chk = 0.0; // (walker_step's unused argument)
#endif
#if RPT_PATHS_FORM == RPT_PATHS_FORM_CAMERA
  const double dim = (double)max(fr.width, fr.height);
#endif
  // rpt_paths<KdFlat>: the NEXT sample's camera ray waits in LDS.  Fetch and ray generation are work for the ~14 lanes of
  // 64 whose path just ended, but the wave ran through them in every iteration: 6 % of the kernel on C2.  Here every lane
  // keeps the ray of the sample that follows its running one in a per-lane stash (ray, Philox position, work item); a lane
  // whose path ended takes it, and the wave generates — for ALL lanes whose stash is empty, together — only when some
  // lane needs a ray and has none, about every third iteration.  The same rays from the same draws.
  //
  // PRETRACE (RPT_RAY_STASH=2, rpt_paths<KdFlat, false>): the stashed ray is also TRACED when it is generated, and a lane
  // whose ray escaped takes its stash right after the closest hit, so it shades the stashed hit in the same iteration
  // instead of idling through the shading phases (about 13 of the ~63 lanes that trace a ray on C2).  A lane that
  // starts an iteration without a running path skips the closest hit and takes its stash there too.  The pre-traces
  // run in the one closest-hit site: a lane that has a running path and a ray to pre-trace runs the query twice, the
  // stashed ray first (with its running ray parked in the stash's slots meanwhile), so nothing it holds in registers
  // lives across a query.  The wave refills when a lane must (as above) or when RPT_STASH_REFILL_MIN lanes could.
  constexpr bool STASH = RPT_RAY_STASH && std::is_same<LDS, KdFlat>::value;
  constexpr bool PRETRACE = STASH && RPT_RAY_STASH >= 2 && !PARK;
  //
  // FUSE (rpt_paths<KdFlat, false, true>: a flat scene with a plane table and one light, a non-ambient one — C2): a hit's
  // shadow ray and bounce ray leave from the same point, and the shadow ray's answer only decides whether the light term
  // is added (renderer.rs:185-201: illuminate draws, then sample_f draws, whatever the shadow ray meets).  So an
  // iteration takes its hit (the previous iteration's bounce result, or a stashed pre-traced one), shades it — illuminate,
  // the light term's bsdf, sample_f, the bounce's bsdf, in the reference's order — and then traces BOTH rays in one
  // two-ray query (flat_query2): it yields this hit's visibility and the next iteration's hit.  The record's f, 1/pdf and
  // |wi.n| go to the ring before the query and A after it, so no material, normal or wo lives across it.  The pending
  // pre-traces of a refill run in a pass of their own.  Per lane and iteration the ring sees the same events as without
  // FUSE (a path that escaped ends when its hit is taken, before the shading), so the bound at the top of this file holds.
  static_assert(!FUSE || PRETRACE, "the fused form is a form of the pre-traced kernel");
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
  static_assert(!STASH, "a stashed hit keeps its position, not its t: the vertices' form hands out work the plain way");
#endif
  //
  // POOL (RPT_HIT_POOL; the fused kernels): the pre-traced hits wait in a FIFO of the WAVE, not in the lane that made
  // them.  Nothing in the result depends on which lane runs a sample — the Philox stream is keyed by (seed, pixel,
  // sample), the radiance goes to lbuf[sample][channel][pixel], and the ring is private to whichever lane runs the
  // path — but with a per-lane stash a hit can only be used by its own lane, so the wave had to refill as soon as ONE
  // lane had neither a path nor a stash: pre-trace passes of 30 lanes of 64 on C2, at the price of 64.  Here a lane
  // keeps a generation CURSOR of its own (work item g_p_local, next sample g_s; ~0 = the item ran out), decoupled from
  // the path it runs (s, p_local, rng), and an entry of the pool is self-contained (HitPool).  At the top of an
  // iteration the wave refills (hit_pool.h rpt_pool_refill) once RPT_POOL_REFILL slots are free, or when the pool
  // cannot serve the lanes that need a hit: every lane with work, by ballot rank up to the free slots, fetches an item
  // if its own ran out (a lane still asks at most once past the end), generates its next sample's camera ray, traces it
  // and pushes the hit — one straight block, so nothing of a pending ray lives across the loop.  The lanes that need a
  // hit — no running path, or a bounce ray that escaped: such a path ends first, exactly as at the swap — are ranked
  // by a ballot and rank r takes entry r of the pool while there is one; a lane that finds none idles this iteration
  // (its escaped path ends in the shading phase, as before).  Per lane and iteration the ring sees what it saw: at most
  // one new record, and every header before the fold step; a lane may still end two paths in one iteration, the
  // escaped one and a depth-0 hit it pops, so the bound at the top of this file and its model
  // (tests/test_ray_stash_swap_model.py) stand.  The same rays from the same draws; only who runs them changes.
  constexpr bool POOL = FUSE && RPT_HIT_POOL != 0;
  using StashT = typename std::conditional<POOL, HitPool, typename std::conditional<PRETRACE, RayStashHit, RayStash>::type>::type;
  __shared__ typename std::conditional<STASH, StashT, int>::type stash_store;
  auto& stash = *reinterpret_cast<StashT*>(&stash_store);
  // POOL only (the other instantiations carry an empty struct): the lane's generation cursor, the pool's head and count
  struct PoolState { uint32_t g_p_local = 0, g_s = ~0u; uint32_t head = 0, cnt = 0; }; // (head, cnt: wave-uniform)
  struct NoPoolState {};
  [[maybe_unused]] typename std::conditional<POOL, PoolState, NoPoolState>::type ps;
  // the per-lane stash's state; the POOL instantiations use none of stash_valid, pend and near, nor pixel and s_end above
  // (the cursor and the entry carry what they held), and the compiler drops them there
  bool stash_valid = false, exhausted = false; // exhausted: the work counter ran out for this lane
  bool pend = false; // PRETRACE: the stashed ray is not traced yet
#if RPT_PRETRACE_CULL
  uint32_t near = ~0u; // FUSE: the screen rectangles that hold the pending ray's pixel (cull_near), from its generation to its pre-trace
#endif
  ItemPool pool{0u, 0u, 0u};
  // parked environment lookups (see the top of this file): park_hd = header slot of a parked path that holds ring slots
  constexpr bool park_on = PARK;
  ParkLds& park = *reinterpret_cast<ParkLds*>(flat_smem + (park_on ? pa.park_off : 0u));
  uint32_t pcnt = 0, park_hd = 0xffffffffu, park_recs = 0; // entries in the lane's queue; (top of this file); records they hold
  D3 nx_pos = mk(0, 0, 0), nx_nrm = mk(0, 0, 0); // FUSE: the hit of the running path's bounce ray (as h_pos, h_nrm, h_obj)
  int nx_obj = -1;
  PROF_INIT(); // -DRPT_PROF builds: wave / lane time per phase, printed by api_render.cpp under RPTGPU_PRINT_PHASES

  for (;;) {
    if constexpr (POOL) {
      // ---- refill the wave's pool of pre-traced hits (POOL above): fetch, camera ray, pre-trace, push
      const uint32_t n_need = (uint32_t)__popcll(__ballot(!in_path || nx_obj < 0)); // the lanes that pop in this iteration
      const uint64_t work_mask = __ballot(!exhausted);
      if (work_mask != 0ull && rpt_pool_refill(ps.cnt, n_need, RPT_POOL_CAP, RPT_POOL_REFILL)) { // (wave-uniform)
        // turns go by rank among the lanes with work: when a forced refill finds fewer free slots than such lanes, the low
        // lanes generate and the high lanes' cursors lag, so at the very end of a launch the high lanes hold the last
        // part-used items and the last refills are narrower than they could be — a tail of at most 64 items of `chunk`
        // samples per wave, not measured on its own (the A/B's whole-launch times include it)
        const bool turn = !exhausted && rpt_pool_rank(work_mask, lane) < rpt_pool_gen_limit(ps.cnt, RPT_POOL_CAP);
        const bool want_item = turn && ps.g_s == ~0u;
        uint32_t f_pixel = 0, f_s_end = 0; // (recomputed below: the cursor keeps neither)
        const bool got = fetch_item(pa, fr, lane, want_item, pool, ps.g_p_local, f_pixel, ps.g_s, f_s_end);
        if (want_item && !got) exhausted = true;
        PROF_PHASE(PF_P_FETCH);
        const bool gen = turn && !exhausted;
        const uint64_t gen_mask = __ballot(gen);
        if (gen) {
          const uint32_t g_pixel = fr.pixels[ps.g_p_local];
          D3 go, gd;
          Rng gr;
          RPT_PATHS_RAY(ps.g_p_local, g_pixel, ps.g_s, go, gd, gr);
          PROF_PHASE(PF_P_RAYGEN);
          double t = INF;
          D3 hn = mk(0, 0, 0);
#if RPT_PRETRACE_CULL
          const uint64_t skip = cull_skip_mask(pa.flat, cull_near(pa.flat, g_pixel, fr.width)); // (wave-uniform; 0 without the host's rectangles: every test runs)
          PROF_COUNT(PF_P_PRETRACE);
          const int ho = flat_query<false, true, CONSTS>(sc, &fl, go, gd, -INF, t, hn, skip);
#else
          const int ho = flat_query<false, false, CONSTS>(sc, &fl, go, gd, -INF, t, hn);
#endif
          n_ext++;
          if (ho < 0) hn = env_color(sc, gd); // renderer.rs:147
          pool_put(stash, rpt_pool_slot(ps.head, ps.cnt + rpt_pool_rank(gen_mask, lane), RPT_POOL_CAP), go + t * gd, gd, hn, ho,
                   ps.g_p_local, g_pixel, ps.g_s, gr);
          // the cursor's next sample; the item ends with its chunk, or with the launch's samples
          ps.g_s++;
          if (ps.g_s % pa.chunk == 0u || ps.g_s == pa.spp) ps.g_s = ~0u;
          PROF_PHASE(PF_P_HIT);
        }
        rpt_pool_after_push(ps.cnt, gen_mask);
        __syncthreads(); // (the block is this wave) the pushes, before other lanes pop them
      }
      done = !in_path && exhausted; // (this lane's part; the wave goes on while the pool holds a hit)
      if (ps.cnt == 0u && __ballot(!done || (fold_st & 0xffffu) != 0u) == 0) break; // (a lane without work still lets its walker finish)
    } else if constexpr (STASH) {
      // ---- generate ahead, when some lane must: it has no running path and no stashed ray
      bool refill = __ballot(!in_path && !stash_valid && !exhausted) != 0ull;
      if constexpr (PRETRACE) refill = refill || __popcll(__ballot(!stash_valid && !exhausted)) >= RPT_STASH_REFILL_MIN;
      if (refill) {
        const bool gen = !stash_valid && !exhausted;
        // the sample after the running one (a lane without a running path has already advanced s)
        uint32_t g_p_local = p_local, g_pixel = pixel, g_s = s + (in_path ? 1u : 0u), g_s_end = s_end;
        const bool want_item = gen && g_s >= g_s_end;
        const bool got = fetch_item(pa, fr, lane, want_item, pool, g_p_local, g_pixel, g_s, g_s_end);
        if (want_item && !got) exhausted = true;
        PROF_PHASE(PF_P_FETCH);
        if (gen && !exhausted) {
          D3 go, gd;
          Rng gr;
          RPT_PATHS_RAY(g_p_local, g_pixel, g_s, go, gd, gr);
#if RPT_PRETRACE_CULL
          if constexpr (FUSE) near = cull_near(pa.flat, g_pixel, fr.width);
#endif
          stash_put_ray(stash, lane, go, gd);
          stash_put_path(stash, lane, g_p_local, g_pixel, g_s, g_s_end, gr);
          stash_valid = true;
          pend = PRETRACE;
        }
        PROF_PHASE(PF_P_RAYGEN);
      }
      // ---- a lane whose path ended starts on its stashed ray (PRETRACE: after the closest hit)
      if (!PRETRACE && !in_path && stash_valid) {
        stash_take_ray(stash, lane, o, d);
        stash_take_path(stash, lane, fr, p_local, pixel, s, s_end, rng);
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VIEWS
        views_rekey(vr, p_local, rng);
#endif
        stash_valid = false;
        depth = 0;
        in_path = true;
      }
      done = !in_path && exhausted && !(PRETRACE && stash_valid); // (without PRETRACE, the take above used any stash left)
      if (__ballot(!done || (fold_st & 0xffffu) != 0u || pcnt != 0u) == 0) break; // (a lane without work still lets its walker finish)
    } else {
      // ---- work hand-out: persistent-thread fetch
      const bool need = !done && !in_path && s == s_end;
      if (!fetch_item(pa, fr, lane, need, pool, p_local, pixel, s, s_end) && need) done = true;
      if (__ballot(!done || (fold_st & 0xffffu) != 0u || pcnt != 0u) == 0) break; // (a lane without work still lets its walker finish)
      PROF_PHASE(PF_P_FETCH);
      // ---- ray generation (renderer.rs:132-139, camera.rs:64-81): camera_ray's body, word for word — a change to either goes
      // into both.  Calling it here costs rpt_paths<KdLds> 16 B of scratch and 6 spilled VGPRs (profiles/paths_split_resources.txt)
#if RPT_PATHS_FORM != RPT_PATHS_FORM_CAMERA
      if (!done && !in_path) { // (the views' or the caller's ray: a device function of its own, paths_views.inc / paths_rays.inc)
        RPT_PATHS_RAY(p_local, pixel, s, o, d, rng);
        depth = 0;
        in_path = true;
      }
#else
      if (!done && !in_path) {
        uint32_t y = pixel / fr.width, x = pixel - y * fr.width;
        double xn = ((double)(2 * x + 1) - (double)fr.width) / dim;
        double yn = ((double)(2 * (fr.height - y) - 1) - (double)fr.height) / dim;
        rng = rng_make(fr.seed, pixel, fr.sample_base + s, 0);
        double dx = gen_range(rng, -1.0 / dim, 1.0 / dim);
        double dy = gen_range(rng, -1.0 / dim, 1.0 / dim);
        double px = xn + dx, py = yn + dy;
        D3 direction = ld3(cam.direction), up = ld3(cam.up), right = ld3(cam.right);
        o = ld3(cam.eye);
        D3 new_dir = cam.d * direction + px * right + py * up;
        if (cam.aperture > 0.0) {
          D3 focal_point = o + normalize(new_dir) * cam.focal_distance;
          double a, b;
          unit_disc(rng, a, b);
          o = o + (a * right + b * up) * cam.aperture;
          new_dir = focal_point - o;
        }
        d = normalize(new_dir);
        depth = 0;
        in_path = true;
      }
#endif
    }

    PROF_PHASE(PF_P_RAYGEN);
    // ---- one path segment: trace_ray's body (renderer.rs:145-174)
    bool ending = false, esc = false; // the path ended in this iteration; with radiance A_end, or (esc) by a parked lookup
    D3 A_end = mk(0, 0, 0);
    // PRETRACE: the hit a lane shades — its point o + t d; its normal, or the environment's colour if the ray escaped
    D3 h_pos = mk(0, 0, 0), h_nrm = mk(0, 0, 0);
    int h_obj = -1;
    if constexpr (FUSE) {
      // ---- the running path's hit is its bounce ray's, found by the previous iteration's query; a refill's pending
      // pre-traces run here, in a pass of their own
      h_pos = nx_pos; h_nrm = nx_nrm; h_obj = nx_obj;
      nx_pos = mk(0, 0, 0); nx_nrm = mk(0, 0, 0); nx_obj = -1; // (so that no old value lives across the queries below)
      if constexpr (!POOL) {
        if (__ballot(pend) != 0ull) {
          if (pend) {
            D3 so, sd;
            stash_take_ray(stash, lane, so, sd);
            double t = INF;
            D3 hn = mk(0, 0, 0);
#if RPT_PRETRACE_CULL
            const uint64_t skip = cull_skip_mask(pa.flat, near); // (wave-uniform; 0 without the host's rectangles: every test runs)
            PROF_COUNT(PF_P_PRETRACE);
            const int ho = flat_query<false, true, CONSTS>(sc, &fl, so, sd, -INF, t, hn, skip);
#else
            const int ho = flat_query<false, false, CONSTS>(sc, &fl, so, sd, -INF, t, hn);
#endif
            n_ext++;
            if (ho < 0) hn = env_color(sc, sd); // renderer.rs:147
            stash_put_hit(stash, lane, so + t * sd, hn, ho);
            pend = false;
          }
        }
      }
    } else if constexpr (PRETRACE) {
      // ---- closest hits: pass 0 (only when some lane has both) the pending pre-traces, pass 1 the running paths and
      // the pre-traces of lanes without one.  Every pass resets what the query writes, so no lane's result of pass 0
      // lives in registers across the query of pass 1.
#pragma unroll 1
      for (uint32_t pass = __ballot(pend && in_path) != 0ull ? 0u : 1u; pass < 2u; pass++) {
        const bool pre = pend, run = pend || (pass == 1u && in_path);
        if (pre) stash_swap_ray(stash, lane, o, d); // the stashed ray into the registers, the running one into its slots meanwhile
        double t = INF;
        h_nrm = mk(0, 0, 0);
        h_obj = -1;
        if (run) {
          h_obj = flat_query<false>(sc, &fl, o, d, -INF, t, h_nrm);
          n_ext++;
          if (h_obj < 0) h_nrm = env_color(sc, d); // renderer.rs:147
        }
        h_pos = o + t * d;
        if (pre) { // the running ray back, the traced one's direction into its slots and its hit where its origin was
          D3 ro, rd;
          stash_take_ray(stash, lane, ro, rd);
          stash_put_dir(stash, lane, d);
          stash_put_hit(stash, lane, h_pos, h_nrm, h_obj);
          o = ro; d = rd;
          pend = false;
        }
      }
    }
    if constexpr (POOL) {
      PROF_PHASE(PF_P_HIT);
      // ---- the pop, in the place of the swap below: a path whose ray escaped ends here if the pool has a hit for its lane,
      // and that lane, like a lane without a running path, takes the hit — sample, Philox position and all — into
      // this iteration's shading
      const bool need = !in_path || h_obj < 0;
      const uint64_t need_mask = __ballot(need);
      if (need && rpt_pool_pop_ok(rpt_pool_rank(need_mask, lane), ps.cnt)) {
        if (in_path) end_path(pa, fr, rec, fold_l, fold_u, lane, fold_st, ring, h_nrm, depth, s, p_local);
        pool_take(stash, rpt_pool_slot(ps.head, rpt_pool_rank(need_mask, lane), RPT_POOL_CAP), fr, h_pos, d, h_nrm, h_obj, p_local, s, rng);
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VIEWS
        views_rekey(vr, p_local, rng);
#endif
        depth = 0;
        in_path = true;
      }
      rpt_pool_after_pop(ps.head, ps.cnt, need_mask, RPT_POOL_CAP);
      PROF_PHASE(PF_P_RAYGEN);
    } else if constexpr (PRETRACE) {
      PROF_PHASE(PF_P_HIT);
      // ---- the swap: a path whose ray escaped ends here (as in the miss branch below), and a lane without a running
      // path takes its stashed one — sample, Philox position and hit — into this iteration's shading
      if (in_path && h_obj < 0 && stash_valid) {
        end_path(pa, fr, rec, fold_l, fold_u, lane, fold_st, ring, h_nrm, depth, s, p_local);
        in_path = false;
      }
      if (!in_path && stash_valid) {
        stash_take_hit(stash, lane, h_pos, d, h_nrm, h_obj);
        stash_take_path(stash, lane, fr, p_local, pixel, s, s_end, rng);
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VIEWS
        views_rekey(vr, p_local, rng);
#endif
        stash_valid = false;
        depth = 0;
        in_path = true;
      }
      PROF_PHASE(PF_P_RAYGEN);
    }
    if constexpr (FUSE) {
      if (in_path && h_obj < 0) { // the ray escaped and the lane had no stash to take: A is the environment's colour
        PROF_PHASE(PF_P_ILLUM);
        ending = true;
        A_end = h_nrm;
      } else if (in_path) {
        const D3 world_pos = h_pos, nrm = h_nrm;
        const Material& mat = fl.obj_mat[h_obj];
        const D3 wo = -normalize_b(d);
        const D3 color = mat.emittance * ld3(mat.color);
        D3 wl, lt, wi;
        double dist;
        bool cont;
#if RPT_SHADE_SPLIT
        // SHADE_SPLIT (hit_draws, paths_shade.inc): a wave whose light is an untransformed mesh and whose lanes hit opaque
        // materials only takes every draw of its hits first and then shades them in one straight-line block: illuminate's tail and the light term's bsdf, sample_f's math and the bounce's bsdf, the two chains side
        // by side, selects in place of branches.  Each value keeps its operations in their order.  A point or
        // directional light, a transformed light or a glass surface in the wave takes the sequence below.
        CLight& lg = clight(sc, 0);
        CInst& li = cinst(sc, lg.inst);
        if (lg.kind == RPT_LIGHT_OBJECT && li.kind == RPT_SHAPE_MESH && !li.has_xf && __ballot(mat.transparent != 0) == 0ull) {
          CTree& tr = ctree(sc, li.tree);
          constexpr bool CM = CONSTS && SC_MAT, CL = CONSTS && SC_LIGHT;
          const MatConsts* mcs = CM ? mat_consts_of(&fl, h_obj) : nullptr;
          double fs;
          if constexpr (CM) {
            fs = mcs->fs;
          } else {
            const D3 mc = ld3(mat.color);
            const double f0 = pow2((mat.index - 1.0) / (mat.index + 1.0)); // sample_f's lobe probability (material.rs)
            const double mean = ((mc.x + mc.y) + mc.z) / 3.0;
            fs = (1.0 - mat.metallic) * f0 + mat.metallic * mean;
            fs = fs * (1.0 - 0.2) + 1.0 * 0.2;
          }
          cont = depth < fr.max_bounces;
          HitDraws dr;
          hit_draws<CM>(rng, cont, tr.num_prims, tr.sample_zone, fs, dr, mcs);
          n_sh++;
          PROF_PHASE(PF_P_DRAWS);
          D3 intensity;
          illuminate_mesh<CL>(lg, tr, sc.tris + tr.prim_base + dr.tri, world_pos, dr, intensity, wl, dist,
                              CL ? light_pdf_of(sc, &fl) : nullptr);
          double pdf;
          sample_f_opaque<CM>(mat, nrm, wo, fs, dr, wi, pdf, mcs);
          lt = mk(0, 0, 0) + cmul(bsdf_opaque<CM>(mat, nrm, wo, wl, mcs), intensity) * dot(wl, nrm);
          const D3 f = bsdf_opaque<CM>(mat, nrm, wo, wi, mcs);
          PROF_PHASE(PF_P_SHADE);
          if (cont) { // the record's f, 1/pdf and |wi.n| now, its A after the query
            rec_store_bsdf(rec + rec_slot(fold_st, depth, ring) * REC_FIELDS, f, 1.0 / pdf, fabs(dot(wi, nrm)));
          } else {
            wi = wl;
          }
          PROF_PHASE(PF_P_RECORD);
        } else
#endif
        {
        D3 intensity;
        illuminate(sc, clight(sc, 0), world_pos, rng, intensity, wl, dist); // sample_lights, renderer.rs:177-204
        n_sh++;
        PROF_PHASE(PF_P_ILLUM);
        // the light term, as it is added if the shadow ray gets through (bsdf is pure: evaluating it either way changes nothing)
        lt = mk(0, 0, 0) + cmul(bsdf(mat, nrm, wo, wl), intensity) * dot(wl, nrm);
        PROF_PHASE(PF_P_NEE);
        wi = wl;
        double pdf = 1.0;
        cont = depth < fr.max_bounces && sample_f(mat, nrm, wo, rng, wi, pdf);
        PROF_PHASE(PF_P_SAMPLE);
        if (cont) { // the record's f, 1/pdf and |wi.n| now, its A after the query
          const D3 f = bsdf(mat, nrm, wo, wi);
          PROF_PHASE(PF_P_BSDF);
          rec_store_bsdf(rec + rec_slot(fold_st, depth, ring) * REC_FIELDS, f, 1.0 / pdf, fabs(dot(wi, nrm)));
          PROF_PHASE(PF_P_RECORD);
        }
        }
        // ---- the fused query: this hit's visibility towards the light, and the closest hit of its bounce ray
        double rtb = cont ? INF : -INF, rts = INF;
        D3 rnb = mk(0, 0, 0);
        const double t_stop = fmin(dist, 1.7976931348623157e308); // as in visible()
        d = wi; // (a path that ends here needs d no more: the incoming direction does not live across the query)
        const int nobj = flat_query2<CONSTS>(sc, &fl, world_pos, d, wl, t_stop, rtb, rnb, rts);
        const bool vis = rts > t_stop; // (false for a NaN hit: see visible(), traversal.inc)
        PROF_PHASE(PF_P_FUSED);
        const D3 A = color + (vis ? lt : mk(0, 0, 0));
        if (cont) {
          double* r = rec + rec_slot(fold_st, depth, ring) * REC_FIELDS;
          r[0] = A.x; r[1] = A.y; r[2] = A.z;
          n_ext++;
          nx_pos = world_pos + rtb * d;
          nx_nrm = nobj < 0 ? env_color(sc, d) : rnb; // renderer.rs:147
          nx_obj = nobj;
          depth++;
        } else {
          ending = true;
          A_end = A;
        }
        PROF_PHASE(PF_P_RECORD);
      }
    } else if (in_path) {
      double t;
      D3 nrm;
      int obj;
      if constexpr (PRETRACE) {
        obj = h_obj;
        nrm = h_nrm;
      } else {
        if constexpr (IS_FLAT) {
          t = INF;
          nrm = mk(0, 0, 0);
          if constexpr (FILTERED) obj = flat_query_filtered<false>(sc, &fl, o, d, -INF, t, nrm);
          else obj = flat_query<false>(sc, &fl, o, d, -INF, t, nrm);
        } else {
          obj = closest_hit<LDS>(sc, o, d, t, nrm, kd_ldsp);
        }
        n_ext++;
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
        vertex_hit(vo, vertex_index(vo, p_local, s, depth), o, d, t, nrm, obj, rng.draw);
#endif
        PROF_PHASE(PF_P_HIT);
      }
      D3 A;
      bool cont = false;
      if (obj < 0) {
        if constexpr (park_on) { esc = true; A = mk(0, 0, 0); }
        else if constexpr (PRETRACE) A = nrm; // (the environment's colour, looked up at the closest hit)
        else {
#ifdef RPT_PROF_PARK
          PROF_COUNT(PF_IK_CHILD);
#endif
          A = env_color(sc, d); // renderer.rs:147
        }
        PROF_PHASE(PF_P_ILLUM); // (-DRPT_PROF builds: the lookup's time shows in the "illuminate" row — in a scene without lights, e.g. glass.rs, it is that row)
      } else {
        D3 world_pos;
        if constexpr (PRETRACE) world_pos = h_pos;
        else world_pos = o + t * d;
        const Material* matp;
        if constexpr (IS_FLAT) matp = fl.obj_mat + obj;
        else matp = sc.materials + sc.insts[obj].material;
        const Material& mat = *matp;
        D3 wo = -normalize(d);
        D3 color = mat.emittance * ld3(mat.color);
        D3 lights = mk(0, 0, 0); // sample_lights, renderer.rs:177-204
        for (int l = 0; l < sc.num_lights; l++) {
          CLight& light = clight(sc, l);
          if (light.kind == RPT_LIGHT_AMBIENT) {
            lights = lights + cmul(ld3(light.color), ld3(mat.color));
          } else {
            D3 intensity, wi;
            double dist;
            illuminate(sc, light, world_pos, rng, intensity, wi, dist);
            n_sh++;
            PROF_PHASE(PF_P_ILLUM);
            bool vis;
            if constexpr (IS_FLAT) {
              double srt = INF;
              D3 srn = mk(0, 0, 0);
              const double t_stop = fmin(dist, 1.7976931348623157e308); // as in visible()
              if constexpr (FILTERED) flat_query_filtered<true>(sc, &fl, world_pos, wi, t_stop, srt, srn);
              else flat_query<true>(sc, &fl, world_pos, wi, t_stop, srt, srn);
              vis = srt > t_stop; // (false for a NaN hit: see visible(), traversal.inc)
            } else {
              vis = visible<LDS>(sc, world_pos, wi, dist, kd_ldsp);
            }
            PROF_PHASE(PF_P_VIS);
            if (vis) {
              D3 f = bsdf(mat, nrm, wo, wi);
              lights = lights + cmul(f, intensity) * dot(wi, nrm);
            }
            PROF_PHASE(PF_P_NEE);
          }
        }
        A = color + lights;
        if (depth < fr.max_bounces) {
          D3 wi;
          double pdf;
          bool some = sample_f(mat, nrm, wo, rng, wi, pdf);
          PROF_PHASE(PF_P_SAMPLE);
          if (some) {
            D3 f = bsdf(mat, nrm, wo, wi);
            PROF_PHASE(PF_P_BSDF);
            const double inv_pdf = 1.0 / pdf, abscos = fabs(dot(wi, nrm));
#ifdef RPT_PROBE_NO_RING
            // DIAGNOSTIC build (wrong images): what does the record ring's trip through global memory cost?  Every value a
            // record holds stays live — it feeds a per-lane checksum that the walker's arithmetic consumes and that ends in
            // lbuf — but no RECORD is stored to or loaded from the ring (64 B per path segment each way; the 40-byte headers of
            // paths that wait for the walker stay, the bookkeeping needs them).
            probe_chk += ((A.x + A.y) + A.z) + ((f.x + f.y) + f.z) + inv_pdf + abscos;
#else
            {
              double* r = rec + rec_slot(fold_st, depth, ring) * REC_FIELDS;
              r[0] = A.x; r[1] = A.y; r[2] = A.z;
              rec_store_bsdf(r, f, inv_pdf, abscos);
            }
#endif
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
            vertex_record(vo, vertex_index(vo, p_local, s, depth), A, f, inv_pdf, abscos);
#endif
            o = world_pos;
            d = wi;
            depth++;
            cont = true;
            PROF_PHASE(PF_P_RECORD);
          }
        }
      }
      PROF_PHASE(PF_P_RECORD);
      ending = !cont;
      A_end = A;
    }
    if constexpr (park_on) {
      if (esc && pcnt < (uint32_t)RPT_PARK_K) { // the lookup waits in the lane's queue, and the lane goes on to its next ray
        park_push(park, lane, pcnt, park_hd, park_recs, fold_st, ring, d, depth, s, p_local);
        esc = false; ending = false;
        s++;
        in_path = false;
      }
      // drain? (top of this file)
      bool back = pcnt != 0u && (done || ending);
      if (park_recs != 0u && in_path && !ending) back = park_recs + depth >= fr.max_bounces;
      const uint64_t c0 = __ballot((pcnt & 1u) != 0u), c1 = __ballot((pcnt & 2u) != 0u), c2 = __ballot((pcnt & 4u) != 0u);
      const uint32_t n_req = (uint32_t)__popcll(c0) + 2u * (uint32_t)__popcll(c1) + 4u * (uint32_t)__popcll(c2);
      if (__ballot(back) != 0ull || n_req >= (uint32_t)RPT_PARK_FLUSH) {
        const uint64_t below = (1ull << lane) - 1ull;
        const uint32_t first = (uint32_t)__popcll(c0 & below) + 2u * (uint32_t)__popcll(c1 & below) + 4u * (uint32_t)__popcll(c2 & below);
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)RPT_PARK_K; k++)
          if (k < pcnt) park.list[first + k] = (uint8_t)(lane | (k << 6));
        __syncthreads(); // (the block is this wave)
        for (uint32_t g0 = 0; g0 < n_req; g0 += 64u) {
          const uint32_t g = g0 + lane;
          if (g < n_req) {
#ifdef RPT_PROF_PARK
            PROF_COUNT(PF_IK_CHILD); // (diagnostic builds: lookup rounds and their lanes in the "in-kernel child test" row)
#endif
            const uint32_t e = park.list[g], owner = e & 63u, k = e >> 6;
            const D3 pd = mk(park.d[k][0][owner], park.d[k][1][owner], park.d[k][2][owner]);
            const D3 col = env_color(sc, pd); // renderer.rs:147
            park.d[k][0][owner] = col.x; park.d[k][1][owner] = col.y; park.d[k][2][owner] = col.z;
          }
        }
        __syncthreads();
        for (uint32_t k = 0; __ballot(k < pcnt) != 0ull; k++) { // the older path first
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
          if (k < pcnt)
            vertex_end(vo, park.u[k][3][lane], park.u[k][2][lane], park.u[k][0][lane],
                       mk(park.d[k][0][lane], park.d[k][1][lane], park.d[k][2][lane]));
#endif
          if (k < pcnt)
            path_ended(pa, fr, rec, fold_l, fold_u, lane, fold_st, mk(park.d[k][0][lane], park.d[k][1][lane], park.d[k][2][lane]),
                       park.u[k][0][lane], park.u[k][1][lane], park.u[k][2][lane], park.u[k][3][lane]);
        }
        pcnt = 0u; park_hd = 0xffffffffu; park_recs = 0u;
      }
      PROF_PHASE(PF_P_ILLUM);
      if (esc) { // (the lane's queue was full: it is empty now)
        park_push(park, lane, pcnt, park_hd, park_recs, fold_st, ring, d, depth, s, p_local);
        ending = false;
        s++;
        in_path = false;
      }
    }
    if (ending) { // the path ended at this depth with radiance A_end
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
      vertex_end(vo, p_local, s, depth, A_end);
#endif
      end_path(pa, fr, rec, fold_l, fold_u, lane, fold_st, ring, A_end, depth, s, p_local);
      s++;
      in_path = false;
    }
    PROF_PHASE(PF_P_RECORD);
    if ((fold_st & 0xffffu) != 0u) { // ---- one step of the walker for every lane that owes one (walker_step)
      PROF_COUNT(PF_P_FOLDIT);
      walker_step<PARK>(pa, fr, rec, fold_l, fold_u, lane, fold_st, ring, park_hd, probe_chk);
    }
    PROF_PHASE(PF_P_FOLD);
  }
  PROF_FLUSH();
  // ray accounting: one atomic per wave and counter
  for (int off = 32; off > 0; off >>= 1) {
    n_ext += __shfl_down(n_ext, off);
    n_sh += __shfl_down(n_sh, off);
  }
  if (lane == 0) {
    atomicAdd(pa.ray_counters, (unsigned long long)n_ext);
    atomicAdd(pa.ray_counters + 1, (unsigned long long)n_sh);
  }
}
#undef RPT_PATHS_RAY
