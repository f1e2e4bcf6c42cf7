// kernels/paths.inc — the persistent path kernel rpt_paths<KdLds|KdFlat>, flat_query, rpt_sum_samples.
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
// What a flat scene keeps in LDS instead of a traversal stack: its intersection records, triangles, leaf
// entries and per-object materials (every tree has fewer than 16 primitives), read with ds_read at LDS
// latency instead of through L1/L2, which the clamp records keep flushing — and, in what is left of the
// wave's 20 KB stays free (rounds 2-3 kept clamp records there; the fold walker's records live in global memory).
// (the layout of the wave's dynamic LDS, FlatLayout, is computed on the host: kernels.h, api_scene.cpp)
struct FlatLds {
  const TriX* lrec;
  const Tri* tris;
  const uint32_t* refs;
  const Material* obj_mat;           // the material OF object i (not the scene's material table)
  const uint32_t (*obj_leaf)[4];     // MESH objects: ref_base, prim_base, first entry, entry count of the one leaf
  double* qtab;                      // [slots][64 lanes]: this ray's quotients (value - o) / d of the shared planes, the x
                                     // planes' first, then y, then z (as many slots as there are distinct planes)
  const double* plane_vals;          // [3][4] distinct plane coordinates (device memory, read through s_load)
  uint32_t plane_cnt;                // 4 bits per axis; 0 = no table
  // object filter (rpt_paths<KdFlatF>, flat_query_filtered): there obj_leaf[i][3] also carries kind << 8 | has_xf << 16
  const double* obox;                // [objects][6]: bounds of MESH objects
  const LeafBox* obj_box;            // [objects] conservative boxes (device memory, read through s_load)
  const double* obj_grid;            // qlo[3], qscale[3], bounds[6] (device memory, s_load)
  uint64_t obj_always;
  // rpt_paths<KdFlat, false, true, true>: what a hit derives from the scene alone, once per wave (SceneConsts below)
  // — ONE address for the three tables (each one more that the loop keeps costs the kernel scalar registers it has to
  // spill): [objects] MatConsts from it on, behind them [triangles of the light's mesh] doubles, and in front of it, back
  // to front, [cubes in two-cube blocks, in object order][face][3] doubles (mat_consts_of, light_pdf_of, cube_nrm_of)
  const unsigned char* consts;
};
// ------------------------------------------------------------------ a hit's scene constants, once per wave
// SceneConsts (rpt_paths<KdFlat, false, true, true>, RPT_SCENE_CONSTS): the straight-line code of a hit computes values
// that depend on the material, the light's triangle or the cube alone — fixed for the whole launch.  Every wave computes
// them once, in its prologue (scene_consts_fill), with the loop's own expressions on the same operands in the same order,
// so the bits are the loop's; it reads the scene's records from device memory as they stand at the launch, so a live
// update needs nothing more.  Lane `ob` does object `ob`, lane `k` triangle `k` of the light's mesh, lanes 0-11 the
// faces of a two-cube block.  (FlatLds::consts says where the three tables lie.)
// The three groups can be built one by one (A/B builds): RPT_SCENE_CONSTS is a mask, 1 = the materials' constants,
// 2 = the light's pdfs, 4 = the cubes' normals (kernels.h says which ones the default builds, and why).
constexpr bool SC_MAT = (RPT_SCENE_CONSTS & 1) != 0, SC_LIGHT = (RPT_SCENE_CONSTS & 2) != 0, SC_CUBE = (RPT_SCENE_CONSTS & 4) != 0;
struct MatConsts {   // of the material of an object (bsdf_opaque, sample_f_opaque and the kernel's lobe probability)
  double m2, m2pi;   // roughness^2; m2 * PI (bsdf's Beckmann denominator m2 * PI * nh2 * nh2; beckmann_pdf's PI * m2)
  double f0s;        // pow2((index - 1) / (index + 1))
  double f0[3];      // lerp((f0s, f0s, f0s), color, metallic)
  double omf0[3];    // (1, 1, 1) - f0
  double fs;         // sample_f's lobe probability
  uint64_t p_int;    // gen_bool(fs)'s threshold (unused when fs == 1.0: gen_bool then takes no draw)
};
static_assert(sizeof(MatConsts) == RPT_MAT_CONSTS_BYTES, "kernels.h sizes the wave's LDS budget with it");
// a face of the unit cube as cube_candidate names its normals: 2 * axis + (1 if the normal points down the axis)
RPT_DEV D3 cube_face_normal(uint32_t face) {
  const double s = (face & 1u) ? -1.0 : 1.0;
  const uint32_t axis = face >> 1;
  return mk(axis == 0u ? s : 0.0, axis == 1u ? s : 0.0, axis == 2u ? s : 0.0);
}
RPT_DEV const MatConsts* mat_consts_of(const FlatLds* fl, int obj) { return reinterpret_cast<const MatConsts*>(fl->consts) + obj; }
RPT_DEV const double* light_pdf_of(const Scene& sc, const FlatLds* fl) {
  return reinterpret_cast<const double*>(fl->consts + (SC_MAT ? (uint32_t)sc.num_objects : 0u) * (uint32_t)sizeof(MatConsts));
}
RPT_DEV D3 cube_nrm_of(const FlatLds* fl, uint32_t slot, uint32_t face) { // cube `slot` sits slot + 1 cubes in front of fl->consts
  return ld3(reinterpret_cast<const double*>(fl->consts) - (slot + 1u) * 18u + face * 3u);
}
RPT_DEV bool xf_cube_pair(const Scene& sc, int i) { // flat_query's condition for its two-cube block
  return cinst(sc, i).kind == RPT_SHAPE_CUBE && cinst(sc, i).has_xf && i + 1 < sc.num_objects &&
         cinst(sc, i + 1).kind == RPT_SHAPE_CUBE && cinst(sc, i + 1).has_xf;
}
// the prologue's part (all 64 lanes, before the barrier; `tris` = the scene's triangles in device memory)
RPT_DEV void scene_consts_fill(const Scene& sc, const Tri* __restrict__ tris, uint32_t l, unsigned char* consts) {
  MatConsts* mc = reinterpret_cast<MatConsts*>(consts);
  double* light_pdf = reinterpret_cast<double*>(consts + (SC_MAT ? (uint32_t)sc.num_objects : 0u) * (uint32_t)sizeof(MatConsts));
  for (uint32_t ob = l; SC_MAT && ob < (uint32_t)sc.num_objects; ob += 64) {
    const Material& mat = sc.materials[sc.insts[ob].material];
    MatConsts c;
    const D3 color = ld3(mat.color);
    const D3 one = mk(1, 1, 1);
    c.m2 = mat.roughness * mat.roughness;
    c.m2pi = c.m2 * PI;
    c.f0s = pow2((mat.index - 1.0) / (mat.index + 1.0));
    const D3 f0 = lerp(mk(c.f0s, c.f0s, c.f0s), color, mat.metallic);
    const D3 omf0 = one - f0;
    c.f0[0] = f0.x; c.f0[1] = f0.y; c.f0[2] = f0.z;
    c.omf0[0] = omf0.x; c.omf0[1] = omf0.y; c.omf0[2] = omf0.z;
    const double mean = ((color.x + color.y) + color.z) / 3.0;
    double fs = (1.0 - mat.metallic) * c.f0s + mat.metallic * mean;
    fs = fs * (1.0 - 0.2) + 1.0 * 0.2;
    c.fs = fs;
    c.p_int = (uint64_t)(fs * 18446744073709551616.0);
    mc[ob] = c;
  }
  CLight& lg = clight(sc, 0);
  CInst& li = cinst(sc, lg.inst);
  if (SC_LIGHT && lg.kind == RPT_LIGHT_OBJECT && li.kind == RPT_SHAPE_MESH && !li.has_xf) { // illuminate_mesh's light
    CTree& tr = ctree(sc, li.tree);
    for (uint32_t k = l; k < tr.num_prims; k += 64) {
      const Tri* tp = tris + tr.prim_base + k;
      const D3 v1 = ld3(tp->v), v2 = ld3(tp->v + 3), v3 = ld3(tp->v + 6);
      const double area = 0.5 * length(cross(v2 - v1, v3 - v1));
      double p = 1.0 / area;
      p = p / (double)tr.num_prims;
      light_pdf[k] = p;
    }
  }
  uint32_t slot = 0;
  for (int i = 0; SC_CUBE && i < sc.num_objects;) { // the two-cube blocks in the order flat_query meets them
    if (!xf_cube_pair(sc, i)) { i++; continue; }
    if (l < 12u) {
      const uint32_t c = l / 6u, face = l - 6u * c;
      const D3 w = normalize(mat3_mul(sc.insts[i + (int)c].nrm, cube_face_normal(face))); // Transformed::intersect shape.rs:131-132
      double* q = reinterpret_cast<double*>(consts) - (slot + c + 1u) * 18u + face * 3u;
      q[0] = w.x; q[1] = w.y; q[2] = w.z;
    }
    slot += 2u;
    i += 2;
  }
}
// cube_candidate (shapes.inc) with the candidate's normal as its face (cube_face_normal): the same tests in the same order
RPT_DEV bool cube_candidate_face(D3 o, const RcpD& rdx, const RcpD& rdy, const RcpD& rdz, double t_min, double& time,
                                 uint32_t& face) {
  double x1, x2, y1, y2, z1, z2;
  uint32_t fx = 1u, fy = 3u, fz = 5u; // the ENTRY face along each axis: the normal -1 unless the interval was swapped
  div6(-0.5 - o.x, 0.5 - o.x, rdx, -0.5 - o.y, 0.5 - o.y, rdy, -0.5 - o.z, 0.5 - o.z, rdz, x1, x2, y1, y2, z1, z2);
  if (x1 > x2) { double t = x1; x1 = x2; x2 = t; fx = 0u; }
  if (y1 > y2) { double t = y1; y1 = y2; y2 = t; fy = 2u; }
  if (z1 > z2) { double t = z1; z1 = z2; z2 = t; fz = 4u; }
  double start, end;
  uint32_t sf, ef; // the exit face is the opposite one of the same axis
  if (x1 > y1 && x1 > z1) { start = x1; sf = fx; }
  else if (y1 > z1) { start = y1; sf = fy; }
  else { start = z1; sf = fz; }
  if (x2 < y2 && x2 < z2) { end = x2; ef = fx ^ 1u; }
  else if (y2 < z2) { end = y2; ef = fy ^ 1u; }
  else { end = z2; ef = fz ^ 1u; }
  if (start > end || end < t_min) return false;
  if (start < t_min) { time = end; face = ef; }
  else { time = start; face = sf; }
  return true;
}
// ------------------------------------------------------------------ flat scenes: batched quad tests
// Renderer::get_closest_hit / the visibility query for a scene whose trees are all single leaves.  The
// reference tests the objects one after the other; for a run of consecutive untransformed meshes (the
// five walls of C2) that means five sparsely populated leaf tests per ray, because a ray inside the box
// passes the (flat) slab of about one wall.  Here the run is handled in two steps with the same outcome:
//  1. the root slab test of every mesh of the run (uniform, all lanes busy): candidate bit k is set
//     unless  m_k = max(b_min, t_min) > min(b_max, rt)  (kdtree.rs:130-134) with rt as it is at the
//     start of the run;
//  2. each lane walks ITS candidates in object order and runs the leaf test on its own object (the
//     records sit in LDS, so per-lane addresses cost nothing).  rt can only have decreased since step
//     1, and for rt' <= rt the reference's condition  m_k > min(b_max, rt')  is  m_k > rt'  whenever
//     the step-1 test passed (then m_k <= b_max), so re-checking  m_k > rt  before the leaf test
//     reproduces the reference's decision exactly — every accept happens in the reference's order.
struct LaneTree {
  uint32_t ref_base, prim_base;
};
constexpr int FLAT_RUN = RPT_FLAT_RUN; // kernels.h: the host caps run lengths with the same constant

// slab tests of a run of N table users starting at object i (N known at compile time: branch-free, interleaved)
template <int N>
RPT_DEV uint32_t run_slabs(const Scene& sc, int i, const double* qt, double rt, double (&m)[FLAT_RUN]) {
  static_assert(N >= 1 && N <= FLAT_RUN, "run length");
  uint32_t cand = 0;
#pragma unroll
  for (int k = 0; k < FLAT_RUN; k++) m[k] = 0.0;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const uint32_t ix = cinst(sc, i + k).plane_idx;
    double fax = qt[((ix >> 0) & 15u) * 64u], fbx = qt[((ix >> 4) & 15u) * 64u];
    double fay = qt[((ix >> 8) & 15u) * 64u], fby = qt[((ix >> 12) & 15u) * 64u];
    double faz = qt[((ix >> 16) & 15u) * 64u], fbz = qt[((ix >> 20) & 15u) * 64u];
    double b_min = fmax(fmax(fmin(fax, fbx), fmin(fay, fby)), fmin(faz, fbz));
    double b_max = fmin(fmin(fmax(fax, fbx), fmax(fay, fby)), fmax(faz, fbz));
    double mm = fmax(b_min, EPSILON);
    if (!(mm > fmin(b_max, rt))) cand |= 1u << k;
    m[k] = mm;
  }
  return cand;
}

// ------------------------------------------------------------------ flat scenes with many objects: the object filter
// A room of 23 polygons, three cubes and three spheres: the reference runs 29 object tests per ray (renderer.rs:211-220),
// 23 of them a root slab test of six divisions, and a ray passes the box of three or four.  Here every ray is first
// tested against a conservative 16-bit box of every object, in f32, in one uniform loop (host_scene.cpp
// fill_object_boxes says why an object whose box the ray misses inside [t_min, record.time] cannot be hit: its test is
// skipped with nothing changed); then each lane walks ITS candidates in object order and runs the object's own, exact
// test — the slab test and the leaf of a mesh (kdtree.rs:129-136, 162-171), Transformed<Sphere | Cube | Plane>
// (shape.rs:128-137) — with the record as it stands, exactly like the reference.  The window is the one at the start
// of the query (record.time only shrinks: a later, narrower window would reject more, never less).
struct ObjGrid {
  double qlo[3], qscale[3];
};
template <bool SHADOW>
RPT_DEV int flat_query_filtered(const Scene& sc, const FlatLds* fl, D3 o, D3 d, double t_stop, double& rt, D3& rn) {
  int obj = -1;
  const int n = sc.num_objects;
  RcpD rwx = rcp_make(d.x), rwy = rcp_make(d.y), rwz = rcp_make(d.z);
  uint64_t cand = n >= 64 ? ~0ull : (1ull << n) - 1ull;
  {
    const double RPT_C* g = (const double RPT_C*)fl->obj_grid;
    ObjGrid gr;
    for (int k = 0; k < 3; k++) { gr.qlo[k] = g[k]; gr.qscale[k] = g[3 + k]; }
    double fax, fbx, fay, fby, faz, fbz; // where the ray enters the bounds of the grid: the filter counts from there
    div6(g[6] - o.x, g[9] - o.x, rwx, g[7] - o.y, g[10] - o.y, rwy, g[8] - o.z, g[11] - o.z, rwz, fax, fbx, fay, fby, faz, fbz);
    const double b_min = fmax(fmax(fmin(fax, fbx), fmin(fay, fby)), fmin(faz, fbz));
    const BoxRay br = boxray_make<true>(gr, o, d, fmax(b_min, 0.0));
    if (br.on) {
      float wl, wh;
      box_window(br, EPSILON, SHADOW ? fmin(rt, t_stop) : rt, wl, wh);
      const LeafBox RPT_C* bx = (const LeafBox RPT_C*)fl->obj_box;
      uint64_t pass = fl->obj_always;
      for (int k = 0; k < n; k++) {
        LeafBox lb;
        lb.w[0] = bx[k].w[0]; lb.w[1] = bx[k].w[1]; lb.w[2] = bx[k].w[2]; lb.w[3] = 0u;
        pass |= (leaf_box_pass(lb, br, wl, wh) ? 1ull : 0ull) << k;
      }
      cand &= pass;
    }
  }
  while (__ballot(cand != 0ull) != 0ull) {
    if (cand != 0ull) {
      PROF_COUNT(PF_P_CAND);
      const int k = __ffsll((long long)cand) - 1;
      cand &= cand - 1ull;
      const uint32_t* e = fl->obj_leaf[k];
      const uint32_t kind = (e[3] >> 8) & 0xffu;
      const bool has_xf = ((e[3] >> 16) & 1u) != 0u;
      const Inst* __restrict__ in = sc.insts + k;
      bool h = false;
      if (kind == RPT_SHAPE_MESH) { // KdTree::intersect of a single-leaf tree: root slab, then the leaf
        D3 lo = o, ld = d;
        RcpD rx = rwx, ry = rwy, rz = rwz;
        if (has_xf) {
          lo = mat4_mul(in->inv, o, 1.0);
          ld = mat4_mul(in->inv, d, 0.0);
          rx = rcp_make(ld.x); ry = rcp_make(ld.y); rz = rcp_make(ld.z);
        }
        const double* bb = fl->obox + 6 * k;
        double fax, fbx, fay, fby, faz, fbz;
        div6(bb[0] - lo.x, bb[3] - lo.x, rx, bb[1] - lo.y, bb[4] - lo.y, ry, bb[2] - lo.z, bb[5] - lo.z, rz, fax, fbx, fay, fby, faz, fbz);
        const double b_min = fmax(fmax(fmin(fax, fbx), fmin(fay, fby)), fmin(faz, fbz));
        const double b_max = fmin(fmin(fmax(fax, fbx), fmax(fay, fby)), fmax(faz, fbz));
        if (!(fmax(b_min, EPSILON) > fmin(b_max, rt))) { // kdtree.rs:130-134
          LaneTree lt{e[0], e[1]};
          KdNode nd;
          nd.split = 0.0; nd.a = e[2]; nd.ib = ((e[3] & 0xffu) << 2) | 3u;
          D3 nn = rn;
          h = kd_leaf<true, SHADOW>(sc, lt, sc.refs + lt.ref_base, nd, lo, ld, EPSILON, t_stop, rt, nn);
          if (h) rn = (!SHADOW && has_xf) ? normalize(mat3_mul(in->nrm, nn)) : nn; // shape.rs:131-132
        }
      } else if (kind == RPT_SHAPE_PLANE) {
        D3 lo = o, ld = d;
        if (has_xf) {
          lo = mat4_mul(in->inv, o, 1.0);
          ld = mat4_mul(in->inv, d, 0.0);
        }
        h = isect_plane(in->plane, lo, ld, EPSILON, rt, rn, !SHADOW);
        if (!SHADOW && h && has_xf) rn = normalize(mat3_mul(in->nrm, rn));
      } else { // sphere, cube
        const ChildM c = ld_child(in);
        h = isect_child(c, in, o, d, EPSILON, rt, rn, !SHADOW);
      }
      if (h) obj = k;
      if (SHADOW && rt <= t_stop) cand = 0ull;
    }
  }
  return obj;
}

#if RPT_PRETRACE_CULL
// ------------------------------------------------------------------ the pre-trace pass: objects no pending ray can hit
// The camera rays a refill pre-traces are the one coherent set of rays in rpt_paths<KdFlat, false, true>: the lanes of a
// wave hold neighbouring pixels of a tile, and most waves' rays pass nowhere near the two cubes of C2 — yet the cube
// block of flat_query is straight-line code that every pass runs for all of its lanes.  Under a pinhole camera the host
// hands the kernel, per render, the screen rectangle of each object outside the plane table (host_scene.cpp
// pinhole_screen_rect says why a camera ray of a pixel outside the rectangle cannot be accepted by the object's exact
// test).  A lane notes at ray generation which rectangles hold its pixel (cull_near: two packed 16-bit operations; bit j =
// rectangle j), and the pre-trace pass skips, for the whole wave, an object whose rectangle holds no pending lane's
// pixel (cull_skip_mask, wave-uniform: bit k = object k).  flat_query<false, true> leaves such an object's test out,
// which changes nothing: none of the wave's tests of it would have accepted.  A lane inside a test that runs is not
// masked: the exact test decides, as before.  (The object filter's f32 boxes, tested per pending ray in the pass, were
// built first: bit-equal, two thirds of the passes skipped the cubes, and 0.9 % slower — profiles/pretrace_cull_ab.txt.)
typedef unsigned short US2 __attribute__((ext_vector_type(2)));
RPT_DEV uint32_t cull_near(const FlatLayout& lay, uint32_t pix, uint32_t width) {
  const uint32_t y = pix / width, x = pix - y * width; // (camera_ray's own quotient)
  const US2 xy = {(unsigned short)x, (unsigned short)y};
  uint32_t near = 0u;
  for (uint32_t j = 0; j < lay.cull_n; j++) { // (wave-uniform) inside: (x - x0, y - y0) <= (x1 - x0, y1 - y0), both halves at once
    const US2 t = xy - __builtin_bit_cast(US2, lay.cull_lo[j]);
    const US2 m = __builtin_elementwise_min(t, __builtin_bit_cast(US2, lay.cull_ext[j]));
    near |= (__builtin_bit_cast(uint32_t, m) == __builtin_bit_cast(uint32_t, t) ? 1u : 0u) << j;
  }
  return near;
}
// among the lanes that call (the pending ones): the objects whose rectangle holds none of their pixels
RPT_DEV uint64_t cull_skip_mask(const FlatLayout& lay, uint32_t near) {
  uint64_t skip = 0ull;
  for (uint32_t j = 0; j < lay.cull_n; j++) // (wave-uniform)
    if (__ballot(((near >> j) & 1u) != 0u) == 0ull) skip |= 1ull << (lay.cull_obj[j] & 63u);
  return skip;
}
#endif

// CULL (the pre-trace pass of rpt_paths<KdFlat, false, true>, RPT_PRETRACE_CULL): bit k of the wave-uniform `skip` = no
// ray of the wave can be accepted by object k (cull_skip_mask), its test is left out
// CONSTS (rpt_paths<KdFlat, false, true, true>): the two-cube block takes an accepted cube's world normal from the
// wave's table (SceneConsts above)
template <bool SHADOW, bool CULL = false, bool CONSTS = false>
RPT_DEV int flat_query(const Scene& sc, const FlatLds* fl, D3 o, D3 d, double t_stop, double& rt, D3& rn, uint64_t skip = 0ull) {
  int obj = -1;
  uint32_t cslot = 0; // CONSTS: the next two-cube block's first cube in the table of normals (cube_nrm_of)
  RcpD rwx = rcp_make(d.x), rwy = rcp_make(d.y), rwz = rcp_make(d.z);
  const int n = sc.num_objects;
  const uint32_t lane = __lane_id();
  if (fl->plane_cnt) { // every distinct (plane - o) / d once per ray: the operands, hence the bits, of the per-object form
    const double RPT_C* pv = (const double RPT_C*)fl->plane_vals;
    const uint32_t nx = fl->plane_cnt & 15u, ny = (fl->plane_cnt >> 4) & 15u, nz = (fl->plane_cnt >> 8) & 15u;
    for (uint32_t j = 0; j < nx; j++) fl->qtab[j * 64u + lane] = (pv[j] - o.x) / d.x;
    for (uint32_t j = 0; j < ny; j++) fl->qtab[(nx + j) * 64u + lane] = (pv[4u + j] - o.y) / d.y;
    for (uint32_t j = 0; j < nz; j++) fl->qtab[(nx + ny + j) * 64u + lane] = (pv[8u + j] - o.z) / d.z;
  }
  int i = 0;
  while (i < n) {
    CInst& in = cinst(sc, i);
    if (in.kind == RPT_SHAPE_MESH && !in.has_xf) {
      uint32_t cand = 0;
      double m[FLAT_RUN];
      int len = 0;
      if (in.plane_use) {
        // run of `len` table users, known on the host: one straight-line block for all of them (a slot beyond the
        // run repeats its last object and is masked out), so the six slab evaluations interleave instead of
        // forming six dependent chains separated by branches
        len = (int)in.plane_use;
        const double* qt = fl->qtab + lane;
        switch (len) { // one straight-line block per run length: no slot is evaluated in vain
          case 1: cand = run_slabs<1>(sc, i, qt, rt, m); break;
          case 2: cand = run_slabs<2>(sc, i, qt, rt, m); break;
          case 3: cand = run_slabs<3>(sc, i, qt, rt, m); break;
          case 4: cand = run_slabs<4>(sc, i, qt, rt, m); break;
          case 5: cand = run_slabs<5>(sc, i, qt, rt, m); break;
          default: cand = run_slabs<FLAT_RUN>(sc, i, qt, rt, m); break;
        }
      } else { // no plane table (more than four distinct plane coordinates on some axis): discover the run here
#pragma unroll
      for (int k = 0; k < FLAT_RUN; k++) {
        m[k] = 0.0;
        if (len == k && i + k < n) { // the run is still growing
          CInst& q = cinst(sc, i + k);
          if (q.kind == RPT_SHAPE_MESH && !q.has_xf) {
            double fax, fbx, fay, fby, faz, fbz; // q.bounds == trees[q.tree].bounds (kdtree.rs:103)
            div6(q.bounds[0] - o.x, q.bounds[3] - o.x, rwx, q.bounds[1] - o.y, q.bounds[4] - o.y, rwy,
                 q.bounds[2] - o.z, q.bounds[5] - o.z, rwz, fax, fbx, fay, fby, faz, fbz);
            double b_min = fmax(fmax(fmin(fax, fbx), fmin(fay, fby)), fmin(faz, fbz));
            double b_max = fmin(fmin(fmax(fax, fbx), fmax(fay, fby)), fmax(faz, fbz));
            double mm = fmax(b_min, EPSILON);
            if (!(mm > fmin(b_max, rt))) cand |= 1u << k;
            m[k] = mm;
            len = k + 1;
          }
        }
      }
      }
      while (__ballot(cand != 0u) != 0ull) {
        if (cand != 0u) {
          PROF_COUNT(PF_P_CAND);
          int k = __ffs((int)cand) - 1;
          cand &= cand - 1u;
          double mk = m[0];
#pragma unroll
          for (int kk = 1; kk < FLAT_RUN; kk++) mk = k == kk ? m[kk] : mk;
          if (!(mk > rt)) {
            const uint32_t* e = fl->obj_leaf[i + k];
            LaneTree lt{e[0], e[1]};
            KdNode nd;
            nd.split = 0.0; nd.a = e[2]; nd.ib = (e[3] << 2) | 3u;
            bool h = kd_leaf<true, SHADOW>(sc, lt, sc.refs + lt.ref_base, nd, o, d, EPSILON, t_stop, rt, rn);
            if (h) obj = i + k;
            if (SHADOW && rt <= t_stop) cand = 0u;
          }
        }
      }
      if (SHADOW && rt <= t_stop) return obj;
      i += len;
    } else if (in.kind == RPT_SHAPE_CUBE && in.has_xf && i + 1 < n && cinst(sc, i + 1).kind == RPT_SHAPE_CUBE &&
               cinst(sc, i + 1).has_xf) {
      // two consecutive Transformed<Cube> (the boxes of C2): both candidates are evaluated in one block — a cube's
      // test depends on the record only through the final `time < record.time` (cube.rs:66) — and then accepted in
      // object order, so the second cube does not wait for the first one's whole chain
      if (CULL && ((skip >> i) & 3ull) == 3ull) { // (the block as it is when one of the two may be hit)
        PROF_COUNT(PF_P_PRECULL);
        i += 2;
        cslot += 2u;
        continue;
      }
      CInst& in2 = cinst(sc, i + 1);
      constexpr bool TAB = CONSTS && SC_CUBE && !SHADOW; // the accepted normal from the wave's table, by the candidate's face
      D3 lo1 = mat4_mul(in.inv, o, 1.0), ld1 = mat4_mul(in.inv, d, 0.0);
      D3 lo2 = mat4_mul(in2.inv, o, 1.0), ld2 = mat4_mul(in2.inv, d, 0.0);
      RcpD ax = rcp_make(ld1.x), ay = rcp_make(ld1.y), az = rcp_make(ld1.z);
      RcpD bx = rcp_make(ld2.x), by = rcp_make(ld2.y), bz = rcp_make(ld2.z);
      double t1 = 0.0, t2 = 0.0;
      D3 n1 = mk(0, 0, 0), n2 = mk(0, 0, 0);
      uint32_t f1 = 0u, f2 = 0u;
      bool c1 = TAB ? cube_candidate_face(lo1, ax, ay, az, EPSILON, t1, f1) : cube_candidate(lo1, ax, ay, az, EPSILON, t1, n1);
      bool c2 = TAB ? cube_candidate_face(lo2, bx, by, bz, EPSILON, t2, f2) : cube_candidate(lo2, bx, by, bz, EPSILON, t2, n2);
      if (c1 && t1 < rt) {
        rt = t1;
        if constexpr (TAB) rn = cube_nrm_of(fl, cslot, f1);
        else if (!SHADOW) rn = normalize(mat3_mul(in.nrm, n1)); // Transformed::intersect shape.rs:131-132
        obj = i;
      }
      if (SHADOW && rt <= t_stop) return obj;
      if (c2 && t2 < rt) {
        rt = t2;
        if constexpr (TAB) rn = cube_nrm_of(fl, cslot + 1u, f2);
        else if (!SHADOW) rn = normalize(mat3_mul(in2.nrm, n2));
        obj = i + 1;
      }
      if (SHADOW && rt <= t_stop) return obj;
      i += 2;
      cslot += 2u;
    } else {
      if (CULL && ((skip >> i) & 1ull) != 0ull) {
        i++;
        continue;
      }
      if (isect_inst<KdFlat, SHADOW>(sc, in, o, d, rwx, rwy, rwz, EPSILON, t_stop, rt, rn, (KdFlat*)nullptr)) obj = i;
      if (SHADOW && rt <= t_stop) return obj;
      i++;
    }
  }
  return obj;
}

// ------------------------------------------------------------------ a hit's shadow ray and bounce ray in one pass
// flat_query<false> of the bounce ray (o, db) and flat_query<true> of the shadow ray (o, ds, t_stop) in one walk over the
// objects (rpt_paths<KdFlat, false, true>; the host keeps a plane table and a second quotient table for it).  Each ray
// keeps its own record and visits the objects in object order, so every accept is the one its own query makes: the
// bounce slot's record (rtb, rnb, the object returned) is flat_query<false>'s, and the shadow slot's rts decides
// visibility as flat_query<true>'s does — it only skips work once rts <= t_stop, and rts never grows again, so
// `rts > t_stop` comes out the same.  What the shared origin allows is computed once: the plane-table numerators
// pv - o and each cube's inv * o.  The two rays' slab quotients, wall candidates and cube candidates sit side by side in
// straight-line code, so that the two dependency chains overlap.
// A slot that is off (no bounce ray: the path ends at this hit) enters with its record at -inf: no test accepts.
// CONSTS: as in flat_query.
template <bool CONSTS_>
RPT_DEV int flat_query2(const Scene& sc, const FlatLds* fl, D3 o, D3 db, D3 ds, double t_stop, double& rtb, D3& rnb,
                        double& rts) {
  constexpr bool CONSTS = CONSTS_ && SC_CUBE;
  int obj = -1;
  uint32_t cslot = 0;
  const int n = sc.num_objects;
  const uint32_t lane = __lane_id();
  const uint32_t nx = fl->plane_cnt & 15u, ny = (fl->plane_cnt >> 4) & 15u, nz = (fl->plane_cnt >> 8) & 15u;
  const uint32_t nq = nx + ny + nz;
  { // both rays' quotients (pv - o) / d: one numerator, two divisions (the bounce ray's table first, the shadow ray's behind it)
    const double RPT_C* pv = (const double RPT_C*)fl->plane_vals;
    double* qb = fl->qtab + lane;
    double* qs = qb + nq * 64u;
    for (uint32_t j = 0; j < nx; j++) { const double a = pv[j] - o.x; qb[j * 64u] = a / db.x; qs[j * 64u] = a / ds.x; }
    for (uint32_t j = 0; j < ny; j++) {
      const double a = pv[4u + j] - o.y;
      qb[(nx + j) * 64u] = a / db.y; qs[(nx + j) * 64u] = a / ds.y;
    }
    for (uint32_t j = 0; j < nz; j++) {
      const double a = pv[8u + j] - o.z;
      qb[(nx + ny + j) * 64u] = a / db.z; qs[(nx + ny + j) * 64u] = a / ds.z;
    }
  }
  int i = 0;
  while (i < n) {
    CInst& in = cinst(sc, i);
    if (in.kind == RPT_SHAPE_MESH && !in.has_xf && in.plane_use) { // a run of table users (flat_query above), both rays
      uint32_t cb = 0, cs = 0;
      double mb[FLAT_RUN], ms[FLAT_RUN];
      const int len = (int)in.plane_use;
      const double* qtb = fl->qtab + lane;
      const double* qts = qtb + nq * 64u;
      switch (len) {
        case 1: cb = run_slabs<1>(sc, i, qtb, rtb, mb); cs = run_slabs<1>(sc, i, qts, rts, ms); break;
        case 2: cb = run_slabs<2>(sc, i, qtb, rtb, mb); cs = run_slabs<2>(sc, i, qts, rts, ms); break;
        case 3: cb = run_slabs<3>(sc, i, qtb, rtb, mb); cs = run_slabs<3>(sc, i, qts, rts, ms); break;
        case 4: cb = run_slabs<4>(sc, i, qtb, rtb, mb); cs = run_slabs<4>(sc, i, qts, rts, ms); break;
        case 5: cb = run_slabs<5>(sc, i, qtb, rtb, mb); cs = run_slabs<5>(sc, i, qts, rts, ms); break;
        default: cb = run_slabs<FLAT_RUN>(sc, i, qtb, rtb, mb); cs = run_slabs<FLAT_RUN>(sc, i, qts, rts, ms); break;
      }
      if (rts <= t_stop) cs = 0u; // (the shadow ray is blocked already)
      while (__ballot((cb | cs) != 0u) != 0ull) {
        PROF_COUNT(PF_P_CAND);
        if (cb != 0u) { // the bounce ray's next candidate
          const int k = __ffs((int)cb) - 1;
          cb &= cb - 1u;
          double mt = mb[0];
#pragma unroll
          for (int kk = 1; kk < FLAT_RUN; kk++) mt = k == kk ? mb[kk] : mt;
          if (!(mt > rtb)) {
            const uint32_t* e = fl->obj_leaf[i + k];
            LaneTree lt{e[0], e[1]};
            KdNode nd;
            nd.split = 0.0; nd.a = e[2]; nd.ib = (e[3] << 2) | 3u;
            if (kd_leaf<true, false>(sc, lt, sc.refs + lt.ref_base, nd, o, db, EPSILON, -INF, rtb, rnb)) obj = i + k;
          }
        }
        if (cs != 0u) { // the shadow ray's
          const int k = __ffs((int)cs) - 1;
          cs &= cs - 1u;
          double mt = ms[0];
#pragma unroll
          for (int kk = 1; kk < FLAT_RUN; kk++) mt = k == kk ? ms[kk] : mt;
          if (!(mt > rts)) {
            const uint32_t* e = fl->obj_leaf[i + k];
            LaneTree lt{e[0], e[1]};
            KdNode nd;
            nd.split = 0.0; nd.a = e[2]; nd.ib = (e[3] << 2) | 3u;
            D3 srn = mk(0, 0, 0);
            kd_leaf<true, true>(sc, lt, sc.refs + lt.ref_base, nd, o, ds, EPSILON, t_stop, rts, srn);
            if (rts <= t_stop) cs = 0u;
          }
        }
      }
      i += len;
    } else if (in.kind == RPT_SHAPE_CUBE && in.has_xf && i + 1 < n && cinst(sc, i + 1).kind == RPT_SHAPE_CUBE &&
               cinst(sc, i + 1).has_xf) {
      // two consecutive Transformed<Cube> (flat_query above): cube by cube, both rays' candidates side by side, each
      // accepted in object order by its own record
      CInst* cu[2] = {&in, &cinst(sc, i + 1)};
#pragma unroll
      for (int c = 0; c < 2; c++) {
        const CInst& q = *cu[c];
        const D3 lo = mat4_mul(q.inv, o, 1.0);
        const D3 lb = mat4_mul(q.inv, db, 0.0), ls = mat4_mul(q.inv, ds, 0.0);
        const RcpD bx = rcp_make(lb.x), by = rcp_make(lb.y), bz = rcp_make(lb.z);
        const RcpD sx = rcp_make(ls.x), sy = rcp_make(ls.y), sz = rcp_make(ls.z);
        double tb = 0.0, ts = 0.0;
        D3 nb = mk(0, 0, 0), ns = mk(0, 0, 0);
        uint32_t fb = 0u;
        const bool hb = CONSTS ? cube_candidate_face(lo, bx, by, bz, EPSILON, tb, fb) : cube_candidate(lo, bx, by, bz, EPSILON, tb, nb);
        const bool hs = cube_candidate(lo, sx, sy, sz, EPSILON, ts, ns);
        if (hb && tb < rtb) {
          rtb = tb;
          if constexpr (CONSTS) rnb = cube_nrm_of(fl, cslot + (uint32_t)c, fb);
          else rnb = normalize(mat3_mul(q.nrm, nb)); // Transformed::intersect shape.rs:131-132
          obj = i + c;
        }
        if (hs && ts < rts) rts = ts;
      }
      i += 2;
      cslot += 2u;
    } else { // anything else: the object's own test, once per ray
      if (!(rtb == -INF)) {
        const RcpD rx = rcp_make(db.x), ry = rcp_make(db.y), rz = rcp_make(db.z);
        if (isect_inst<KdFlat, false>(sc, in, o, db, rx, ry, rz, EPSILON, -INF, rtb, rnb, (KdFlat*)nullptr)) obj = i;
      }
      if (!(rts <= t_stop)) {
        const RcpD rx = rcp_make(ds.x), ry = rcp_make(ds.y), rz = rcp_make(ds.z);
        D3 srn = mk(0, 0, 0);
        isect_inst<KdFlat, true>(sc, in, o, ds, rx, ry, rz, EPSILON, t_stop, rts, srn, (KdFlat*)nullptr);
      }
      i++;
    }
  }
  return obj;
}

#if RPT_SHADE_SPLIT
// ------------------------------------------------------------------ a hit's draws first, its shading in one block
// The fast form of the fused kernel's shading (rpt_paths<KdFlat, false, true>, RPT_SHADE_SPLIT): a wave whose light is
// an untransformed mesh and whose shading lanes all hit opaque materials (C2).  Every draw of a hit is taken first, in
// the reference's order and by its own loops: illuminate's triangle index and (u, v) pairs until u + v <= 1, then, if
// the path goes on, gen_bool(f), u_theta for the specular lobe and +-1 pairs until one is accepted (sample_f).  What
// the draws decide is kept as their integers, and the shading that follows is one straight-line block.
// (One loop for the whole sequence, a Philox block per lane and round with each lane stepping through its own state
// machine, was measured too: the per-round selects of that state cost far more than the blocks it saved, 25 % slower.)
struct HitDraws {
  uint64_t tri;   // the light triangle's index
  uint64_t a, b;  // the (u, v) pair that was kept
  uint64_t th;    // u_theta's draw (the specular lobe; a dummy 0.5 otherwise)
  uint64_t qa, qb; // the +-1 pair that was kept
  bool spec;      // gen_bool(f)
};
// sf: sample_f runs (depth < max_bounces); f: sample_f's lobe probability; mc (CONSTS): the material's constants, with
// gen_bool(f)'s threshold among them
template <bool CONSTS = false>
RPT_DEV void hit_draws(Rng& r, bool sf, uint64_t n, uint64_t zone, double f, HitDraws& o, const MatConsts* mc = nullptr) {
  o.tri = gen_index_zone(r, n, zone);
  next2_u64(r, o.a, o.b);
  while ((o.a >> 11) + (o.b >> 11) >= (1ull << 53) + 2ull) {
    PROF_COUNT(PF_P_REJECT);
    next2_u64(r, o.a, o.b);
  }
  o.th = 1ull << 63; o.qa = 0; o.qb = 0; o.spec = false;
  if (!sf) return;
  if constexpr (CONSTS) o.spec = f == 1.0 ? true : next_u64(r) < mc->p_int; // gen_bool: no draw when f == 1.0
  else o.spec = gen_bool(r, f);
  if (o.spec) o.th = next_u64(r);
  for (;;) {
    PROF_COUNT(PF_P_REJECT);
    next2_u64(r, o.qa, o.qb);
    const double x = u52_of(o.qa) * 2.0 + -1.0, y = u52_of(o.qb) * 2.0 + -1.0;
    const double sum = x * x + y * y;
    if (o.spec ? sum < 1.0 : sum <= 1.0) break;
  }
}

// bsdf() for an opaque material: both directions outside (the reflection case) or zero, its early return a select
// (CONSTS: m2, m2 * PI, f0 and one - f0 from the material's constants)
template <bool CONSTS = false>
RPT_DEV D3 bsdf_opaque(const Material& m, D3 n, D3 wo, D3 wi, const MatConsts* mc = nullptr) { // material.rs:125-170
  D3 color = ld3(m.color);
  double n_dot_wi = dot(n, wi);
  double n_dot_wo = dot(n, wo);
  const bool lit = !__builtin_signbit(n_dot_wi) && !__builtin_signbit(n_dot_wo);
  const D3 one = mk(1, 1, 1);
  double m2, m2pi;
  D3 f0, omf0;
  if constexpr (CONSTS) {
    m2 = mc->m2; m2pi = mc->m2pi;
    f0 = ld3(mc->f0); omf0 = ld3(mc->omf0);
  } else {
    m2 = m.roughness * m.roughness;
    m2pi = m2 * PI;
    double f0s = pow2((m.index - 1.0) / (m.index + 1.0));
    f0 = lerp(mk(f0s, f0s, f0s), color, m.metallic);
    omf0 = one - f0;
  }
  D3 h = normalize(wi + wo); // (wi * 1.0 + wo in bsdf)
  double wo_dot_h = dot(wo, h);
  double n_dot_h = dot(n, h);
  double nh2 = pow2(n_dot_h);
  double dd = rptc_exp((nh2 - 1.0) / (m2 * nh2)) / (m2pi * nh2 * nh2);
  D3 f = f0 + omf0 * pow5(1.0 - wo_dot_h);
  double ga = n_dot_wi * n_dot_h, gb = n_dot_wo * n_dot_h;
  double g = fmin(ga, gb);
  g = (2.0 * g) / wo_dot_h;
  g = fmin(g, 1.0);
  D3 q = dd * f * g / (4.0 * n_dot_wo * n_dot_wi);
  D3 diffuse = cmul(one - f, color) / PI;
  return lit ? q + diffuse : mk(0, 0, 0);
}

// sample_f() for an opaque material on the drawn values: both lobes' local vectors, the lane's one behind a select
template <bool CONSTS = false>
RPT_DEV void sample_f_opaque(const Material& m, D3 n, D3 wo, double f, const HitDraws& dr, D3& wi, double& pdf,
                             const MatConsts* mc = nullptr) {
  double m2; // material.rs:224-313
  if constexpr (CONSTS) m2 = mc->m2;
  else m2 = m.roughness * m.roughness;
  const double u_theta = (double)(dr.th >> 11) * (1.0 / 9007199254740992.0);
  const double x = u52_of(dr.qa) * 2.0 + -1.0, y = u52_of(dr.qb) * 2.0 + -1.0;
  const double sum = x * x + y * y;
  double theta = rptc_atan(sqrt(m2 * -rpt_log(u_theta)));
  double sin_t, cos_t;
  rptc_sincos_pio2(theta, &sin_t, &cos_t);
  double diff = x * x - y * y;
  double cx = diff / sum, cy = 2.0 * x * y / sum;
  const D3 loc = dr.spec ? mk(cx * sin_t, cy * sin_t, cos_t) : mk(x, y, sqrt(1.0 - x * x - y * y));
  const D3 world = local_to_world_mul(n, loc);
  wi = dr.spec ? -(wo - world * (dot(world, wo) * 2.0)) : world; // -glm::reflect_vec(wo, h)
  double p = 0.0;
  {
    D3 h = normalize(wi + wo);
    double p_h;
    if constexpr (CONSTS) { // beckmann_pdf with its PI * m2 from the table (the product m2 * PI: the same number)
      double cos_t = fabs(dot(h, n));
      double sin_t = sqrt(1.0 - cos_t * cos_t);
      p_h = (1.0 / (mc->m2pi * pow3(cos_t))) * rptc_exp(-pow2(sin_t / cos_t) / m2);
    } else {
      p_h = beckmann_pdf(m2, n, h);
    }
    p += f * p_h / (4.0 * fabs(dot(h, wo)));
  }
  p += (1.0 - f) * fmax(dot(wi, n), 0.0) * FRAC_1_PI;
  pdf = p;
}

// illuminate() of an untransformed mesh light on the drawn values (light.rs:23-47, mesh.rs:84-98, kdtree.rs:138-143)
// (CONSTS: Shape::sample's pdf of the drawn triangle, (1 / area) / num_prims, from the wave's table)
template <bool CONSTS = false>
RPT_DEV void illuminate_mesh(CLight& l, CTree& tr, const Tri* __restrict__ tp, D3 pos, const HitDraws& dr, D3& intensity,
                             D3& wi, double& dist, const double* light_pdf = nullptr) {
  const double u = (double)(dr.a >> 11) * (1.0 / 9007199254740992.0), v = (double)(dr.b >> 11) * (1.0 / 9007199254740992.0);
  double w = 1.0 - u - v;
  D3 v1 = ld3(tp->v), v2 = ld3(tp->v + 3), v3 = ld3(tp->v + 6);
  D3 n1 = ld3(tp->v + 9), n2 = ld3(tp->v + 12), n3 = ld3(tp->v + 15);
  SampleOut s{u * v1 + v * v2 + w * v3, normalize(u * n1 + v * n2 + w * n3), 0.0};
  if constexpr (CONSTS) {
    s.p = light_pdf[dr.tri];
  } else {
    double area = 0.5 * length(cross(v2 - v1, v3 - v1));
    s.p = 1.0 / area;
    s.p = s.p / (double)tr.num_prims;
  }
  D3 disp = s.v - pos;
  double len = length(disp);
  double cosine = fmax(-dot(disp, s.n), 0.0) / len;
  double surface_area = fmax(cosine, 0.0) / (len * len);
  intensity = ld3(l.mat_color) * l.mat_emittance * surface_area / s.p;
  wi = disp / len;
  dist = len;
}
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
    uint32_t nb = b + depth + 1u;
    if (nb >= ring) nb -= ring;
    fold_st = (fold_st & 0xffffu) | (nb << 16);
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
#ifndef RPT_STASH_REFILL_MIN
#define RPT_STASH_REFILL_MIN 32 // RayStashHit: the wave also refills once this many lanes have an empty stash
#endif
// a path that ends at `depth` with radiance A (path_ended) and the next path's header slot behind its records
RPT_DEV void end_path(const PersistArgs& pa, const Frame& fr, double* __restrict__ rec, double (*fold_l)[64],
                      uint32_t (*fold_u)[64], uint32_t lane, uint32_t& fold_st, uint32_t ring, const D3& A, uint32_t depth,
                      uint32_t s, uint32_t p_local) {
  const uint32_t b = fold_st >> 16;
  path_ended(pa, fr, rec, fold_l, fold_u, lane, fold_st, A, depth, b, s, p_local);
  if (depth != 0u) {
    uint32_t nb = b + depth + 1u; // the next path's header slot
    if (nb >= ring) nb -= ring;
    fold_st = (fold_st & 0xffffu) | (nb << 16);
  }
}
template <class LDS, bool PARK /* environment lookups parked per lane (pa.park_off) */,
          bool FUSE = false /* a hit's shadow ray and bounce ray in one query (FUSE below) */,
          bool CONSTS = false /* FUSE with a hit's scene constants in the wave's tables (SceneConsts above) */>
__global__ void __launch_bounds__(64, RPT_PATHS_WAVES) rpt_paths(Scene sc, Frame fr, Camera cam, PersistArgs pa) {
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
#endif
  const double dim = (double)max(fr.width, fr.height);
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
  using StashT = typename std::conditional<PRETRACE, RayStashHit, RayStash>::type;
  __shared__ typename std::conditional<STASH, StashT, int>::type stash_store;
  auto& stash = *reinterpret_cast<StashT*>(&stash_store);
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
    if constexpr (STASH) {
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
          camera_ray(fr, cam, dim, g_pixel, g_s, go, gd, gr);
#if RPT_PRETRACE_CULL
          if constexpr (FUSE) near = cull_near(pa.flat, g_pixel, fr.width);
#endif
          stash.v[0][lane] = go.x; stash.v[1][lane] = go.y; stash.v[2][lane] = go.z;
          stash.v[3][lane] = gd.x; stash.v[4][lane] = gd.y; stash.v[5][lane] = gd.z;
          stash.v[6][lane] = __longlong_as_double((long long)gr.hi);
          stash.u[0][lane] = g_p_local; stash.u[1][lane] = g_pixel; stash.u[2][lane] = g_s; stash.u[3][lane] = g_s_end;
          stash.u[4][lane] = gr.draw;
          stash_valid = true;
          pend = PRETRACE;
        }
        PROF_PHASE(PF_P_RAYGEN);
      }
      // ---- a lane whose path ended starts on its stashed ray (PRETRACE: after the closest hit)
      if (!PRETRACE && !in_path && stash_valid) {
        o = mk(stash.v[0][lane], stash.v[1][lane], stash.v[2][lane]);
        d = mk(stash.v[3][lane], stash.v[4][lane], stash.v[5][lane]);
        p_local = stash.u[0][lane]; pixel = stash.u[1][lane]; s = stash.u[2][lane]; s_end = stash.u[3][lane];
        rng = rng_make(fr.seed, pixel, fr.sample_base + s, 0);
        rng.draw = stash.u[4][lane];
        rng.hi = (uint64_t)__double_as_longlong(stash.v[6][lane]);
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
      // ---- ray generation (renderer.rs:132-139, camera.rs:64-81)
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
      if (__ballot(pend) != 0ull) {
        if (pend) {
          const D3 so = mk(stash.v[0][lane], stash.v[1][lane], stash.v[2][lane]);
          const D3 sd = mk(stash.v[3][lane], stash.v[4][lane], stash.v[5][lane]);
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
          const D3 hp = so + t * sd;
          stash.v[0][lane] = hp.x; stash.v[1][lane] = hp.y; stash.v[2][lane] = hp.z;
          stash.v[7][lane] = hn.x; stash.v[8][lane] = hn.y; stash.v[9][lane] = hn.z;
          stash.u[5][lane] = (uint32_t)ho;
          pend = false;
        }
      }
    } else if constexpr (PRETRACE) {
      // ---- closest hits: pass 0 (only when some lane has both) the pending pre-traces, pass 1 the running paths and
      // the pre-traces of lanes without one.  Every pass resets what the query writes, so no lane's result of pass 0
      // lives in registers across the query of pass 1.
#pragma unroll 1
      for (uint32_t pass = __ballot(pend && in_path) != 0ull ? 0u : 1u; pass < 2u; pass++) {
        const bool pre = pend, run = pend || (pass == 1u && in_path);
        if (pre) { // the stashed ray into the registers, the running one into its slots meanwhile
          const D3 so = mk(stash.v[0][lane], stash.v[1][lane], stash.v[2][lane]);
          const D3 sd = mk(stash.v[3][lane], stash.v[4][lane], stash.v[5][lane]);
          stash.v[0][lane] = o.x; stash.v[1][lane] = o.y; stash.v[2][lane] = o.z;
          stash.v[3][lane] = d.x; stash.v[4][lane] = d.y; stash.v[5][lane] = d.z;
          o = so;
          d = sd;
        }
        double t = INF;
        h_nrm = mk(0, 0, 0);
        h_obj = -1;
        if (run) {
          h_obj = flat_query<false>(sc, &fl, o, d, -INF, t, h_nrm);
          n_ext++;
          if (h_obj < 0) h_nrm = env_color(sc, d); // renderer.rs:147
        }
        h_pos = o + t * d;
        if (pre) {
          const D3 ro = mk(stash.v[0][lane], stash.v[1][lane], stash.v[2][lane]);
          const D3 rd = mk(stash.v[3][lane], stash.v[4][lane], stash.v[5][lane]);
          stash.v[0][lane] = h_pos.x; stash.v[1][lane] = h_pos.y; stash.v[2][lane] = h_pos.z;
          stash.v[3][lane] = d.x; stash.v[4][lane] = d.y; stash.v[5][lane] = d.z;
          stash.v[7][lane] = h_nrm.x; stash.v[8][lane] = h_nrm.y; stash.v[9][lane] = h_nrm.z;
          stash.u[5][lane] = (uint32_t)h_obj;
          o = ro;
          d = rd;
          pend = false;
        }
      }
    }
    if constexpr (PRETRACE) {
      PROF_PHASE(PF_P_HIT);
      // ---- the swap: a path whose ray escaped ends here (as in the miss branch below), and a lane without a running
      // path takes its stashed one — sample, Philox position and hit — into this iteration's shading
      if (in_path && h_obj < 0 && stash_valid) {
        end_path(pa, fr, rec, fold_l, fold_u, lane, fold_st, ring, h_nrm, depth, s, p_local);
        in_path = false;
      }
      if (!in_path && stash_valid) {
        h_pos = mk(stash.v[0][lane], stash.v[1][lane], stash.v[2][lane]);
        d = mk(stash.v[3][lane], stash.v[4][lane], stash.v[5][lane]);
        h_nrm = mk(stash.v[7][lane], stash.v[8][lane], stash.v[9][lane]);
        h_obj = (int)stash.u[5][lane];
        p_local = stash.u[0][lane]; pixel = stash.u[1][lane]; s = stash.u[2][lane]; s_end = stash.u[3][lane];
        rng = rng_make(fr.seed, pixel, fr.sample_base + s, 0);
        rng.draw = stash.u[4][lane];
        rng.hi = (uint64_t)__double_as_longlong(stash.v[6][lane]);
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
        const D3 wo = -normalize(d);
        const D3 color = mat.emittance * ld3(mat.color);
        D3 wl, lt, wi;
        double dist;
        bool cont;
#if RPT_SHADE_SPLIT
        // SHADE_SPLIT (hit_draws above): a wave whose light is an untransformed mesh and whose lanes hit opaque
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
            uint32_t pos = (fold_st >> 16) + 1u + depth; // slot b is the path's header, b + 1 + k its level k
            if (pos >= ring) pos -= ring;
            double* r = rec + pos * REC_FIELDS;
            r[3] = f.x; r[4] = f.y; r[5] = f.z;
            r[6] = 1.0 / pdf;
            r[7] = fabs(dot(wi, nrm));
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
          uint32_t pos = (fold_st >> 16) + 1u + depth; // slot b is the path's header, b + 1 + k its level k
          if (pos >= ring) pos -= ring;
          double* r = rec + pos * REC_FIELDS;
          r[3] = f.x; r[4] = f.y; r[5] = f.z;
          r[6] = 1.0 / pdf;
          r[7] = fabs(dot(wi, nrm));
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
          uint32_t pos = (fold_st >> 16) + 1u + depth;
          if (pos >= ring) pos -= ring;
          double* r = rec + pos * REC_FIELDS;
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
              uint32_t pos = (fold_st >> 16) + 1u + depth; // slot b is the path's header, b + 1 + k its level k
              if (pos >= ring) pos -= ring;
              double* r = rec + pos * REC_FIELDS;
              r[0] = A.x; r[1] = A.y; r[2] = A.z;
              r[3] = f.x; r[4] = f.y; r[5] = f.z;
              r[6] = inv_pdf;
              r[7] = abscos;
            }
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
      end_path(pa, fr, rec, fold_l, fold_u, lane, fold_st, ring, A_end, depth, s, p_local);
      s++;
      in_path = false;
    }
    PROF_PHASE(PF_P_RECORD);
    // ---- one step of the walker for every lane that owes one: L = A_k + min(1/pdf * (f . L) * |wi.n|, 100)
    // (renderer.rs:162-167), k = the deepest level not yet folded of the oldest path that ended
    if ((fold_st & 0xffffu) != 0u) {
      PROF_COUNT(PF_P_FOLDIT);
      const uint32_t wk = fold_st & 0xffffu, cb = fold_st >> 16;
      const uint32_t wD = fold_u[0][lane], wb = fold_u[1][lane];
      uint32_t pos = wb + wk; // level wk - 1 of the walker's path
      if (pos >= ring) pos -= ring;
      uint32_t nh = wb + wD + 1u; // header slot of the path behind it; == cb when no path waits
      if (nh >= ring) nh -= ring;
      const bool last = wk == 1u, more = last && nh != cb && (!park_on || nh != park_hd); // (a parked path's header is not written yet)
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
