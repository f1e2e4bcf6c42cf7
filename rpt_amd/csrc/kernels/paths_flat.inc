// kernels/paths_flat.inc — rpt_paths<KdFlat | KdFlatG | KdFlatF>'s closest-hit and visibility queries of flat scenes:
// cube_candidate_face, slab_window, run_slabs, flat_leaf_test, flat_query_filtered, cull_near / cull_skip_mask, flat_query, flat_query2.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ a cube's candidate with its face
// cube_candidate (shapes.inc) with the candidate's normal as its face (cube_face_normal): the same tests in the same order
RPT_DEV bool cube_candidate_face(D3 o, const RcpD& rdx, const RcpD& rdy, const RcpD& rdz, double t_min, double& time,
                                 uint32_t& face) {
  double x1, x2, y1, y2, z1, z2;
  uint32_t fx = 1u, fy = 3u, fz = 5u; // the ENTRY face along each axis: the normal -1 unless the interval was swapped
  div6<true>(-0.5 - o.x, 0.5 - o.x, rdx, -0.5 - o.y, 0.5 - o.y, rdy, -0.5 - o.z, 0.5 - o.z, rdz, x1, x2, y1, y2, z1, z2);
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
// the root slab test's window [b_min, b_max] from the six quotients (plane - o) / d of a box (kdtree.rs:130-134)
RPT_DEV void slab_window(double fax, double fbx, double fay, double fby, double faz, double fbz, double& b_min, double& b_max) {
  b_min = fmax(fmax(fmin(fax, fbx), fmin(fay, fby)), fmin(faz, fbz));
  b_max = fmin(fmin(fmax(fax, fbx), fmax(fay, fby)), fmax(faz, fbz));
}

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
    double b_min, b_max;
    slab_window(fax, fbx, fay, fby, faz, fbz, b_min, b_max);
    double mm = fmax(b_min, EPSILON);
    if (!(mm > fmin(b_max, rt))) cand |= 1u << k;
    m[k] = mm;
  }
  return cand;
}
// The shadow ray's window (RPT_SHADOW_WINDOW, flat_layout.h): of the run's N table users, those that are axis-flat
// (RPT_PLANE_AXIS_FLAT in plane_idx: the host verified, bit for bit, that the mesh lies in one axis plane — scene_plan.h
// axis_flat_mesh, with the proof) and whose slab entry m[k] lies beyond the light (rpt_shadow_window_beyond: more than 2^13
// doubles above t_stop, hence m[k] > t_stop * (1 + 2^-40)).  Every time such an object's leaf can accept is
// >= m[k] * (1 - 2^-50) > t_stop, so the shadow ray leaves it out: rts could only become a value above t_stop, and
// `rts > t_stop` is all the shadow slot returns.  The marks are wave-uniform scalars of records run_slabs has just read,
// m[] is run_slabs' own, and the comparison keeps no value alive.  0 when the switch is off
template <int N>
RPT_DEV uint32_t run_beyond(const Scene& sc, int i, const double (&m)[FLAT_RUN], double t_stop) {
  uint32_t drop = 0;
  if constexpr (RPT_SHADOW_WINDOW != 0) {
#pragma unroll
    for (int k = 0; k < N; k++)
      if ((cinst(sc, i + k).plane_idx & RPT_PLANE_AXIS_FLAT) != 0u && rpt_shadow_window_beyond(m[k], t_stop)) drop |= 1u << k;
  }
  return drop;
}
// run_slabs<len> of one ray, or of two side by side: the statement(s) with LEN = the run's length as a compile-time
// constant — one straight-line block per run length, no slot is evaluated in vain.  (A macro: the same switch as a
// function over a lambda cost the fused kernels SGPR spills, profiles/paths_split_resources.txt.)
#define RUN_SLABS_LEN(len, ...)                                       \
  switch (len) {                                                      \
    case 1: { constexpr int LEN = 1; __VA_ARGS__; } break;            \
    case 2: { constexpr int LEN = 2; __VA_ARGS__; } break;            \
    case 3: { constexpr int LEN = 3; __VA_ARGS__; } break;            \
    case 4: { constexpr int LEN = 4; __VA_ARGS__; } break;            \
    case 5: { constexpr int LEN = 5; __VA_ARGS__; } break;            \
    default: { constexpr int LEN = FLAT_RUN; __VA_ARGS__; } break;    \
  }
// m[k] of a lane's own candidate k (selects: m stays in registers).  A macro as well, one that yields the value: as a
// function taking m[] by reference, the same loop left m[] in scratch (profiles/paths_split_resources.txt).  k is
// evaluated once per slot: no side effects in it
#define RUN_PICK(m, k) ({ double pick_ = (m)[0]; \
  _Pragma("unroll") for (int kk_ = 1; kk_ < FLAT_RUN; kk_++) pick_ = (k) == kk_ ? (m)[kk_] : pick_; \
  pick_; })
// the leaf test of MESH object `obj`, a single-leaf tree, from its entry in FlatLds::obj_leaf (step 2 above; the ray in
// the object's own space).  PACKED: the object filter's entries, which carry kind and has_xf above the count's 8 bits
// DIVB: the leaf's divisions in batches (shapes.inc tri_batch)
template <bool SHADOW, bool PACKED = false, bool DIVB = false>
RPT_DEV bool flat_leaf_test(const Scene& sc, const FlatLds* fl, int obj, D3 o, D3 d, double t_stop, double& rt, D3& rn) {
  const uint32_t* e = fl->obj_leaf[obj];
  LaneTree lt{e[0], e[1]};
  KdNode nd;
  nd.split = 0.0; nd.a = e[2]; nd.ib = ((PACKED ? e[3] & 0xffu : e[3]) << 2) | 3u;
  return kd_leaf<true, SHADOW, DIVB>(sc, lt, sc.refs + lt.ref_base, nd, o, d, EPSILON, t_stop, rt, rn);
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
    double b_min, b_max; // (only the entry counts here)
    slab_window(fax, fbx, fay, fby, faz, fbz, b_min, b_max);
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
        double b_min, b_max;
        slab_window(fax, fbx, fay, fby, faz, fbz, b_min, b_max);
        if (!(fmax(b_min, EPSILON) > fmin(b_max, rt))) { // kdtree.rs:130-134
          D3 nn = rn;
          h = flat_leaf_test<SHADOW, true>(sc, fl, k, lo, ld, t_stop, rt, nn);
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

// an axis' share of the plane table: q[j][lane] = (pv[j] - o) / d for its cnt distinct planes (q: the lane's column).
// The quotients are independent of each other, so they go two at a time as one batch (vec.inc div_ieee)
RPT_DEV void plane_quotients(const double RPT_C* pv, uint32_t cnt, double o, double d, double* q) {
  uint32_t j = 0;
  for (; j + 2u <= cnt; j += 2u) {
    const double n2[2] = {pv[j] - o, pv[j + 1u] - o}, d2[2] = {d, d};
    double t[2];
    div_ieee<2>(n2, d2, t);
    q[j * 64u] = t[0]; q[(j + 1u) * 64u] = t[1];
  }
  for (; j < cnt; j++) q[j * 64u] = (pv[j] - o) / d;
}
// the same for the two rays of flat_query2, which share the numerators: two planes by both rays, a batch of four
RPT_DEV void plane_quotients2(const double RPT_C* pv, uint32_t cnt, double o, double db, double ds, double* qb, double* qs) {
  uint32_t j = 0;
  for (; j + 2u <= cnt; j += 2u) {
    const double a0 = pv[j] - o, a1 = pv[j + 1u] - o;
    const double n4[4] = {a0, a0, a1, a1}, d4[4] = {db, ds, db, ds};
    double t[4];
    div_ieee<4>(n4, d4, t);
    qb[j * 64u] = t[0]; qs[j * 64u] = t[1];
    qb[(j + 1u) * 64u] = t[2]; qs[(j + 1u) * 64u] = t[3];
  }
  for (; j < cnt; j++) {
    const double a = pv[j] - o;
    const double n2[2] = {a, a}, d2[2] = {db, ds};
    double t[2];
    div_ieee<2>(n2, d2, t);
    qb[j * 64u] = t[0]; qs[j * 64u] = t[1];
  }
}

// CULL (the pre-trace pass of rpt_paths<KdFlat, false, true>, RPT_PRETRACE_CULL): bit k of the wave-uniform `skip` = no
// ray of the wave can be accepted by object k (cull_skip_mask), its test is left out
// CONSTS (rpt_paths<KdFlat, false, true, true>): the two-cube block takes an accepted cube's world normal from the
// wave's table (SceneConsts, paths_consts.inc)
// DIVB: the query's divisions in batches (vec.inc div_ieee) — the fused kernels' pre-trace pass, which is the caller
// that sets CULL or CONSTS; the other kernels' queries keep the plain form (their registers: vec.inc)
template <bool SHADOW, bool CULL = false, bool CONSTS = false, bool DIVB = CULL || CONSTS>
RPT_DEV int flat_query(const Scene& sc, const FlatLds* fl, D3 o, D3 d, double t_stop, double& rt, D3& rn, uint64_t skip = 0ull) {
  int obj = -1;
  uint32_t cslot = 0; // CONSTS: the next two-cube block's first cube in the table of normals (cube_nrm_of)
  RcpD rwx = rcp_make(d.x), rwy = rcp_make(d.y), rwz = rcp_make(d.z);
  const int n = sc.num_objects;
  const uint32_t lane = __lane_id();
  if (fl->plane_cnt) { // every distinct (plane - o) / d once per ray: the operands, hence the bits, of the per-object form
    const double RPT_C* pv = (const double RPT_C*)fl->plane_vals;
    const uint32_t nx = fl->plane_cnt & 15u, ny = (fl->plane_cnt >> 4) & 15u, nz = (fl->plane_cnt >> 8) & 15u;
    if constexpr (DIVB && RPT_DIV_BATCH != 0) {
      double* q = fl->qtab + lane;
      plane_quotients(pv, nx, o.x, d.x, q);
      plane_quotients(pv + 4, ny, o.y, d.y, q + nx * 64u);
      plane_quotients(pv + 8, nz, o.z, d.z, q + (nx + ny) * 64u);
    } else {
      for (uint32_t j = 0; j < nx; j++) fl->qtab[j * 64u + lane] = (pv[j] - o.x) / d.x;
      for (uint32_t j = 0; j < ny; j++) fl->qtab[(nx + j) * 64u + lane] = (pv[4u + j] - o.y) / d.y;
      for (uint32_t j = 0; j < nz; j++) fl->qtab[(nx + ny + j) * 64u + lane] = (pv[8u + j] - o.z) / d.z;
    }
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
        RUN_SLABS_LEN(len, cand = run_slabs<LEN>(sc, i, qt, rt, m))
      } else { // no plane table (more than four distinct plane coordinates on some axis): discover the run here
#pragma unroll
      for (int k = 0; k < FLAT_RUN; k++) {
        m[k] = 0.0;
        if (len == k && i + k < n) { // the run is still growing
          CInst& q = cinst(sc, i + k);
          if (q.kind == RPT_SHAPE_MESH && !q.has_xf) {
            double fax, fbx, fay, fby, faz, fbz; // q.bounds == trees[q.tree].bounds (kdtree.rs:103)
            div6<DIVB>(q.bounds[0] - o.x, q.bounds[3] - o.x, rwx, q.bounds[1] - o.y, q.bounds[4] - o.y, rwy,
                 q.bounds[2] - o.z, q.bounds[5] - o.z, rwz, fax, fbx, fay, fby, faz, fbz);
            double b_min, b_max;
            slab_window(fax, fbx, fay, fby, faz, fbz, b_min, b_max);
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
          const double mt = RUN_PICK(m, k);
          if (!(mt > rt)) {
            if (flat_leaf_test<SHADOW, false, DIVB>(sc, fl, i + k, o, d, t_stop, rt, rn)) obj = i + k;
            if (SHADOW && rt <= t_stop) cand = 0u;
          }
        }
      }
      if (SHADOW && rt <= t_stop) return obj;
      i += len;
    } else if (xf_cube_pair(sc, i)) {
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
      bool c1 = TAB ? cube_candidate_face(lo1, ax, ay, az, EPSILON, t1, f1) : cube_candidate<DIVB>(lo1, ax, ay, az, EPSILON, t1, n1);
      bool c2 = TAB ? cube_candidate_face(lo2, bx, by, bz, EPSILON, t2, f2) : cube_candidate<DIVB>(lo2, bx, by, bz, EPSILON, t2, n2);
      if (c1 && t1 < rt) {
        rt = t1;
        if constexpr (TAB) rn = cube_nrm_of(fl, cslot, f1);
        else if (!SHADOW) rn = normalize_t<DIVB>(mat3_mul(in.nrm, n1)); // Transformed::intersect shape.rs:131-132
        obj = i;
      }
      if (SHADOW && rt <= t_stop) return obj;
      if (c2 && t2 < rt) {
        rt = t2;
        if constexpr (TAB) rn = cube_nrm_of(fl, cslot + 1u, f2);
        else if (!SHADOW) rn = normalize_t<DIVB>(mat3_mul(in2.nrm, n2));
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
// straight-line code, so that the two dependency chains overlap; its divisions go in batches (vec.inc div_ieee).
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
#if RPT_DIV_BATCH
    plane_quotients2(pv, nx, o.x, db.x, ds.x, qb, qs);
    plane_quotients2(pv + 4, ny, o.y, db.y, ds.y, qb + nx * 64u, qs + nx * 64u);
    plane_quotients2(pv + 8, nz, o.z, db.z, ds.z, qb + (nx + ny) * 64u, qs + (nx + ny) * 64u);
#else
    for (uint32_t j = 0; j < nx; j++) { const double a = pv[j] - o.x; qb[j * 64u] = a / db.x; qs[j * 64u] = a / ds.x; }
    for (uint32_t j = 0; j < ny; j++) {
      const double a = pv[4u + j] - o.y;
      qb[(nx + j) * 64u] = a / db.y; qs[(nx + j) * 64u] = a / ds.y;
    }
    for (uint32_t j = 0; j < nz; j++) {
      const double a = pv[8u + j] - o.z;
      qb[(nx + ny + j) * 64u] = a / db.z; qs[(nx + ny + j) * 64u] = a / ds.z;
    }
#endif
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
      RUN_SLABS_LEN(len, cb = run_slabs<LEN>(sc, i, qtb, rtb, mb); cs = run_slabs<LEN>(sc, i, qts, rts, ms);
                    cs &= ~run_beyond<LEN>(sc, i, ms, t_stop)) // (flat walls beyond the light)
      if (rts <= t_stop) cs = 0u; // (the shadow ray is blocked already)
      while (__ballot((cb | cs) != 0u) != 0ull) {
        PROF_COUNT(PF_P_CAND);
        if (cb != 0u) { // the bounce ray's next candidate
          const int k = __ffs((int)cb) - 1;
          cb &= cb - 1u;
          const double mt = RUN_PICK(mb, k);
          if (!(mt > rtb) && flat_leaf_test<false, false, true>(sc, fl, i + k, o, db, -INF, rtb, rnb)) obj = i + k;
        }
        if (cs != 0u) { // the shadow ray's
          const int k = __ffs((int)cs) - 1;
          cs &= cs - 1u;
          const double mt = RUN_PICK(ms, k);
          if (!(mt > rts)) {
            PROF_COUNT(PF_P_SHLEAF);
            D3 srn = mk(0, 0, 0);
            flat_leaf_test<true, false, true>(sc, fl, i + k, o, ds, t_stop, rts, srn);
            if (rts <= t_stop) cs = 0u;
          }
        }
      }
      i += len;
    } else if (xf_cube_pair(sc, i)) {
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
        const bool hb = CONSTS ? cube_candidate_face(lo, bx, by, bz, EPSILON, tb, fb) : cube_candidate<true>(lo, bx, by, bz, EPSILON, tb, nb);
        const bool hs = cube_candidate<true>(lo, sx, sy, sz, EPSILON, ts, ns);
        if (hb && tb < rtb) {
          rtb = tb;
          if constexpr (CONSTS) rnb = cube_nrm_of(fl, cslot + (uint32_t)c, fb);
          else rnb = normalize_b(mat3_mul(q.nrm, nb)); // Transformed::intersect shape.rs:131-132
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
