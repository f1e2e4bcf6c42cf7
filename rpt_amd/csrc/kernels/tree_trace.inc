// kernels/tree_trace.inc — the per-tree query's persistent walkers, rpt_tree_trace (one deep tree) and rpt_nest_trace (a
// kd-tree of kd-trees), and the steps the two share: the deferred write-out, the queue claim, the stack, the round's end.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// persistent traversal of one deep tree over the queued rays.  Latency-bound (L2/HBM misses on nodes and
// leaf records), so it runs at its own, higher occupancy: RPT_TT_WAVES waves/SIMD with the first
// RPT_TT_LEVELS stack levels in LDS (RPT_TT_WAVES * 4 * 64 lanes * 20 B * levels <= 160 KB per CU).
using KdLdsTT = KdLdsT<RPT_TT_LEVELS, 256>;
// (An LDS table of the ray's axis-indexed operands in place of the node step's three 3-way selects — 24 instead of 37
// VALU instructions per step — and the LDS levels as a window over the TOP of the stack were built and measured in round
// 5: variants/tree_trace_axis_table_top_window.patch.  The step is bound by its dependent child-pair load, not by VALU
// issue: 1.5 % for a third of the instructions, less than the LDS levels the table costs.)
using KdLdsTree = KdLdsTT;
struct TreeTraceLds {
  KdLdsTree st;
};

// ------------------------------------------------------------------ the steps both walkers take
// Write out the results of the rays that finished since the last refill.  A lane whose ray is done idles until the wave
// refills anyway, so its normal transform and its five scattered stores (hit_epilogue) wait until then and run ONCE for all
// of them instead of in nearly every iteration for one or two lanes (measured: no difference in kernel time — the block
// was never waited for).  fin: the lane's ray is done and hit something, result not yet written out; the caller clears it.
template <bool SHADOW>
RPT_DEV void write_finished(bool fin, const RayBatch& rb, CInst& in, int obj_index, uint32_t slot, double rt, D3 rn) {
  if (__ballot(fin) != 0) {
    if (fin) hit_epilogue<SHADOW>(rb, in, obj_index, slot, rt, rn);
  }
}

// Refill: the idle lanes (need; need_mask = their ballot, not empty) claim the next positions of the tree's queue with one
// atomic per wave.  true: this lane has one, `pos` — the row of the entry table and, through the query's queue, the slot;
// a lane that asked behind the queue's end is `exhausted` and asks no more.
RPT_DEV bool queue_claim(bool need, uint64_t need_mask, const uint32_t* __restrict__ tq, uint32_t count,
                         uint32_t* __restrict__ tq_head, uint32_t& pos, bool& exhausted) {
  const uint32_t lane = __lane_id();
  uint32_t leader = (uint32_t)__ffsll((long long)need_mask) - 1u;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(tq_head, (uint32_t)__popcll(need_mask));
  base = __shfl(base, (int)leader);
  if (!need) return false;
  uint32_t idx = base + (uint32_t)__popcll(need_mask & ((1ull << lane) - 1ull));
  if (idx < count) {
    pos = tq[idx];
    return true;
  }
  exhausted = true;
  return false;
}

// The traversal stack: the first L deferred children of a lane sit in LDS ([level][thread], bank-conflict free),
// deeper ones — rare: most levels of a descent defer nothing — in a global-memory spill area of the same shape, one
// column per thread of this (persistent) grid, addressed as GLOBAL memory.  No scratch: a private array indexed by
// the stack pointer next to the LDS levels made the compiler select between the two POINTERS and emit flat loads.
struct SpillCols {
  uint32_t* sp_node;
  double* sp_ts;
  double* sp_bmax;
  uint32_t threads; // the columns' stride
};
RPT_DEV SpillCols spill_cols(const StackSpill& spill) {
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  return {spill.node + gtid, spill.ts + gtid, spill.bmax + gtid, spill.threads};
}
RPT_DEV void stack_push(KdLdsTT& lds, const SpillCols& sc, int& sp, uint32_t far, double ts, double b_max) {
  constexpr int L = KdLdsTT::levels;
  const uint32_t tix = threadIdx.x;
  if (sp < L) { lds.node[sp][tix] = far; lds.ts[sp][tix] = ts; lds.bmax[sp][tix] = b_max; }
  else {
    const uint64_t k = (uint64_t)(sp - L) * sc.threads;
    sc.sp_node[k] = far; sc.sp_ts[k] = ts; sc.sp_bmax[k] = b_max;
  }
  sp++;
}
// Resume the lane's nearest deferred far child above `floor` that can still matter (kdtree.rs:213-220); false: there is none.
// The LDS entry is read unconditionally (clamped level, volatile) and a spilled one overrides it: with the two sides in
// an if / else — or speculated — the compiler selects between the POINTERS and emits flat loads.
RPT_DEV bool stack_pop(KdLdsTT& lds, const SpillCols& sc, int& sp, int floor, double rt, uint32_t& node, double& b_min,
                       double& b_max, double& t_min) {
  constexpr int L = KdLdsTT::levels;
  const uint32_t tix = threadIdx.x;
  while (sp > floor) {
    PROF_COUNT(PF_TT_POP);
    sp--;
    const int spc = min(sp, L - 1);
    double ts = lds_read_f64(&lds.ts[spc][tix]), bm = lds_read_f64(&lds.bmax[spc][tix]);
    uint32_t nd = lds_read_u32(&lds.node[spc][tix]);
    if (sp >= L) {
      const uint64_t k = (uint64_t)(sp - L) * sc.threads;
      ts = sc.sp_ts[k]; bm = sc.sp_bmax[k]; nd = sc.sp_node[k];
    }
    if (rt < ts) continue;
    node = nd; b_min = ts; b_max = bm; t_min = ts;
    return true;
  }
  return false;
}

// One node step of the compact traversal (kdtree.rs:172-222; kd_intersect_fast's, traversal.inc) for the lane's inner node
// n: defers the far child if both can matter, narrows the slab interval, and leaves the near child in n / axis / node.
// ZEROS: the ray may have a zero direction component.  true — nothing done — for a 0/0 split: the origin lies ON the split
// plane of an axis the ray does not move along, and only the general form walks that (rpt_tree_generic).
// FAST: t_split = (value - o) / d through the ray's refined reciprocals (rcx, rcy, rcz) where the wave may (wave_fast:
// tree_trace_body says when); both sides give the same bits.
template <bool SHADOW, bool ZEROS, bool FAST>
RPT_DEV bool node_step(const KdNode* __restrict__ nodes, KdNode& n, uint32_t& axis, uint32_t& node, const D3& o, const D3& d,
                       double rcx, double rcy, double rcz, bool wave_fast, double rt, double t_min, double t_stop,
                       double& b_min, double& b_max, KdLdsTT& lds, const SpillCols& cols, int& sp) {
  PROF_COUNT(PF_TT_NODE);
  // both children (adjacent, 32 B) are requested before the split is evaluated: the division and the
  // decision below run while the load is in flight, and the chosen child is already in registers
  const KdNode* __restrict__ ch = nodes + n.a; // one address for the adjacent pair
  KdNode c0 = ch[0], c1 = ch[1];
  double value = n.split;
  double o_ax = sel((int)axis, o), d_ax = sel((int)axis, d);
  double ts;
  if (FAST && wave_fast) {
    const double num = value - o_ax, r_ax = axis == 0 ? rcx : (axis == 1 ? rcy : rcz);
    const double q = num * r_ax;
    ts = __builtin_fma(__builtin_fma(-d_ax, q, num), r_ax, q);
  } else {
    ts = (value - o_ax) / d_ax;
  }
  if constexpr (ZEROS) {
    if (ts != ts) return true;
  }
  // the decisions as mask arithmetic (| and & on lane masks): `||` / `&&` compile to one masked region and one
  // branch per operand — thirteen branches per step instead of eight, C3 195 -> 198
  // (without a zero component d_ax <= 0 IS d_ax < 0: one compare serves `dle` and `neg`)
  const bool neg = d_ax < 0.0;
  const bool lt = o_ax < value, eq = o_ax == value, dle = ZEROS ? d_ax <= 0.0 : neg;
  const bool left_first = lt | (eq & dle);
  const double lim_hi = fmin_raw(b_max, rt), lim_lo = fmax_raw(b_min, t_min);
  const bool only_first = (ts > lim_hi) | (ts <= 0.0);
  const bool only_second = !only_first & (ts < lim_lo);
  const bool go_left = only_second != left_first;
  const bool defer = !only_first & !only_second & !(SHADOW & (ts > t_stop));
  if (defer) stack_push(lds, cols, sp, n.a + (left_first ? 1u : 0u), ts, b_max);
  if (!ZEROS || d_ax != 0.0) { // a zero component: the child's slab interval is the parent's (traversal.inc)
    if (go_left != neg) b_max = fmin_raw(b_max, ts);
    else b_min = fmax_raw(b_min, ts);
  }
  node = n.a + (go_left ? 0u : 1u);
  n = go_left ? c0 : c1;
  axis = n.ib & 3u;
  return false;
}

// The end of a round of the while-while traversal: nobody has a ray, or too few lanes still have one while the queue may
// hold more — then the wave goes back and refills.  Once the queue is exhausted it runs to completion.
RPT_DEV bool round_over(bool active, bool exhausted) {
  uint32_t n_active = (uint32_t)__popcll(__ballot(active));
  bool more = __ballot(!exhausted) != 0; // some lane may still get a ray from the queue
  return n_active == 0 || (more && n_active < RPT_REFILL_BELOW);
}

// ------------------------------------------------------------------ rpt_tree_trace
// ZEROS: the form for the rays with a zero direction component (their own queue, see rpt_tree_enter)
// This body keeps its own copy of the steps above — the write-out with a hit's epilogue, the claim, the entry row and
// the slab of the refill, the node step with its push, the pop, the exit test — expression for expression: through the
// functions the compiler allocated the kernel's registers otherwise (121 instead of 123 VGPRs, ten instructions more)
// and rpt_tree_trace<true, ...> took 0.6 % longer on the 100k-triangle mesh, whichever single step was shared
// (profiles/wavefront_split_ab.txt).  As written here its code is what it was before the steps were shared, instruction
// for instruction.  A change to a step goes into both copies; each copy below names the function it repeats.
template <bool TRIS, bool SHADOW, bool ZEROS>
RPT_DEV void tree_trace_body(TreeTraceLds& tl, const Scene& sc, const RayBatch& rb, const int obj_index,
                             const uint32_t* __restrict__ queue, const uint32_t* __restrict__ tq,
                             const uint32_t* __restrict__ tq_count, uint32_t* __restrict__ tq_head,
                             uint32_t* __restrict__ fq, uint32_t* __restrict__ fq_count, const StackSpill& spill) {
  KdLdsTree& lds = tl.st;
  constexpr int L = KdLdsTree::levels;
  CInst& in = cinst(sc, obj_index);
  CTree& tr = ctree(sc, in.tree);
  const KdNode* __restrict__ nodes = sc.nodes + tr.node_base;
  const uint32_t* __restrict__ refs = sc.refs + tr.ref_base;
  const uint32_t count = *tq_count;
  const uint32_t lane = __lane_id(), tix = threadIdx.x;
  // (spill_cols)
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t* __restrict__ sp_node = spill.node + gtid;
  double* __restrict__ sp_ts = spill.ts + gtid;
  double* __restrict__ sp_bmax = spill.bmax + gtid;

  bool active = false, exhausted = false, found = false;
  bool fin = false; // the lane's ray is done and hit something: result not yet written out
  uint32_t slot = 0, node = 0;
  int sp = 0;
  D3 o = mk(0, 0, 0), d = mk(0, 0, 1), rn = mk(0, 0, 0);
  double rt = INF, t_min = EPSILON, t_stop = -INF, b_min = 0.0, b_max = 0.0;
  BoxRay br{};
  PROF_INIT();
  // t_split = (value - o) / d through the ray's refined reciprocals (div_fast, vec.inc: three instructions that ARE the
  // IEEE quotient when numerator and denominator are in [2^-400, 2^400]).  The range is established per RAY, not per
  // step: a tree whose splits are all 0 or in [2^-340, 2^399) (Tree::split_range_ok), an origin whose coordinates are,
  // and direction components in [2^-400, 2^400) make every numerator 0 — exact: 0 * r = 0 with the quotient's sign —
  // or at least 2^-393.  The choice is per WAVE and refreshed at every refill; both sides give the same bits.
  // Measured on the 100k-triangle mesh: 188 -> 192 Msamples/s (-> 195 with fmin_raw / fmax_raw, vec.inc).
  double rcx = 0.0, rcy = 0.0, rcz = 0.0;
  bool fast_ok = true, wave_fast = false;

  for (;;) {
    // ---- write_finished
    if (__ballot(fin) != 0) {
      if (fin) {
        rb.rt[slot] = rt; // hit_epilogue
        if (!SHADOW) {
          if (in.has_xf) rn = normalize(mat3_mul(in.nrm, rn)); // Transformed::intersect shape.rs:131-132
          st_soa3(rb.rn, rb.n_stride, slot, rn);
          rb.obj[slot] = obj_index;
        }
        fin = false;
      }
    }
    PROF_PHASE(PF_TT_WRITE); // result write-out
    // ---- refill idle lanes from the tree's queue: queue_claim, entry_ray / entry_record, slab_quotients / slab_fold
    bool need = !active && !exhausted;
    uint64_t need_mask = __ballot(need);
    if (need_mask) {
      uint32_t leader = (uint32_t)__ffsll((long long)need_mask) - 1u;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(tq_head, (uint32_t)__popcll(need_mask));
      base = __shfl(base, (int)leader);
      if (need) {
        uint32_t idx = base + (uint32_t)__popcll(need_mask & ((1ull << lane) - 1ull));
        if (idx < count) {
          const uint32_t pos = tq[idx];
          const double* __restrict__ e = spill.rays + (uint64_t)pos * 8u; // rpt_tree_enter's row: object-space ray, record, stop
          slot = queue ? queue[pos] : pos;
          o = mk(e[0], e[1], e[2]);
          d = mk(e[3], e[4], e[5]);
          rt = e[6];
          if (SHADOW) t_stop = e[7];
          double fax = (tr.bounds[0] - o.x) / d.x, fbx = (tr.bounds[3] - o.x) / d.x;
          double fay = (tr.bounds[1] - o.y) / d.y, fby = (tr.bounds[4] - o.y) / d.y;
          double faz = (tr.bounds[2] - o.z) / d.z, fbz = (tr.bounds[5] - o.z) / d.z;
          b_min = fmax(fmax(fmin(fax, fbx), fmin(fay, fby)), fmin(faz, fbz));
          b_max = fmin(fmin(fmax(fax, fbx), fmax(fay, fby)), fmax(faz, fbz));
          node = 0; sp = 0; t_min = EPSILON; found = false;
          rn = mk(0, 0, 0);
          br = boxray_make<!TRIS>(tr, o, d, fmax(b_min, 0.0));
          if (!sc.use_leaf_boxes) br.on = false;
          if constexpr (!ZEROS) {
            RcpD qx = rcp_make(d.x), qy = rcp_make(d.y), qz = rcp_make(d.z);
            rcx = qx.r; rcy = qy.r; rcz = qz.r;
            fast_ok = tr.split_range_ok && qx.ok && qy.ok && qz.ok && safe_coord(o.x) && safe_coord(o.y) && safe_coord(o.z);
          }
          active = true;
        } else {
          exhausted = true;
        }
      }
      if constexpr (!ZEROS) wave_fast = __ballot(active && !fast_ok) == 0ull;
    }
    PROF_PHASE(PF_TT_REFILL);
    if (__ballot(active) == 0) break;

    // ---- while-while traversal (the loop structure of kd_intersect_fast) until too few lanes
    // still have a ray; then go back and refill.  Once the queue is exhausted, run to completion.
    for (;;) {
      if (active) {
        KdNode n = nodes[node];
        uint32_t axis = n.ib & 3u;
        while (axis != 3u) { // kdtree.rs:172-222, compact form
          PROF_COUNT(PF_TT_NODE); // node_step<SHADOW, ZEROS, !ZEROS>, with stack_push
          const KdNode* __restrict__ ch = nodes + n.a; // one address for the adjacent pair
          KdNode c0 = ch[0], c1 = ch[1];
          double value = n.split;
          double o_ax = sel((int)axis, o), d_ax = sel((int)axis, d);
          double ts;
          if (!ZEROS && wave_fast) {
            const double num = value - o_ax, r_ax = axis == 0 ? rcx : (axis == 1 ? rcy : rcz);
            const double q = num * r_ax;
            ts = __builtin_fma(__builtin_fma(-d_ax, q, num), r_ax, q);
          } else {
            ts = (value - o_ax) / d_ax;
          }
          if constexpr (ZEROS) {
            if (ts != ts) {
              // 0/0: the origin lies ON the split plane of an axis the ray does not move along (kd_intersect_fast,
              // traversal.inc).  The ray is handed to rpt_tree_generic, which starts it over in the general form; here
              // it ends at an empty leaf with nothing found, so nothing of it is written out.
              fq[atomicAdd(fq_count, 1u)] = slot;
              n.a = 0u; n.ib = 3u; sp = 0; found = false;
              break;
            }
          }
          const bool neg = d_ax < 0.0;
          const bool lt = o_ax < value, eq = o_ax == value, dle = ZEROS ? d_ax <= 0.0 : neg;
          const bool left_first = lt | (eq & dle);
          const double lim_hi = fmin_raw(b_max, rt), lim_lo = fmax_raw(b_min, t_min);
          const bool only_first = (ts > lim_hi) | (ts <= 0.0);
          const bool only_second = !only_first & (ts < lim_lo);
          const bool go_left = only_second != left_first;
          const bool defer = !only_first & !only_second & !(SHADOW & (ts > t_stop));
          if (defer) {
            uint32_t far = n.a + (left_first ? 1u : 0u);
            if (sp < L) { lds.node[sp][tix] = far; lds.ts[sp][tix] = ts; lds.bmax[sp][tix] = b_max; }
            else {
              const uint64_t k = (uint64_t)(sp - L) * spill.threads;
              sp_node[k] = far; sp_ts[k] = ts; sp_bmax[k] = b_max;
            }
            sp++;
          }
          if (!ZEROS || d_ax != 0.0) { // a zero component: the child's slab interval is the parent's (traversal.inc)
            if (go_left != neg) b_max = fmin_raw(b_max, ts);
            else b_min = fmax_raw(b_min, ts);
          }
          node = n.a + (go_left ? 0u : 1u);
          n = go_left ? c0 : c1;
          axis = n.ib & 3u;
        }
        PROF_PHASE(PF_TT_NODE);
        bool h = false;
        {
          if constexpr (TRIS) h = kd_leaf_boxed<SHADOW>(sc, tr, refs, n, o, d, t_min, t_stop, rt, rn, br);
          else
            h = kd_leaf<TRIS, SHADOW>(sc, tr, refs, n, o, d, t_min, t_stop, rt, rn, &br);
        }
        found = found || h;
        PROF_PHASE(PF_TT_EXACT); // (kd_leaf_boxed marks the end of its box tests itself)
        bool finished = SHADOW && rt <= t_stop;
        if (!finished) { // stack_pop, floor 0
          bool resumed = false;
          while (sp > 0) {
            PROF_COUNT(PF_TT_POP);
            sp--;
            double ts, bm;
            uint32_t nd;
            const int spc = min(sp, L - 1);
            ts = lds_read_f64(&lds.ts[spc][tix]); bm = lds_read_f64(&lds.bmax[spc][tix]);
            nd = lds_read_u32(&lds.node[spc][tix]);
            if (sp >= L) {
              const uint64_t k = (uint64_t)(sp - L) * spill.threads;
              ts = sp_ts[k]; bm = sp_bmax[k]; nd = sp_node[k];
            }
            if (rt < ts) continue;
            node = nd; b_min = ts; b_max = bm; t_min = ts;
            resumed = true;
            break;
          }
          finished = !resumed;
        }
        PROF_PHASE(PF_TT_POP);
        if (finished) {
          fin = found; // written out before the next refill
          active = false;
        }
      }
      uint32_t n_active = (uint32_t)__popcll(__ballot(active));
      bool more = __ballot(!exhausted) != 0; // round_over
      if (n_active == 0 || (more && n_active < RPT_REFILL_BELOW)) break;
    }
  }
  PROF_FLUSH();
}
// The kernel: one pass of the loop above.  ZEROS = false: the tree's queue.  ZEROS = true: the queue of its rays with a
// zero direction component — launched only for scenes that make such rays common (StackSpill::zeros_common: a
// directional light along an axis or in a coordinate plane).  Everywhere else rpt_tree_enter hands the few there are to
// rpt_tree_generic, which is launched anyway: until round 5 every (tree, query) pair paid an 8-us launch of the ZEROS
// build that found its queue empty (wine glass: 68 per step).  Both forms in ONE launch (the ZEROS pass inlined behind the
// main one, or called) cost the main loop registers: +1.5 % kernel time on the 100k-triangle mesh, or 0.5 KB of scratch.
template <bool TRIS, bool SHADOW, bool ZEROS>
__global__ void __launch_bounds__(256, RPT_TT_WAVES) rpt_tree_trace(Scene sc, RayBatch rb, int obj_index,
                                                                    const uint32_t* __restrict__ queue,
                                                                    const uint32_t* __restrict__ tq,
                                                                    const uint32_t* __restrict__ tq_count,
                                                                    uint32_t* __restrict__ tq_head,
                                                                    uint32_t* __restrict__ fq,
                                                                    uint32_t* __restrict__ fq_count, StackSpill spill) {
  __shared__ TreeTraceLds tl;
  tree_trace_body<TRIS, SHADOW, ZEROS>(tl, sc, rb, obj_index, queue, tq, tq_count, tq_head, fq, fq_count, spill);
}

#ifdef RPT_EXT_SHAPES
// rpt_nest_trace: rpt_tree_trace for a kd-tree of kd-trees (examples/fractal_teapots.rs: 937 placed copies of a 12-level
// mesh tree under 7-level group trees), BOTH levels in the one persistent loop.  rpt_tree_trace<false> walks the group's
// tree and, at a leaf, calls isect_child_mesh for a mesh child: the lanes that have one run their inner traversals side
// by side and wait for the longest — 7 of 64 lanes per inner node step, because a ray that clips a corner of a child's
// bounds takes two steps and one through the teapot sixty.  Here a lane is EITHER in the group's tree or in one child's
// tree (node base, ray, slab interval, box parameters are per-lane state; one stack, the child's entries above sp_in),
// every pass gives each lane a turn at what IT needs next — node steps, then its leaf — and a lane whose child is
// done walks on through the group, finishes its ray and takes the next from the queue: nobody waits for a neighbour's
// child.  Per ray the sequence of tests, the record they see and every operand are those of the nested form, i.e. of
// the reference's recursion (kdtree.rs:151-223 inside Transformed::intersect shape.rs:128-137 inside kdtree.rs:162-171).
// The node step is kd_intersect_fast's, zero direction components included, so the queue of the rays that have one (zq)
// runs through this kernel too; a 0/0 split sends the ray to rpt_tree_generic, which starts it over.  No calls, hence no
// call frames in scratch (the nested form's chain of out-of-line traversals needs 14 KB per lane): the host sends an
// object here only when its tree and all its mesh children's trees are regular, none of its children is a group, and
// the two levels' depths fit one stack (scene_plan.h route_object); otherwise, and under RPT_FLAG_GENERAL_TRAVERSAL, rpt_tree_trace<false>.
struct NestTree {
  uint32_t ref_base, prim_base; // what kd_leaf reads of a mesh tree
};
template <bool SHADOW>
RPT_DEV void nest_trace_body(KdLdsTT& lds, const Scene& sc, const RayBatch& rb, const int obj_index,
                             const uint32_t* __restrict__ queue, const uint32_t* __restrict__ tq,
                             const uint32_t* __restrict__ tq_count, uint32_t* __restrict__ tq_head,
                             uint32_t* __restrict__ fq, uint32_t* __restrict__ fq_count, const StackSpill& spill) {
  CInst& in = cinst(sc, obj_index);
  CTree& tr = ctree(sc, in.tree);
  const uint32_t* __restrict__ refs0 = sc.refs + tr.ref_base;
  const LeafBox* __restrict__ boxes0 = sc.lbox + tr.ref_base;
  const Inst* __restrict__ kids = sc.insts + tr.prim_base;
  const uint32_t count = *tq_count;
  const SpillCols cols = spill_cols(spill);

  bool active = false, exhausted = false, found = false, fin = false;
  uint32_t slot = 0, node = 0;
  int sp = 0, sp_in = 0;
  D3 o = mk(0, 0, 0), d = mk(0, 0, 1), rn = mk(0, 0, 0);
  double rt = INF, t_min = EPSILON, t_stop = -INF, b_min = 0.0, b_max = 0.0;
  double t0_root = 0.0, t_min_leaf = EPSILON; // the group tree's: where its box parameters count from; t_min at the leaf
  BoxRay br{};                                // of the tree the lane is in
  const KdNode* __restrict__ nodes = sc.nodes + tr.node_base;
  bool inner = false, in_leaf = false;
  const Inst* __restrict__ child = kids;
  NestTree ct{0u, 0u};
  uint32_t lf_first = 0, lf_cnt = 0, lf_base = 0, lf_next = 0, lf_mask = 0;
  PROF_INIT();

  // the ray in the group's space: rpt_tree_enter's row (read again when a lane comes back from a child: twelve
  // registers less to carry through the child's traversal)
  uint32_t pos = 0;

  for (;;) {
    write_finished<SHADOW>(fin, rb, in, obj_index, slot, rt, rn);
    fin = false;
    PROF_PHASE(PF_TT_WRITE);
    const bool need = !active && !exhausted;
    const uint64_t need_mask = __ballot(need);
    if (need_mask) {
      if (queue_claim(need, need_mask, tq, count, tq_head, pos, exhausted)) {
        slot = queue ? queue[pos] : pos;
        entry_ray(spill.rays, pos, o, d);
        entry_record<SHADOW>(spill.rays, pos, rt, t_stop);
        slab_fold(slab_quotients(tr, o, d), b_min, b_max);
        node = 0; sp = 0; t_min = EPSILON; found = false;
        rn = mk(0, 0, 0);
        t0_root = fmax(b_min, 0.0);
        br = boxray_make<true>(tr, o, d, t0_root);
        if (!sc.use_leaf_boxes) br.on = false;
        nodes = sc.nodes + tr.node_base;
        inner = false; in_leaf = false;
        active = true;
      }
    }
    PROF_PHASE(PF_TT_REFILL);
    if (__ballot(active) == 0) break;

    for (;;) {
      if (active) {
        bool bail = false;
        if (!in_leaf || inner) { // (a lane in the middle of a group leaf has no node to step through)
          KdNode n = nodes[node];
          uint32_t axis = n.ib & 3u;
          while (axis != 3u) { // kdtree.rs:172-222, compact form (kd_intersect_fast's step: either level)
            // (a child's ray may have a zero component the group's has not)
            if (node_step<SHADOW, true, false>(nodes, n, axis, node, o, d, 0.0, 0.0, 0.0, false, rt, t_min, t_stop, b_min, b_max, lds, cols, sp)) { bail = true; break; }
          }
          PROF_PHASE(PF_TT_NODE);
          if (!bail) {
            if (inner) { // a leaf of the child's mesh tree
              D3 nn = mk(0, 0, 0);
              bool h = kd_leaf<true, SHADOW>(sc, ct, sc.refs + ct.ref_base, n, o, d, t_min, t_stop, rt, nn, &br);
              if (h) { // Transformed::intersect's epilogue for the hit that stands so far (shape.rs:131-132)
                found = true;
                if (!SHADOW) rn = child->has_xf ? normalize(mat3_mul(child->nrm, nn)) : nn;
              }
            } else { // a fresh leaf of the group's tree
              lf_first = n.a; lf_cnt = n.ib >> 2; lf_next = 0; lf_mask = 0;
              in_leaf = true;
            }
          }
          PROF_PHASE(PF_TT_EXACT);
        }
        bool finished = bail || (SHADOW && rt <= t_stop);
        if (!finished && inner) {
          if (!stack_pop(lds, cols, sp, sp_in, rt, node, b_min, b_max, t_min)) { // the child is done: back to the group's leaf
            inner = false;
            entry_ray(spill.rays, pos, o, d);
            nodes = sc.nodes + tr.node_base;
            t_min = t_min_leaf;
            br = boxray_make<true>(tr, o, d, t0_root);
            if (!sc.use_leaf_boxes) br.on = false;
          }
        }
        if (!finished && !inner && in_leaf) {
          // the group's leaf: its children in leaf order (kdtree.rs:162-171) until one is a mesh to walk
          bool entered = false;
          while (!entered) {
            if (lf_mask == 0u) {
              if (lf_next >= lf_cnt) break; // leaf exhausted
              lf_base = lf_next;
              const uint32_t lim = min(lf_cnt - lf_base, 32u);
              lf_next = lf_base + 32u;
              uint32_t m = lim >= 32u ? 0xffffffffu : ((1u << lim) - 1u);
              if (br.on && lf_cnt > 2u) {
                float wl, wh;
                box_window(br, t_min, SHADOW ? fmin(rt, t_stop) : rt, wl, wh);
                uint32_t pass = 0u;
                for (uint32_t b = 0; b < lim; b += RPT_GBOX_BATCH) {
                  PROF_COUNT(PF_TT_BOX);
                  LeafBox w[RPT_GBOX_BATCH];
#pragma unroll
                  for (uint32_t k = 0; k < RPT_GBOX_BATCH; k++) w[k] = boxes0[lf_first + lf_base + b + k]; // (unclamped, as in kd_leaf)
                  uint32_t p = 0u;
#pragma unroll
                  for (uint32_t k = 0; k < RPT_GBOX_BATCH; k++) p |= (leaf_box_pass(w[k], br, wl, wh) ? 1u : 0u) << k;
                  pass |= p << b;
                }
                m &= pass;
              }
              lf_mask = m;
              continue;
            }
            const uint32_t i = (uint32_t)__ffs((int)lf_mask) - 1u;
            lf_mask &= lf_mask - 1u;
            const Inst* __restrict__ c = kids + refs0[lf_first + lf_base + i];
            const int32_t kind = c->kind;
            bool h = false;
            if (kind == RPT_SHAPE_MESH) {
              const Tree& t1 = sc.trees[c->tree];
              {
                D3 lo = o, ld = d;
                if (c->has_xf) { // Ray::apply_transform shape.rs:64-71
                  lo = mat4_mul(c->inv, o, 1.0);
                  ld = mat4_mul(c->inv, d, 0.0);
                }
                double bn, bx;
                slab_fold(slab_quotients(t1, lo, ld), bn, bx);
                if (!(fmax(bn, t_min) > fmin(bx, rt))) { // kdtree.rs:130-134: walk this child
                  inner = true;
                  entered = true;
                  child = c;
                  ct.ref_base = t1.ref_base; ct.prim_base = t1.prim_base;
                  br = boxray_make<false>(t1, lo, ld, fmax(bn, 0.0));
                  if (!sc.use_leaf_boxes) br.on = false;
                  o = lo; d = ld;
                  b_min = bn; b_max = bx;
                  nodes = sc.nodes + t1.node_base;
                  t_min_leaf = t_min;
                  sp_in = sp;
                  node = 0;
                }
              }
            } else { // a sphere, a cube, a monomial surface (no group children here: the host sees to it)
              const ChildM cur = ld_child(c);
              h = isect_child(cur, c, o, d, t_min, rt, rn, !SHADOW);
            }
            found = found || h;
            if (SHADOW && rt <= t_stop) { finished = true; break; }
          }
          if (!finished && !entered) { // the group's leaf is exhausted
            in_leaf = false;
            finished = !stack_pop(lds, cols, sp, 0, rt, node, b_min, b_max, t_min);
          }
        }
        PROF_PHASE(PF_TT_POP);
        if (finished) {
          if (bail) { // rpt_tree_generic starts the ray over in the general form; nothing of it is written here
            fq[atomicAdd(fq_count, 1u)] = slot;
            found = false;
          }
          fin = found;
          active = false;
        }
      }
      if (round_over(active, exhausted)) break;
    }
  }
  PROF_FLUSH();
}
// (one launch for the tree's queue and the queue of its rays with a zero direction component, like rpt_tree_trace; the
// node step here is the general compact one, so both run the same code)
template <bool SHADOW>
__global__ void __launch_bounds__(256, RPT_TT_WAVES) rpt_nest_trace(Scene sc, RayBatch rb, int obj_index,
                                                                    const uint32_t* __restrict__ queue,
                                                                    const uint32_t* __restrict__ tq,
                                                                    const uint32_t* __restrict__ zq,
                                                                    uint32_t* __restrict__ ctr,
                                                                    uint32_t* __restrict__ fq, StackSpill spill) {
  __shared__ KdLdsTT lds;
  for (int pass = 0; pass < 2; pass++) { // (a loop, not two inlined copies: the passes are the same code)
    if (ctr[2 * pass] != 0u) nest_trace_body<SHADOW>(lds, sc, rb, obj_index, queue, pass ? zq : tq, ctr + 2 * pass, ctr + 2 * pass + 1, fq, ctr + 4, spill);
  }
}
#endif
