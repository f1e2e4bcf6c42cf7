// kernels/tree_generic.inc — the per-tree query's general walker: generic_walk and its kernel, rpt_tree_generic.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ rpt_tree_generic: KdTree::intersect, whatever the tree
// The per-tree pipeline's kernel of last resort, and the only place where a tree inside a tree is walked to ANY depth.
// It takes (i) the rays the fast kernels hand on — a 0/0 split (rpt_tree_trace<ZEROS>, rpt_nest_trace), every ray of an
// irregular tree or under RPT_FLAG_GENERAL_TRAVERSAL — and (ii) every ray of an object the fast kernels are not built
// for (Tree::generic_only): a group with a group among its children, to any nesting depth (kdtree.rs:14-24 forwards
// Bounded through Box without limit), a group whose mesh children do not qualify for rpt_nest_trace, a tree deeper than
// KD_MAX_STACK.  One loop, no calls, nothing private: the reference's recursion (kdtree.rs:129-223 inside
// Transformed::intersect shape.rs:128-137 inside the leaf loop kdtree.rs:162-171 ...) with its two kinds of pending work
// kept in global memory, one column per thread of this kernel's (persistent, bounded) grid —
//   deferred far children  [level][8][thread]: the six carried face parameters, t_split, the node   (the general,
//                          box-carrying form: exact for irregular trees and NaN splits, kd_intersect_general)
//   suspended leaves       [frame][12][thread]: a group's leaf loop interrupted by a tree child — the group's ray and
//                          t_min, where in which leaf to go on, its part of the deferred stack, its `result` so far
// — so the nesting depth and the tree depth are bounded by what api_render.cpp allocates for the scene (it knows both), not by
// a template level or a frame in scratch.  Speed is not the point here (no LDS, no box filter): the scenes that need it
// are rare, the rays handed on a handful.  Per ray: the reference's tests in the reference's order on the one record.
// (GenericStack: kernels.h)
// returns KdTree::intersect's result for tree `root` (tris: a Mesh's tree) and the ray (o, d) in ITS space; *overflow is
// set — and false returned — if the scene outgrew the columns (api_render.cpp sizes them from the scene: cannot happen)
template <bool SHADOW>
RPT_DEV bool generic_walk(const Scene& sc, uint32_t root, bool root_tris, D3 o, D3 d, double t_min, const double t_stop,
                          double& rt, D3& rn, const GenericStack& gs, const uint32_t tid, uint32_t* overflow) {
  const uint64_t T = gs.threads;
  double* __restrict__ dcol = gs.defer + tid;
  double* __restrict__ fcol = gs.frame + tid;
  uint32_t tidx = root, sp = 0, sp_base = 0, depth = 0;
  bool tris = root_tris, found = false, result = false;
  uint32_t node = 0, lf_first = 0, lf_cnt = 0, lf_i = 0;
  Slab face{}; // the six face parameters of the cell the walk is in (slab_quotients at the root, t_split on the way down)
  enum { ENTER, DESCEND, LEAF, POP, RETURN };
  int mode = ENTER;
  for (;;) {
    const Tree& tr = sc.trees[tidx];
    if (mode == ENTER) { // KdTree::intersect kdtree.rs:129-135
      face = slab_quotients(tr, o, d);
      double b_min, b_max;
      slab_fold(face, b_min, b_max);
      if (fmax(b_min, t_min) > fmin(b_max, rt)) { result = false; mode = RETURN; }
      else { node = 0; found = false; sp_base = sp; mode = DESCEND; }
    }
    if (mode == DESCEND) { // intersect_subtree kdtree.rs:151-223, the far child deferred with its own box
      const KdNode* __restrict__ nodes = sc.nodes + tr.node_base;
      KdNode n = nodes[node];
      uint32_t axis = n.ib & 3u;
      while (axis != 3u) {
        const double value = n.split;
        const double o_ax = sel((int)axis, o), d_ax = sel((int)axis, d);
        const double ts = (value - o_ax) / d_ax;
        const bool left_first = (o_ax < value) || (o_ax == value && d_ax <= 0.0);
        double b_min, b_max;
        slab_fold(face, b_min, b_max);
        const bool only_first = (ts > fmin(b_max, rt)) || (ts <= 0.0);     // kdtree.rs:207
        const bool only_second = !only_first && (ts < fmax(b_min, t_min)); // kdtree.rs:209
        const bool go_left = only_second ? !left_first : left_first;
        if (!only_first && !only_second) {
          if (sp >= gs.levels) { *overflow = 1u; return false; }
          const bool sec_left = !left_first;
          double* e = dcol + (uint64_t)sp * 8u * T;
          e[0] = (!sec_left && axis == 0) ? ts : face.fax;
          e[T] = (!sec_left && axis == 1) ? ts : face.fay;
          e[2 * T] = (!sec_left && axis == 2) ? ts : face.faz;
          e[3 * T] = (sec_left && axis == 0) ? ts : face.fbx;
          e[4 * T] = (sec_left && axis == 1) ? ts : face.fby;
          e[5 * T] = (sec_left && axis == 2) ? ts : face.fbz;
          e[6 * T] = ts;
          e[7 * T] = pack_u32(n.a + (sec_left ? 0u : 1u), 0u);
          sp++;
        }
        if (go_left) {
          face.fbx = axis == 0 ? ts : face.fbx; face.fby = axis == 1 ? ts : face.fby; face.fbz = axis == 2 ? ts : face.fbz;
        } else {
          face.fax = axis == 0 ? ts : face.fax; face.fay = axis == 1 ? ts : face.fay; face.faz = axis == 2 ? ts : face.faz;
        }
        node = n.a + (go_left ? 0u : 1u);
        n = nodes[node];
        axis = n.ib & 3u;
      }
      lf_first = n.a; lf_cnt = n.ib >> 2; lf_i = 0;
      mode = LEAF;
    }
    if (mode == LEAF) { // kdtree.rs:162-171: every object of the leaf, in order, on the one record
      const uint32_t* __restrict__ refs = sc.refs + tr.ref_base;
      if (tris) {
        const TriX* __restrict__ recs = sc.lrec + tr.ref_base + lf_first;
        const Tri* __restrict__ tp = sc.tris + tr.prim_base;
        for (uint32_t b = 0; b < lf_cnt; b += 4) {
          const bool h = tri_batch<SHADOW>(recs + b, tp, refs + lf_first + b, lf_cnt - b, lf_cnt <= 2, o, d, t_min, rt, rn);
          found = found || h;
          if (SHADOW && rt <= t_stop) return true;
        }
        mode = POP;
      } else {
        const Inst* __restrict__ kids = sc.insts + tr.prim_base;
        mode = POP;
        while (lf_i < lf_cnt) {
          const Inst* __restrict__ c = kids + refs[lf_first + lf_i];
          lf_i++;
          const ChildM cur = ld_child(c);
          if (cur.kind == RPT_SHAPE_MESH || cur.kind == RPT_SHAPE_GROUP) {
            // Transformed<KdTree<..>>::intersect (shape.rs:128-137): suspend this leaf, walk the child's tree with the
            // ray in the child's space and the same t_min
            if (depth >= gs.frames) { *overflow = 1u; return false; }
            double* f = fcol + (uint64_t)depth * 12u * T;
            f[0] = o.x; f[T] = o.y; f[2 * T] = o.z; f[3 * T] = d.x; f[4 * T] = d.y; f[5 * T] = d.z;
            f[6 * T] = t_min;
            f[7 * T] = pack_u32(tidx, (uint32_t)(c - sc.insts));
            f[8 * T] = pack_u32(lf_first, lf_cnt);
            f[9 * T] = pack_u32(lf_i, sp_base);
            f[10 * T] = pack_u32(found ? 1u : 0u, 0u);
            depth++;
            if (c->has_xf) { // Ray::apply_transform shape.rs:64-71
              const D3 lo = mat4_mul(c->inv, o, 1.0), ld = mat4_mul(c->inv, d, 0.0);
              o = lo; d = ld;
            }
            tidx = (uint32_t)c->tree;
            tris = cur.kind == RPT_SHAPE_MESH;
            mode = ENTER;
            break;
          }
          const bool h = isect_child(cur, c, o, d, t_min, rt, rn, !SHADOW);
          found = found || h;
          if (SHADOW && rt <= t_stop) return true;
        }
      }
    }
    if (mode == POP) { // the nearest deferred far child of THIS tree that can still matter (kdtree.rs:213-220)
      mode = RETURN;
      result = found;
      while (sp > sp_base) {
        sp--;
        const double* e = dcol + (uint64_t)sp * 8u * T;
        const double ts = e[6 * T];
        if (rt < ts) continue;
        face.fax = e[0]; face.fay = e[T]; face.faz = e[2 * T]; face.fbx = e[3 * T]; face.fby = e[4 * T]; face.fbz = e[5 * T];
        uint32_t nd, unused;
        unpack_u32(e[7 * T], nd, unused);
        node = nd;
        t_min = ts;
        mode = DESCEND;
        break;
      }
    }
    if (mode == RETURN) { // this tree's intersect returns `result`
      if (depth == 0) return result;
      depth--;
      const double* f = fcol + (uint64_t)depth * 12u * T;
      uint32_t ci, fnd, unused;
      o = mk(f[0], f[T], f[2 * T]); d = mk(f[3 * T], f[4 * T], f[5 * T]);
      t_min = f[6 * T];
      unpack_u32(f[7 * T], tidx, ci);
      unpack_u32(f[8 * T], lf_first, lf_cnt);
      unpack_u32(f[9 * T], lf_i, sp_base);
      unpack_u32(f[10 * T], fnd, unused);
      const Inst* __restrict__ c = sc.insts + ci;
      if (result && !SHADOW && c->has_xf) rn = normalize(mat3_mul(c->nrm, rn)); // shape.rs:131-132
      found = fnd != 0u || result;
      tris = false; // (only a group's leaf is ever suspended)
      mode = LEAF;
    }
  }
}
template <bool SHADOW>
__global__ void __launch_bounds__(256) rpt_tree_generic(Scene sc, RayBatch rb, int obj_index, const uint32_t* __restrict__ fq,
                                                        const uint32_t* __restrict__ fq_count, GenericStack gs,
                                                        uint32_t* __restrict__ overflow, uint32_t* __restrict__ zero_next) {
  // the counters of the NEXT (tree, query) pair — the other of two sets (launch_query): this kernel is the last
  // launch of every pair, and the set it clears was last used by the pair before.  One memset per pair less.
  if (zero_next && blockIdx.x == 0 && threadIdx.x < 5u) zero_next[threadIdx.x] = 0u;
  const uint32_t count = *fq_count;
  CInst& in = cinst(sc, obj_index);
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= gs.threads) return; // (the grid never exceeds the columns: api_render.cpp / launch_query)
  for (uint32_t i = tid; i < count; i += gridDim.x * blockDim.x) {
    const uint32_t slot = fq[i];
    D3 o = ld_soa3(rb.o, rb.o_stride, slot), d = ld_soa3(rb.d, rb.d_stride, slot);
    if (in.has_xf) {
      D3 lo = mat4_mul(in.inv, o, 1.0), ld = mat4_mul(in.inv, d, 0.0);
      o = lo; d = ld;
    }
    double rt = rb.rt[slot], t_stop;
    if (shadow_stop<SHADOW>(SHADOW ? rb.dist[slot] : 0.0, rt, t_stop)) continue; // already occluded by an earlier object
    D3 rn = mk(0, 0, 0);
    const bool hit = generic_walk<SHADOW>(sc, (uint32_t)in.tree, in.kind == RPT_SHAPE_MESH, o, d, EPSILON, t_stop, rt, rn, gs, tid, overflow);
    if (hit) hit_epilogue<SHADOW>(rb, in, obj_index, slot, rt, rn);
  }
}
