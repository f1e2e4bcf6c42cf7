// kernels/hit_surface.inc — rptgpu_hit_surface's resolve pass (include/rpt_gpu_hit_surface.h, DESIGN.md §21): which triangle,
// which barycentrics and which child of a group stand behind a first hit.  The first-hit query has run (rptgpu_first_hits'
// own, unchanged) and left t_i and obj_i per ray; rpt_hit_surface walks object obj_i ALONE, in the reference's order, with the
// record starting at the next double above t_i, and a sink remembers every accept: the leaf entry (refs[] gives the caller's
// index), the (u, v, w) of mesh.rs:71-73, the top-level group's child.  The last accept is the record that stands.
// The walk is generic_walk's (tree_generic.inc) restated with that sink and without normals: the reference's recursion for any
// tree of trees at any depth, its pending work in global columns sized from the scene (surface_plan.h).  The walkers of the
// renders are not touched: they are register-bound, and their code objects stay what they were.
// Compiled in translation units of its own (kernels_surface_strict[_ext].hip, RPT_SURFACE_TU; inside namespace RPT_NS).

// RPT_SURFACE_FROM_INF=1: the walk starts from record.time = +inf, as the original did (A/B builds: what the cut is worth)
#ifndef RPT_SURFACE_FROM_INF
#define RPT_SURFACE_FROM_INF 0
#endif

// the next double above t (t is a hit's time: not NaN; +inf stays +inf)
RPT_DEV double next_above(double t) {
  if (t == 0.0) return __longlong_as_double(1ll); // (either zero)
  if (!(t < INF)) return t;
  const long long b = __double_as_longlong(t);
  return __longlong_as_double(t > 0.0 ? b + 1 : b - 1);
}

struct SurfaceSink {
  int32_t child, primitive;
  double u, v, w;
};

// Triangle::intersect (mesh.rs:49-82) of the leaf's entries in order on the one record — tri_plane, tri_accept's guards and
// tri_bary, the expressions every walker's accept uses —, the accepted entry and its weights into the sink
RPT_DEV bool surface_tri_leaf(const TriX* __restrict__ recs, const uint32_t* __restrict__ refp, uint32_t cnt, D3 o, D3 d,
                              double t_min, double& rt, int32_t top_child, SurfaceSink& sink) {
  bool found = false;
  for (uint32_t j = 0; j < cnt; j++) {
    const TriX* __restrict__ tx = recs + j;
    const TriPlane pl = tri_plane(tx, o, d);
    if ((fabs(pl.cosine) < 1e-8) | (pl.time < t_min) | (pl.time >= rt)) continue; // mesh.rs:53-58
    const TriBary b = tri_bary(tx, pl, o, d);
    if ((b.u >= 0.0) & (b.v >= 0.0) & (b.w >= 0.0)) {
      rt = pl.time;
      found = true;
      sink.child = top_child;
      sink.primitive = (int32_t)refp[j];
      sink.u = b.u; sink.v = b.v; sink.w = b.w;
    }
  }
  return found;
}

// KdTree::intersect of tree `root` (tris: a Mesh's tree) for the ray (o, d) in ITS space on the record rt: generic_walk's
// loop — ENTER kdtree.rs:129-135, DESCEND :151-223 with the far child deferred with its own box, LEAF :162-171, POP :213-220,
// RETURN through Transformed::intersect shape.rs:128-137 — with every accept noted in `sink`.  *overflow is set, and the walk
// ends, if the scene outgrew the columns (the host sizes them from the scene: cannot happen)
RPT_DEV void surface_walk(const Scene& sc, uint32_t root, bool root_tris, D3 o, D3 d, double t_min, double& rt,
                          const GenericStack& gs, const uint32_t tid, uint32_t* overflow, SurfaceSink& sink) {
  const uint64_t T = gs.threads;
  double* __restrict__ dcol = gs.defer + tid;
  double* __restrict__ fcol = gs.frame + tid;
  uint32_t tidx = root, sp = 0, sp_base = 0, depth = 0;
  bool tris = root_tris, found = false, result = false;
  uint32_t node = 0, lf_first = 0, lf_cnt = 0, lf_i = 0;
  int32_t top_child = -1; // the child of the ROOT group the walk is in or below
  D3 rn = mk(0, 0, 0);    // (isect_child's; not asked for)
  Slab face{};
  enum { ENTER, DESCEND, LEAF, POP, RETURN };
  int mode = ENTER;
  for (;;) {
    const Tree& tr = sc.trees[tidx];
    if (mode == ENTER) {
      face = slab_quotients(tr, o, d);
      double b_min, b_max;
      slab_fold(face, b_min, b_max);
      if (fmax(b_min, t_min) > fmin(b_max, rt)) { result = false; mode = RETURN; }
      else { node = 0; found = false; sp_base = sp; mode = DESCEND; }
    }
    if (mode == DESCEND) {
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
          if (sp >= gs.levels) { *overflow = 1u; return; }
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
    if (mode == LEAF) { // every object of the leaf, in order, on the one record
      const uint32_t* __restrict__ refs = sc.refs + tr.ref_base;
      if (tris) {
        const bool h = surface_tri_leaf(sc.lrec + tr.ref_base + lf_first, refs + lf_first, lf_cnt, o, d, t_min, rt, top_child, sink);
        found = found || h;
        mode = POP;
      } else {
        const Inst* __restrict__ kids = sc.insts + tr.prim_base;
        mode = POP;
        while (lf_i < lf_cnt) {
          const uint32_t k = refs[lf_first + lf_i];
          const Inst* __restrict__ c = kids + k;
          lf_i++;
          if (depth == 0u) top_child = (int32_t)k;
          const ChildM cur = ld_child(c);
          if (cur.kind == RPT_SHAPE_MESH || cur.kind == RPT_SHAPE_GROUP) { // suspend this leaf, walk the child's tree
            if (depth >= gs.frames) { *overflow = 1u; return; }
            double* f = fcol + (uint64_t)depth * 12u * T;
            f[0] = o.x; f[T] = o.y; f[2 * T] = o.z; f[3 * T] = d.x; f[4 * T] = d.y; f[5 * T] = d.z;
            f[6 * T] = t_min;
            f[7 * T] = pack_u32(tidx, 0u);
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
          if (isect_child(cur, c, o, d, t_min, rt, rn, false)) { // a sphere, a cube, a monomial surface: no triangle
            found = true;
            sink.child = top_child;
            sink.primitive = -1;
            sink.u = 0.0; sink.v = 0.0; sink.w = 0.0;
          }
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
      if (depth == 0) return;
      depth--;
      const double* f = fcol + (uint64_t)depth * 12u * T;
      uint32_t fnd, unused;
      o = mk(f[0], f[T], f[2 * T]); d = mk(f[3 * T], f[4 * T], f[5 * T]);
      t_min = f[6 * T];
      unpack_u32(f[7 * T], tidx, unused);
      unpack_u32(f[8 * T], lf_first, lf_cnt);
      unpack_u32(f[9 * T], lf_i, sp_base);
      unpack_u32(f[10 * T], fnd, unused);
      found = fnd != 0u || result;
      tris = false; // (only a group's leaf is ever suspended)
      mode = LEAF;
    }
  }
}

// One lane per ray of the piece (origins, dirs: [n][3] f64, already offset to it), in strides of the grid: a thread owns one
// column of gs, and the grid never exceeds the columns.  Rays without a hit, with a NaN time or on an object that is neither
// a mesh nor a group skip the walk.  The channel mask is a kernel argument (wave-uniform), as in hit_store
__global__ void __launch_bounds__(256) rpt_hit_surface(Scene sc, const double* __restrict__ origins, const double* __restrict__ dirs,
                                                       uint32_t n, SurfaceOut out, GenericStack gs, uint32_t groups_from_inf,
                                                       uint32_t* __restrict__ overflow) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= gs.threads) return;
  const uint32_t ch = out.channels;
  for (uint32_t i = tid; i < n; i += gridDim.x * blockDim.x) {
    const double t = out.t[i];
    const int obj = out.object[i];
    SurfaceSink sink{-1, -1, 0.0, 0.0, 0.0};
    if (obj >= 0 && obj < sc.num_objects && t == t) {
      const Inst* __restrict__ in = sc.insts + obj;
      const int kind = in->kind;
      if (kind == RPT_SHAPE_MESH || kind == RPT_SHAPE_GROUP) {
        D3 o = ld3(origins + 3 * (uint64_t)i), d = ld3(dirs + 3 * (uint64_t)i);
        if (in->has_xf) {
          const D3 lo = mat4_mul(in->inv, o, 1.0), ld = mat4_mul(in->inv, d, 0.0);
          o = lo; d = ld;
        }
        double rt = next_above(t);
#if RPT_SURFACE_FROM_INF
        rt = INF;
#endif
        // MonomialSurface::intersect rejects `r > record.time` (monomial_surface.rs:132), not `time >= record.time`: the cut's
        // argument does not hold for a group that may hold one, so in a scene with such a child (groups_from_inf: the host
        // knows the children's kinds) a group's walk starts where the original did
        if (groups_from_inf && kind == RPT_SHAPE_GROUP) rt = INF;
        surface_walk(sc, (uint32_t)in->tree, kind == RPT_SHAPE_MESH, o, d, EPSILON, rt, gs, tid, overflow, sink);
      }
    }
    if (ch & RPT_SURFACE_CHILD) out.child[i] = sink.child;
    if (ch & RPT_SURFACE_PRIMITIVE) out.primitive[i] = sink.primitive;
    if (ch & RPT_SURFACE_BARYCENTRIC) {
      const uint64_t i3 = 3ull * i;
      out.barycentric[i3] = sink.u; out.barycentric[i3 + 1] = sink.v; out.barycentric[i3 + 2] = sink.w;
    }
  }
}

#ifndef __HIP_DEVICE_COMPILE__
void launch_hit_surface(hipStream_t st, const Scene& sc, const double* origins, const double* dirs, uint32_t n,
                        const SurfaceOut& out, const GenericStack& gs, bool groups_from_inf, uint32_t* overflow, uint32_t blocks) {
  hipLaunchKernelGGL(rpt_hit_surface, dim3(blocks), dim3(256), 0, st, sc, origins, dirs, n, out, gs, groups_from_inf ? 1u : 0u, overflow);
}
#endif
