// scene_plan.h — what rptgpu_scene_create_opts decides between "flatten the scene" and "upload it", as pure host functions
// of numbers (tests/cpp/scene_plan_check.cpp): the route of every top-level object and the scene's flags that follow
// (route_object, fold_routes), the same decision again after a live update rebuilt a tree (reroute_object,
// rebuilt_too_deep), and the whole dynamic-LDS layout of the flat path kernel (plan_flat).  Creation (api_scene.cpp) and
// the live updates (api_scene.cpp commit_update, tree_splice.h) apply the results to the handle; free of HIP.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rpt_gpu.h"
#include "device_types.h"
#include "flat_layout.h"
#include "launch_limits.h"

namespace rptscene {

// ---- routing: which pipeline and which traversal kernel walk a top-level object

// what the routing reads of one top-level object and its tree (the tree fields: MESH and GROUP only)
struct ObjectFacts {
  int32_t kind = 0;         // RPT_SHAPE_*
  uint32_t depth = 0;       // depth of the tree's deepest leaf
  uint32_t tree_kids = 0;   // GROUP: bit 0 a child is a MESH, bit 1 a GROUP sits somewhere below it (FlatScene::tree_kids)
  bool regular = true;      // Tree::regular
  bool root_leaf = false;   // Tree::root_leaf != 0
  uint64_t bytes = 0;       // the tree's nodes + leaf entries (+ leaf records of a mesh)
  uint32_t kids_depth = 0;  // a group with mesh children: the deepest of their trees ...
  bool kids_regular = true; // ... and whether all of them are regular
};
struct ObjectRoute {
  uint8_t deep = 0, tris = 0; // the route bytes (launch_limits.h)
  bool generic_only = false;  // -> Tree::generic_only
  // the object's contribution to the scene's flags (fold_routes)
  bool has_deep = false, tree_kids = false, sort_rays = false, gen_all = false;
};

inline ObjectRoute route_object(const ObjectFacts& f, const RptSceneOptions& opt) {
  ObjectRoute r;
  const bool tree = f.kind == RPT_SHAPE_MESH || f.kind == RPT_SHAPE_GROUP;
  bool deep = tree && f.depth >= opt.deep_depth;
  // A group with TREE children (meshes: fractal_teapots.rs; groups: kdtree.rs:14-24 nests without limit) goes through
  // the per-tree kernels whatever its own depth — they are the only ones that walk a tree inside a tree: rpt_nest_trace
  // (two regular levels, one loop) or rpt_tree_generic (anything).  So does a tree deeper than the fast stacks.
  const bool kids = f.kind == RPT_SHAPE_GROUP && f.tree_kids != 0;
  // deeper than the private stacks of the in-kernel traversals (KD_MAX_STACK): the per-tree kernels, whose stack
  // beyond the LDS levels is a global column as high as the scene's deepest tree (ensure_workspace).
  // RPTGPU_FAST_MAX_DEPTH (tests): treat trees deeper than this as too deep for the in-kernel traversals.  The build rule
  // itself keeps real trees far below 32: both children of a median split hold (n + straddlers) / 2 primitives, so a path
  // d levels long needs 16 / 0.85^d primitives with an unsplittable sibling at every level, or 16 * 2^d balanced ones.
  const bool too_deep = tree && f.depth > opt.fast_max_depth;
  deep = deep || kids || too_deep;
  r.tree_kids = kids || too_deep; // (= the object is for the per-tree pipeline only)
  // rays entering a large tree are sorted by entry cell and octant first: neighbours in a wave then walk the same
  // nodes.  Measured with the VALU-bound traversal kernel of round 2: 100k-triangle mesh (66 MB of nodes + leaf
  // records) 144 -> 172 Msamples/s, 16k-triangle glass (17 MB) 469 -> 528, a 25k-triangle mesh under few bounces
  // (25 MB) 781 -> 766, two 768-triangle meshes (0.6 MB) 4243 -> 3248: the sort sorts EVERY ray of the depth, the
  // gain grows with the work of the rays that enter — so by size, with the threshold well below the glass
  bool sort = false, sort_shadow = false;
  if (deep) {
    sort = opt.sort_rays == 1 || (opt.sort_rays < 0 && f.bytes >= opt.sort_min_bytes);
    // shadow rays point at ONE light from surfaces that the closest-hit pass just visited in sorted order: for a tree
    // that is not many times the L2s their sort costs more than it gives (16k-triangle glass, ~10 MB: shadow stage
    // 47.7 -> 42.8 ms per two steps without it; 100k-triangle mesh, ~60 MB: 137 -> 180)
    sort_shadow = sort && (opt.sort_rays == 1 || f.bytes >= opt.sort_shadow_min_bytes);
  }
  uint8_t trace_kind = f.kind == RPT_SHAPE_MESH ? RPT_TRACE_MESH : RPT_TRACE_GROUP;
  if (kids) {
    const bool ok = f.regular && !(f.tree_kids & 2u) && f.kids_regular; // rpt_nest_trace: no group children, no irregular trees
    if (ok && opt.nest_trace != 0 && f.depth + f.kids_depth + 2 <= (uint32_t)rptdev::KD_MAX_STACK) trace_kind = RPT_TRACE_NEST;
    else r.generic_only = true;
  }
  if (r.generic_only) {
    trace_kind = RPT_TRACE_GENERIC;
    sort = false;
    sort_shadow = false;
  }
  r.sort_rays = sort;
  r.gen_all = deep && (r.generic_only || !f.regular);
  r.deep = deep ? (uint8_t)((sort ? RPT_DEEP_SORTED : RPT_DEEP_PER_TREE) | (r.gen_all ? RPT_DEEP_ALL_GENERIC : 0) |
                            (sort && !sort_shadow ? RPT_DEEP_SORT_CLOSEST : 0))
                : 0;
  const bool one_leaf = !tree || f.root_leaf;
  r.tris = (uint8_t)(trace_kind | (!deep && one_leaf ? RPT_TRIS_ONE_LEAF : 0));
  r.has_deep = deep;
  return r;
}

// the scene's flags: the objects' contributions folded, and what follows from them before the flat layout is tried
struct SceneRoute {
  bool has_deep = false, tree_kids = false, sort_rays = false, gen_all = false;
  bool prefer_wavefront = false; // the scene has real kd-trees (traversal-latency bound), or only the per-tree pipeline walks it
  bool path_reorder = false;
  bool all_flat = false;         // every tree is a single leaf: plan_flat says whether the scene also fits the LDS tables
};
// max_tree_depth, scene_bounds_ok: FlatScene's; n_trees, all_root_leaf: how many trees, and whether each is one leaf;
// reorder_switch: RPTGPU_PATH_REORDER (an A/B switch, environment only — scheduling, not results; unset = true)
inline SceneRoute fold_routes(const std::vector<ObjectRoute>& routes, uint32_t max_tree_depth, bool scene_bounds_ok, size_t n_trees,
                              bool all_root_leaf, bool reorder_switch) {
  SceneRoute s;
  for (const ObjectRoute& r : routes) {
    s.has_deep = s.has_deep || r.has_deep;
    s.tree_kids = s.tree_kids || r.tree_kids;
    s.sort_rays = s.sort_rays || r.sort_rays;
    s.gen_all = s.gen_all || r.gen_all;
  }
  s.prefer_wavefront = max_tree_depth >= 3 || s.tree_kids;
  // scenes whose trees are all walked inside rpt_extend / rpt_shadow_rays get their paths re-ordered per depth
  s.path_reorder = !s.has_deep && scene_bounds_ok && n_trees != 0 && reorder_switch;
  s.all_flat = all_root_leaf;
  if (s.all_flat) s.path_reorder = false; // every tree a single leaf: nothing in rpt_extend diverges by where a ray goes
  return s;
}

// ---- the same decision after a live update rebuilt the tree of an object (tree_splice.h applies it after the swap)

// What the routing took from the tree at creation.  A per-tree object: the all-generic bit of obj_deep follows `regular`
// (gen_all sizes a grid and only grows), and a tree beyond fast_max_depth is for the per-tree pipeline only.  An object
// walked inside the path kernels: the single-leaf bit of obj_tris follows root_leaf (the lean build of rpt_rays_objects
// takes single leaves only)
struct Reroute {
  uint8_t deep, tris;
  bool gen_all, tree_kids; // the scene's flag rises (neither ever falls)
};
inline Reroute reroute_object(uint8_t deep, uint8_t tris, bool regular, bool root_leaf, uint32_t depth, uint32_t fast_max_depth) {
  Reroute r{deep, tris, false, false};
  if (deep) {
    r.deep = (uint8_t)((deep & ~RPT_DEEP_ALL_GENERIC) | (regular ? 0 : RPT_DEEP_ALL_GENERIC)); // an irregular tree: every ray through rpt_tree_generic
    r.gen_all = !regular;
    r.tree_kids = depth > fast_max_depth; // only the per-tree pipeline walks it
  } else {
    r.tris = (uint8_t)((tris & ~RPT_TRIS_ONE_LEAF) | (root_leaf ? RPT_TRIS_ONE_LEAF : 0));
  }
  return r;
}
// the live updates' depth refusal: an object the handle walks inside the path kernels keeps that route, and their stacks
// hold fast_max_depth levels
inline bool rebuilt_too_deep(uint8_t deep, uint32_t depth, uint32_t fast_max_depth) { return !deep && depth > fast_max_depth; }

// ---- the flat path kernel's dynamic LDS

// all n top-level objects as a mask (the filter and the cull take the first 64)
inline uint64_t every_object(size_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }
// bit i: top-level object i is a user of the flat kernel's plane table (plane_use(i) != 0; the first 64 count)
template <class Use> uint64_t plane_users(size_t n, Use plane_use) {
  uint64_t m = 0;
  for (size_t i = 0; i < n && i < 64; i++)
    if (plane_use(i)) m |= 1ull << i;
  return m;
}
// The fused kernel's pre-trace pass skips, per wave, objects whose screen rectangle holds none of its pending pixels
// (kernels/paths_flat.inc cull_skip_mask; the rectangles are the render's: api_render.cpp).  Never skipped: the plane
// table's users (their slab run is cheap) and what the object filter exempts (ObjectBounds::obj_always, host_scene.cpp
// fill_object_boxes: unbounded, not finite, sliver meshes, ill-conditioned placements)
inline uint64_t cull_always(uint64_t obj_always, uint64_t users, size_t n) { return (obj_always | users) & every_object(n); }

// ---- axis-flat meshes: the shadow ray's window in the two-ray query (RPT_SHADOW_WINDOW, kernels/paths_flat.inc flat_query2)
//
// An object is AXIS-FLAT when all of this holds, bit for bit:
//   (1) it is an untransformed mesh whose tree is a single leaf, and `recs` are all n >= 1 of that leaf's records;
//   (2) on one axis k, bounds[k] and bounds[3 + k] are the same finite double c;
//   (3) every record has v1[k] == c (the same bits), pn zero (either sign) on the two other axes, pn[k] finite with
//       2^-100 <= |pn[k]| <= 2^100, and v1 finite on all three axes.
// What follows for a ray (o, d), with a = fl(c - o_k), q = fl(a / d_k) the plane table's quotient of the object's slab on
// axis k, and Triangle::intersect's time = fl(dot(pn, v1 - o) / dot(pn, d)) (kernels/shapes.inc tri_plane, built with
// -ffp-contract=off, mesh.rs:50-58):
//   * both dot products add two zero products to the axis' own: time = fl(fl(pn_k * a) / fl(pn_k * d_k)).  (A product
//     0 * x is a zero unless x is infinite or NaN; then time is NaN and the test accepts nothing.)
//   * an ACCEPT needs |fl(pn_k * d_k)| >= 1e-8 and time >= EPSILON (shapes.inc tri_accept).  With neither product
//     overflowing or underflowing, time and q are the exact a / d_k under three and one roundings: time >= q * (1 - u)^2
//     / (1 + u)^2 > q * (1 - 2^-50) for q > 0, u = 2^-53.  fl(pn_k * a) underflows: |time| < 2^-1022 / 1e-8 < EPSILON, no
//     accept.  fl(pn_k * d_k) underflows: below 1e-8, no accept; it overflows: time is a zero, no accept.  fl(pn_k * a)
//     overflows: time is infinite, and `time >= rt` rejects +inf as `time < t_min` does -inf.  q overflows to +inf where
//     time does not: then time > DBL_MAX * (1 - 2^-50), and the rule below drops the candidate only if t_stop lies more
//     than 2^13 doubles below +inf, that is t_stop <= DBL_MAX * (1 - 2^-41) < time.
//   * a slab candidate of such an object has b_min == b_max == q (run_slabs: the window is inside [q, q] and not empty), so
//     its mm = max(q, EPSILON), and every time the object's leaf can accept has  time >= mm * (1 - 2^-50):  for
//     q <= EPSILON that is time >= EPSILON.  (q NaN, 0 / 0: time is NaN as well, nothing is accepted.)
// The rule (flat_query2): the shadow ray drops a candidate of an axis-flat object when mm lies more than 2^13 doubles above
// t_stop (flat_layout.h rpt_shadow_window_beyond, which says why that implies  mm > t_stop * (1 + 2^-40)  for every t_stop
// but a NaN).  Then every time it could accept is > t_stop * (1 + 2^-40) * (1 - 2^-50) > t_stop: the object could only set
// rts to a value above t_stop.  That changes nothing the query returns, which is `rts > t_stop` alone: an object at or
// before t_stop is accepted with or without the dropped one in front of it (an accept needs time < rts, and rts > t_stop
// either way), one beyond t_stop leaves rts > t_stop, and the early exits test rts <= t_stop.  mm is never a NaN (fmax
// with EPSILON), and under a NaN t_stop `rts > t_stop` is false whatever was dropped.  A directional light's
// t_stop = DBL_MAX has nothing 2^13 doubles above it: no drop.  A quad in the light's own plane (the light's shape where
// it is an object too) has q within a few ulp of t_stop, far inside the margin: it is never dropped, and the reference's
// behaviour at the light stays what it is.
// An object that fails any part of (1)-(3) is simply not marked, and the exact test runs as before.
inline bool axis_flat_mesh(int32_t kind, int32_t has_xf, bool single_leaf, const double bounds[6], const rptdev::TriX* recs, size_t n) {
  if (kind != RPT_SHAPE_MESH || has_xf || !single_leaf || !recs || n == 0) return false;
  auto bits = [](double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; };
  auto finite = [&](double v) { return ((bits(v) >> 52) & 0x7ffu) != 0x7ffu; };
  for (int k = 0; k < 3; k++) {
    const double c = bounds[k];
    if (bits(c) != bits(bounds[3 + k]) || !finite(c)) continue;
    bool ok = true;
    for (size_t j = 0; j < n && ok; j++) {
      const rptdev::TriX& t = recs[j];
      const double p = t.pn[k] < 0.0 ? -t.pn[k] : t.pn[k];
      ok = bits(t.v1[k]) == bits(c) && t.pn[(k + 1) % 3] == 0.0 && t.pn[(k + 2) % 3] == 0.0 && finite(t.pn[k]) &&
           p >= 0x1p-100 && p <= 0x1p100 && finite(t.v1[0]) && finite(t.v1[1]) && finite(t.v1[2]);
    }
    if (ok) return true;
  }
  return false;
}

struct FlatObject {
  int32_t kind, has_xf; // Inst's
  double bounds[6];     // MESH: Inst::bounds
  // MESH: the tree is one leaf, and its records (FlatScene::lrec from Tree::ref_base + root_first on) — what axis_flat_mesh reads
  bool single_leaf = false;
  const rptdev::TriX* recs = nullptr;
  size_t n_recs = 0;
};
struct FlatInput {
  uint64_t n_refs = 0, n_tris = 0;
  std::vector<FlatObject> objects; // the top-level objects
  size_t n_lights = 0;
  int32_t light0_kind = 0;         // with n_lights >= 1 ...
  bool light0_plain_mesh = false;  // ... light 0 is a Light::Object whose shape is an untransformed mesh ...
  uint64_t light0_tris = 0;        // ... of this many triangles
  bool obj_filter_ok = false;      // ObjectBounds's
  uint64_t obj_always = ~0ull;
  int32_t object_filter_min = 0;   // RptSceneOptions::object_filter_min
  bool tris_global = false;        // RPTGPU_FLAT_TRIS_GLOBAL is set: the triangles stay in global memory (A/B)
  bool no_plane_table = false;     // RPTGPU_NO_PLANE_TABLE is set (A/B)
};
struct FlatPlan {
  bool flat = false;     // the scene's tables fit the wave's share (else `lay` is not used; the planes and plane_idx / plane_use are)
  FlatLayout lay{};      // plane_vals, obj_box and obj_grid are the uploader's
  double planes[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // [3][4]: upload when lay.plane_cnt
  std::vector<uint32_t> plane_idx, plane_use; // per object -> Inst's (plane_use 0: not a user, Inst::plane_idx stays)
  bool upload_filter = false; // lay.obj_filter: the object filter's boxes and grid go to the device
};

// does the scene (every tree a single leaf) fit a wave's share of LDS (160 KB per CU / 8 waves), and where is what?
inline FlatPlan plan_flat(const FlatInput& in) {
  constexpr uint32_t WAVE_LDS = RPT_PATHS_WAVE_LDS - RPT_PATHS_WALKER_LDS; // the wave's share less the fold walker's state
  auto up16 = [](uint64_t v) { return (v + 15) & ~15ull; };
  const int n = (int)in.objects.size();
  FlatPlan pl;
  FlatLayout& lay = pl.lay;
  uint64_t off = 0;
  lay.n_refs = (uint32_t)in.n_refs;
  // intersection records, leaf entries and materials are what a query reads; the triangles themselves (vertex
  // normals of the hit that stands, light sampling) join them only if everything still fits — C2 does (12
  // triangles), a room of 23 polygons keeps them in global memory and is flat all the same
  auto assign = [&](bool with_tris) {
    lay.n_tris = with_tris ? (uint32_t)in.n_tris : 0u;
    off = up16(in.n_refs * sizeof(rptdev::TriX));
    lay.off_tris = (uint32_t)off; off = up16(off + (uint64_t)lay.n_tris * sizeof(rptdev::Tri));
    lay.off_refs = (uint32_t)off; off = up16(off + in.n_refs * sizeof(uint32_t));
    lay.off_mat = (uint32_t)off;  off = up16(off + (uint64_t)n * sizeof(rptdev::Material));
    lay.off_leaf = (uint32_t)off; off = up16(off + (uint64_t)n * 16);
  };
  assign(true); // (rpt_paths<KdFlat>: that instantiation also stashes camera rays in LDS)
  if (off + 12 * 64 * sizeof(double) + RPT_PATHS_STASH_MAX_LDS > WAVE_LDS || in.tris_global) assign(false); // (room for the plane table)
  // shared slab quotients: distinct plane coordinates per axis over the untransformed meshes (bitwise
  // distinct: -0.0 and 0.0 give differently signed zeros), at most 4 per axis or the feature stays off
  uint32_t cnt[3] = {0, 0, 0};
  bool planes_ok = true;
  auto slot_of = [&](int axis, double v) -> int {
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    for (uint32_t j = 0; j < cnt[axis]; j++) {
      uint64_t b2;
      std::memcpy(&b2, &pl.planes[axis * 4 + j], 8);
      if (b2 == bits) return axis * 4 + (int)j;
    }
    if (cnt[axis] == 4) return -1;
    pl.planes[axis * 4 + cnt[axis]] = v;
    return axis * 4 + (int)cnt[axis]++;
  };
  static const int FACE[6] = {0, 3, 1, 4, 2, 5}; // bounds[] index of the faces in div6's order
  auto table_user = [&](int i) { return in.objects[i].kind == RPT_SHAPE_MESH && !in.objects[i].has_xf; };
  pl.plane_idx.assign(n, 0);
  pl.plane_use.assign(n, 0);
  for (int i = 0; i < n && planes_ok; i++) {
    if (!table_user(i)) continue;
    for (int k = 0; k < 6; k++) {
      int sl = slot_of(FACE[k] % 3, in.objects[i].bounds[FACE[k]]);
      if (sl < 0) { planes_ok = false; break; }
      pl.plane_idx[i] |= (uint32_t)sl << (4 * k);
    }
  }
  if (planes_ok && cnt[0] + cnt[1] + cnt[2] > 0 && !in.no_plane_table) {
    // plane_use = number of consecutive table users starting here, capped at the device's run length
    for (int i = n - 1; i >= 0; i--) {
      if (!table_user(i)) continue;
      uint32_t next = (i + 1 < n) ? pl.plane_use[i + 1] : 0u;
      pl.plane_use[i] = std::min<uint32_t>((uint32_t)RPT_FLAT_RUN, 1u + next);
    }
    lay.plane_cnt = cnt[0] | (cnt[1] << 4) | (cnt[2] << 8);
    // the table's slots are packed (x planes, then y, then z): plane_idx goes from axis * 4 + j to that numbering
    const uint32_t base[3] = {0u, cnt[0], cnt[0] + cnt[1]};
    for (int i = 0; i < n; i++) {
      if (!pl.plane_use[i]) continue;
      uint32_t packed = 0;
      for (int k = 0; k < 6; k++) {
        const uint32_t sl = (pl.plane_idx[i] >> (4 * k)) & 15u;
        packed |= (base[sl >> 2] + (sl & 3u)) << (4 * k);
      }
      const FlatObject& o = in.objects[i]; // (above the slots' 24 bits: the shadow window's mark, axis_flat_mesh)
      if (axis_flat_mesh(o.kind, o.has_xf, o.single_leaf, o.bounds, o.recs, o.n_recs)) packed |= RPT_PLANE_AXIS_FLAT;
      pl.plane_idx[i] = packed;
    }
    const uint64_t qtab_bytes = (uint64_t)(cnt[0] + cnt[1] + cnt[2]) * 64 * sizeof(double);
    lay.off_qtab = (uint32_t)off; off = up16(off + qtab_bytes);
    // one light, and it casts shadow rays: rpt_paths<KdFlat> traces a hit's shadow ray and bounce ray in one query,
    // with the shadow ray's quotients in a second table behind the first — if the wave's share still holds it
    if (RPT_FUSE_QUERY && RPT_RAY_STASH >= 2 && lay.n_tris && in.n_lights == 1 && in.light0_kind != RPT_LIGHT_AMBIENT &&
        up16(off + qtab_bytes) + RPT_PATHS_STASH_MAX_LDS <= WAVE_LDS) {
      lay.fuse_query = 1;
      off = up16(off + qtab_bytes);
    }
    // the fused kernel's tables of what a hit derives from the scene alone (kernels/paths_consts.inc SceneConsts), behind the
    // quotient tables — if the wave's share holds them too; a scene in which it does not keeps the kernel without them
    if (RPT_SCENE_CONSTS && lay.fuse_query) {
      // (as the kernel counts them: scene_consts_fill; RPT_SCENE_CONSTS is the mask of the groups that are built)
      uint64_t light_tris = 0, cubes = 0;
      const uint64_t mats = (RPT_SCENE_CONSTS & 1) ? (uint64_t)n : 0u;
      if ((RPT_SCENE_CONSTS & 2) && in.light0_plain_mesh) light_tris = in.light0_tris;
      auto xf_cube = [&](int i) { return i < n && in.objects[i].kind == RPT_SHAPE_CUBE && in.objects[i].has_xf; };
      for (int i = 0; (RPT_SCENE_CONSTS & 4) && i < n;) {
        if (xf_cube(i) && xf_cube(i + 1)) { cubes += 2; i += 2; }
        else i++;
      }
      // the cubes' normals (back to front), then at off_consts the materials' constants and the light's pdfs
      const uint64_t base = off + cubes * RPT_CUBE_NORMALS_BYTES; // (a multiple of 16, as `off` is)
      const uint64_t end = up16(base + mats * RPT_MAT_CONSTS_BYTES + light_tris * sizeof(double));
      if (end + RPT_PATHS_STASH_MAX_LDS <= WAVE_LDS) {
        lay.scene_consts = 1;
        lay.off_consts = (uint32_t)base;
        off = end;
      }
    }
    if (RPT_PRETRACE_CULL && lay.fuse_query && in.obj_filter_ok) { // (cull_always says what the pass never skips)
      lay.cull_always = cull_always(in.obj_always, plane_users((size_t)n, [&](size_t i) { return pl.plane_use[i]; }), (size_t)n);
      lay.pretrace_cull = 1;
    }
  } else {
    pl.plane_idx.assign(n, 0);
  }
  // many small objects and no plane table (a room of polygons rather than C2's five walls): the object filter
  // (host_scene.cpp fill_object_boxes).  RPTGPU_OBJECT_FILTER_MIN: from how many objects (0 = never).  Measured:
  // 2 objects -5..-11 % (C1, glass spheres), 5 objects +8 % (basic.rs), 6 objects +4 % (spheres.rs), 29 objects +40 %
  const uint64_t every = every_object((size_t)n);
  if (!lay.plane_cnt && in.object_filter_min > 0 && n >= in.object_filter_min && in.obj_filter_ok && (in.obj_always & every) != every) {
    // rpt_paths<KdFlatF> reads triangles from global memory (no plane table here, so `off` is final)
    const FlatLayout keep = lay;
    const uint64_t keep_off = off;
    if (lay.n_tris) assign(false);
    const uint64_t with_boxes = up16(off + (uint64_t)n * 6 * sizeof(double));
    if (with_boxes <= WAVE_LDS) {
      lay.obj_filter = 1;
      lay.obj_always = in.obj_always & every;
      lay.off_obox = (uint32_t)off; off = with_boxes;
      pl.upload_filter = true;
    } else {
      lay = keep;
      off = keep_off;
    }
  }
  lay.off_end = (uint32_t)off;
  pl.flat = off <= WAVE_LDS;
  return pl;
}

} // namespace rptscene
