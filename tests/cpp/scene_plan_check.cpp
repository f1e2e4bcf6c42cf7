// Host-side check of rpt_amd/csrc/scene_plan.h: the routing of a scene's objects, the re-route after a live rebuild and the
// flat path kernel's LDS layout, compared field for field with the expressions rptgpu_scene_create_opts, reroute_object and
// the live updates' depth refusal carried before the planner existed (transcribed below over the same plain inputs), over
// the enumerated boundaries of every rule, and pinned to a few literal layouts derived by hand from device_types.h.
// Usage: scene_plan_check <section>; prints "ok <checks>" or one "FAIL" line per failed check (exit status 1).
// scene_plan_check live <7 numbers> prints the route of one tree and its re-route after a live rebuild (see live() below).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>

#include "../../rpt_amd/csrc/scene_plan.h"

using namespace rptscene;

static long checks = 0, failures = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    checks++;                                                                                    \
    if (!(cond) && failures++ < 20) std::printf("FAIL scene_plan_check.cpp:%d: %s\n", __LINE__, #cond); \
  } while (0)

static RptSceneOptions options() { // rptgpu_scene_options_default's values of the fields the planner reads
  RptSceneOptions o;
  std::memset(&o, 0, sizeof o);
  o.deep_depth = 8;
  o.fast_max_depth = (uint32_t)rptdev::KD_MAX_STACK;
  o.sort_rays = -1;
  o.sort_min_bytes = 8ull << 20;
  o.sort_shadow_min_bytes = 8ull << 20;
  o.nest_trace = 1;
  o.object_filter_min = 5;
  return o;
}

// ---- the routing loop of rptgpu_scene_create_opts as it stood, one object per call: `h` is what it kept on the handle
struct OldHandle {
  bool tree_kids = false, sort_rays = false, gen_all = false, has_deep = false, prefer_wavefront = false, path_reorder = false,
       all_flat = false;
  std::vector<uint8_t> obj_deep, obj_tris;
  int sort_mode = -1;
  uint64_t sort_min_bytes = 0, sort_shadow_min_bytes = 0;
};
static bool old_route(OldHandle* h, const ObjectFacts& f, const RptSceneOptions& opt) { // -> Tree::generic_only
  const uint32_t fast_max_depth = opt.fast_max_depth, deep_depth = opt.deep_depth;
  h->sort_mode = opt.sort_rays;
  h->sort_min_bytes = opt.sort_min_bytes;
  h->sort_shadow_min_bytes = opt.sort_shadow_min_bytes;
  bool tree = f.kind == RPT_SHAPE_MESH || f.kind == RPT_SHAPE_GROUP;
  bool deep = tree && f.depth >= deep_depth;
  const bool kids = f.kind == RPT_SHAPE_GROUP && f.tree_kids != 0;
  const bool too_deep = tree && f.depth > fast_max_depth;
  deep = deep || kids || too_deep;
  h->tree_kids = h->tree_kids || kids || too_deep;
  bool sort = false, sort_shadow = false;
  if (deep) {
    uint64_t bytes = f.bytes;
    sort = h->sort_mode == 1 || (h->sort_mode < 0 && bytes >= h->sort_min_bytes);
    sort_shadow = sort && (h->sort_mode == 1 || bytes >= h->sort_shadow_min_bytes);
  }
  uint8_t trace_kind = f.kind == RPT_SHAPE_MESH ? 1 : 0;
  bool generic_only = false;
  if (kids) {
    uint32_t inner_depth = 0;
    bool ok = f.regular && !(f.tree_kids & 2u);
    if (f.tree_kids & 1u) { // (the loop over the mesh children, folded by the caller into kids_depth / kids_regular)
      inner_depth = std::max(inner_depth, f.kids_depth);
      ok = ok && f.kids_regular;
    }
    if (ok && opt.nest_trace != 0 && f.depth + inner_depth + 2 <= (uint32_t)rptdev::KD_MAX_STACK) trace_kind = 2;
    else generic_only = true;
  }
  if (generic_only) {
    trace_kind = 3;
    sort = false;
    sort_shadow = false;
  }
  h->sort_rays = h->sort_rays || sort;
  const bool all_generic = deep && (generic_only || !f.regular);
  h->gen_all = h->gen_all || all_generic;
  h->obj_deep.push_back(deep ? (uint8_t)((sort ? 2 : 1) | (all_generic ? 4 : 0) | (sort && !sort_shadow ? 8 : 0)) : 0);
  const bool one_leaf = !tree || f.root_leaf != 0;
  h->obj_tris.push_back((uint8_t)(trace_kind | (!deep && one_leaf ? 16 : 0)));
  h->has_deep = h->has_deep || deep;
  return generic_only;
}
// ... and what followed the loop, before the layout
static void old_fold(OldHandle* h, uint32_t max_tree_depth, bool scene_bounds_ok, size_t n_trees, bool all_root_leaf, const char* env) {
  h->prefer_wavefront = max_tree_depth >= 3 || h->prefer_wavefront;
  h->path_reorder = !h->has_deep && scene_bounds_ok && n_trees != 0;
  if (const char* e = env) h->path_reorder = h->path_reorder && std::atoi(e) != 0;
  if (h->tree_kids) h->prefer_wavefront = true;
  h->all_flat = all_root_leaf;
  if (h->all_flat) h->path_reorder = false;
}

static std::vector<ObjectFacts> routing_facts(const RptSceneOptions& opt) {
  std::vector<ObjectFacts> all;
  std::set<uint32_t> depths = {0u, 1u, opt.deep_depth - 1, opt.deep_depth, opt.fast_max_depth, opt.fast_max_depth + 1};
  std::set<uint64_t> sizes = {0ull, opt.sort_min_bytes - 1, opt.sort_min_bytes, opt.sort_shadow_min_bytes - 1, opt.sort_shadow_min_bytes};
  for (int kind : {RPT_SHAPE_SPHERE, RPT_SHAPE_PLANE, RPT_SHAPE_CUBE, RPT_SHAPE_MESH, RPT_SHAPE_GROUP, RPT_SHAPE_MONOMIAL})
    for (uint32_t depth : depths)
      for (uint64_t bytes : sizes)
        for (int regular = 0; regular < 2; regular++)
          for (int root_leaf = 0; root_leaf < 2; root_leaf++)
            for (uint32_t tk = 0; tk < 4; tk++) {
              ObjectFacts f;
              f.kind = kind; f.depth = depth; f.bytes = bytes; f.regular = regular != 0; f.root_leaf = root_leaf != 0;
              f.tree_kids = kind == RPT_SHAPE_GROUP ? tk : 0u;
              if (kind != RPT_SHAPE_GROUP && tk) continue;
              if (!(f.tree_kids & 1u)) { all.push_back(f); continue; }
              // mesh children: the two levels sum to KD_MAX_STACK - 2 (fits one stack) and - 1 (does not), one shallow
              // pair, and one irregular child
              std::set<uint32_t> inner = {0u, 3u};
              for (uint32_t sum : {(uint32_t)rptdev::KD_MAX_STACK - 2, (uint32_t)rptdev::KD_MAX_STACK - 1})
                if (sum >= depth) inner.insert(sum - depth);
              for (uint32_t kd : inner)
                for (int kr = 0; kr < 2; kr++) {
                  f.kids_depth = kd; f.kids_regular = kr != 0;
                  all.push_back(f);
                }
            }
  return all;
}

static void routing() {
  std::vector<RptSceneOptions> opts;
  for (int sort_rays = -1; sort_rays <= 1; sort_rays++)
    for (int nest = 0; nest < 2; nest++)
      for (int variant = 0; variant < 3; variant++) {
        RptSceneOptions o = options();
        o.sort_rays = sort_rays;
        o.nest_trace = nest;
        if (variant == 1) { o.sort_min_bytes = 1000; o.sort_shadow_min_bytes = 5000; o.fast_max_depth = 12; }
        if (variant == 2) { o.sort_min_bytes = 5000; o.sort_shadow_min_bytes = 1000; o.fast_max_depth = 5; o.deep_depth = 8; } // (tests: too deep below deep_depth)
        opts.push_back(o);
      }
  long nest_seen = 0, generic_seen = 0, closest_only_seen = 0;
  for (const RptSceneOptions& o : opts) {
    const std::vector<ObjectFacts> facts = routing_facts(o);
    for (const ObjectFacts& f : facts) {
      OldHandle h;
      const bool generic_only = old_route(&h, f, o);
      const ObjectRoute r = route_object(f, o);
      CHECK(r.deep == h.obj_deep[0] && r.tris == h.obj_tris[0] && r.generic_only == generic_only);
      CHECK(r.has_deep == h.has_deep && r.tree_kids == h.tree_kids && r.sort_rays == h.sort_rays && r.gen_all == h.gen_all);
      nest_seen += (r.tris & RPT_TRACE_KIND) == RPT_TRACE_NEST;
      generic_seen += (r.tris & RPT_TRACE_KIND) == RPT_TRACE_GENERIC;
      closest_only_seen += (r.deep & RPT_DEEP_SORT_CLOSEST) != 0;
    }
    // the fold: every pair of (a sample of) the objects, in order, under every scene-level input
    std::vector<ObjectFacts> sample;
    for (size_t i = 0; i < facts.size(); i += 37) sample.push_back(facts[i]);
    for (const ObjectFacts& a : sample)
      for (const ObjectFacts& b : sample)
        for (int bits = 0; bits < 48; bits++) {
          const uint32_t max_depth = (bits & 1) ? 3u : 2u;
          const bool bounds_ok = bits & 2, all_root_leaf = bits & 4;
          const size_t n_trees = (bits & 8) ? 2 : 0;
          const char* env = bits < 16 ? nullptr : bits < 32 ? "0" : "1";
          OldHandle h;
          old_route(&h, a, o); old_route(&h, b, o);
          old_fold(&h, max_depth, bounds_ok, n_trees, all_root_leaf, env);
          const SceneRoute s = fold_routes({route_object(a, o), route_object(b, o)}, max_depth, bounds_ok, n_trees, all_root_leaf,
                                           !env || std::atoi(env) != 0);
          CHECK(s.has_deep == h.has_deep && s.tree_kids == h.tree_kids && s.sort_rays == h.sort_rays && s.gen_all == h.gen_all);
          CHECK(s.prefer_wavefront == h.prefer_wavefront && s.path_reorder == h.path_reorder && s.all_flat == h.all_flat);
        }
  }
  CHECK(nest_seen > 0 && generic_seen > 0 && closest_only_seen > 0); // (the enumeration reaches every route)
  // literals: a primitive, a one-leaf mesh, a deep mesh under the three sort modes, the kd-trees-of-kd-trees rule
  RptSceneOptions o = options();
  ObjectFacts f;
  f.kind = RPT_SHAPE_SPHERE;
  CHECK(route_object(f, o).deep == 0 && route_object(f, o).tris == 16);
  f.kind = RPT_SHAPE_MESH; f.depth = 0; f.root_leaf = true;
  CHECK(route_object(f, o).deep == 0 && route_object(f, o).tris == 17);
  f.depth = 7; f.root_leaf = false;
  CHECK(route_object(f, o).deep == 0 && route_object(f, o).tris == 1);
  f.depth = 8; f.bytes = (8ull << 20) - 1;
  CHECK(route_object(f, o).deep == 1 && route_object(f, o).tris == 1);
  f.bytes = 8ull << 20;
  CHECK(route_object(f, o).deep == 2 && route_object(f, o).sort_rays);
  o.sort_shadow_min_bytes = 32ull << 20;
  CHECK(route_object(f, o).deep == (2 | 8));
  f.regular = false;
  CHECK(route_object(f, o).deep == (2 | 4 | 8) && route_object(f, o).gen_all);
  o.sort_rays = 0;
  CHECK(route_object(f, o).deep == (1 | 4));
  o = options();
  f = ObjectFacts();
  f.kind = RPT_SHAPE_GROUP; f.depth = 2; f.tree_kids = 1; f.kids_depth = 28;
  CHECK(route_object(f, o).deep == 1 && route_object(f, o).tris == 2 && route_object(f, o).tree_kids);
  f.kids_depth = 29;
  CHECK(route_object(f, o).deep == (1 | 4) && route_object(f, o).tris == 3 && route_object(f, o).generic_only);
  f.kids_depth = 3; f.tree_kids = 3;
  CHECK(route_object(f, o).tris == 3);
  f.tree_kids = 1; f.kids_regular = false;
  CHECK(route_object(f, o).tris == 3);
  f.kids_regular = true; o.nest_trace = 0;
  CHECK(route_object(f, o).tris == 3);
}

// ---- reroute_object of tree_splice.h and the depth refusal of the two live updates, as they stood
struct OldReroute {
  uint8_t obj_deep, obj_tris;
  bool gen_all, ws_stale, tree_kids, prefer_wavefront;
};
static void old_reroute(OldReroute* h, bool regular, bool root_leaf, uint32_t depth, uint32_t fast_max_depth) {
  if (h->obj_deep) {
    h->obj_deep = (uint8_t)((h->obj_deep & ~4) | (regular ? 0 : 4));
    if (!regular && !h->gen_all) { h->gen_all = true; h->ws_stale = true; }
    if (depth > fast_max_depth) { h->tree_kids = true; h->prefer_wavefront = true; }
  } else {
    h->obj_tris = (uint8_t)((h->obj_tris & ~16) | (root_leaf ? 16 : 0));
  }
}
static void rerouting() {
  for (uint8_t deep : {0, 1, 2, 1 | 4, 2 | 4, 2 | 8, 2 | 4 | 8})
    for (uint8_t tris : {0, 1, 2, 3, 16, 17})
      for (int regular = 0; regular < 2; regular++)
        for (int root_leaf = 0; root_leaf < 2; root_leaf++)
          for (uint32_t fmd : {5u, 32u})
            for (uint32_t depth : {0u, fmd - 1, fmd, fmd + 1})
              for (int flags = 0; flags < 4; flags++) {
                OldReroute h{deep, tris, (flags & 1) != 0, false, (flags & 2) != 0, (flags & 2) != 0};
                old_reroute(&h, regular, root_leaf, depth, fmd);
                const Reroute r = reroute_object(deep, tris, regular, root_leaf, depth, fmd);
                // as tree_splice.h applies it
                bool gen_all = (flags & 1) != 0, ws_stale = false, tree_kids = (flags & 2) != 0, prefer_wavefront = tree_kids;
                if (r.gen_all && !gen_all) { gen_all = true; ws_stale = true; }
                if (r.tree_kids) { tree_kids = true; prefer_wavefront = true; }
                CHECK(r.deep == h.obj_deep && r.tris == h.obj_tris);
                CHECK(gen_all == h.gen_all && ws_stale == h.ws_stale && tree_kids == h.tree_kids && prefer_wavefront == h.prefer_wavefront);
                CHECK(rebuilt_too_deep(deep, depth, fmd) == (!deep && depth > fmd));
              }
  CHECK(reroute_object(1, 1, false, false, 33, 32).deep == 5 && reroute_object(1, 1, false, false, 33, 32).tree_kids);
  CHECK(reroute_object(6, 1, true, false, 3, 32).deep == 2 && !reroute_object(6, 1, true, false, 3, 32).gen_all);
  CHECK(reroute_object(0, 1, true, true, 3, 32).tris == 17 && reroute_object(0, 17, true, false, 3, 32).tris == 1);
  CHECK(rebuilt_too_deep(0, 33, 32) && !rebuilt_too_deep(0, 32, 32) && !rebuilt_too_deep(1, 33, 32));
}

// ---- the layout block of rptgpu_scene_create_opts as it stood, over FlatInput; `insts` stands for fs.insts
struct OldInst {
  int32_t kind, has_xf;
  double bounds[6];
  uint32_t plane_idx, plane_use;
};
struct OldLayout {
  bool all_flat = true;
  FlatLayout lay{}, flat_layout{};
  std::vector<double> planes;
  std::vector<OldInst> insts;
  bool planes_uploaded = false, filter_uploaded = false;
  int64_t margin[5] = {-1, -1, -1, -1, -1}; // bytes to spare at each fit check (tris, second table, constants, boxes, end); -1: not made
};
static uint64_t old_plane_users(const std::vector<OldInst>& insts, size_t n) {
  uint64_t m = 0;
  for (size_t i = 0; i < n && i < 64; i++)
    if (insts[i].plane_use) m |= 1ull << i;
  return m;
}
static OldLayout old_layout(const FlatInput& fi) {
  OldLayout h;
  for (const FlatObject& o : fi.objects) {
    OldInst in{o.kind, o.has_xf, {}, 0u, 0u};
    std::memcpy(in.bounds, o.bounds, sizeof in.bounds);
    h.insts.push_back(in);
  }
  const int num_objects = (int)fi.objects.size();
  const size_t refs_size = fi.n_refs, tris_size = fi.n_tris;
  constexpr uint32_t WAVE_LDS = RPT_PATHS_WAVE_LDS - RPT_PATHS_WALKER_LDS;
  auto up16 = [](uint64_t v) { return (v + 15) & ~15ull; };
  auto spare = [&](uint64_t need) { return (int64_t)WAVE_LDS - (int64_t)need + 0x100000; }; // (biased: -1 stays "not made")
  uint64_t off = 0;
  FlatLayout lay{};
  lay.n_refs = (uint32_t)refs_size;
  auto assign = [&](bool with_tris) {
    lay.n_tris = with_tris ? (uint32_t)tris_size : 0u;
    off = up16(refs_size * sizeof(rptdev::TriX));
    lay.off_tris = (uint32_t)off; off = up16(off + (uint64_t)lay.n_tris * sizeof(rptdev::Tri));
    lay.off_refs = (uint32_t)off; off = up16(off + refs_size * sizeof(uint32_t));
    lay.off_mat = (uint32_t)off;  off = up16(off + (uint64_t)num_objects * sizeof(rptdev::Material));
    lay.off_leaf = (uint32_t)off; off = up16(off + (uint64_t)num_objects * 16);
  };
  assign(true);
  h.margin[0] = spare(off + 12 * 64 * sizeof(double) + RPT_PATHS_STASH_MAX_LDS);
  if (off + 12 * 64 * sizeof(double) + RPT_PATHS_STASH_MAX_LDS > WAVE_LDS || fi.tris_global) assign(false);
  std::vector<double> planes(12, 0.0);
  uint32_t cnt[3] = {0, 0, 0};
  bool planes_ok = true;
  auto slot_of = [&](int axis, double v) -> int {
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    for (uint32_t j = 0; j < cnt[axis]; j++) {
      uint64_t b2;
      std::memcpy(&b2, &planes[axis * 4 + j], 8);
      if (b2 == bits) return axis * 4 + (int)j;
    }
    if (cnt[axis] == 4) return -1;
    planes[axis * 4 + cnt[axis]] = v;
    return axis * 4 + (int)cnt[axis]++;
  };
  static const int FACE[6] = {0, 3, 1, 4, 2, 5};
  std::vector<uint32_t> idx(num_objects, 0);
  for (int i = 0; i < num_objects && planes_ok; i++) {
    const OldInst& in = h.insts[i];
    if (in.kind != RPT_SHAPE_MESH || in.has_xf) continue;
    for (int k = 0; k < 6; k++) {
      int sl = slot_of(FACE[k] % 3, in.bounds[FACE[k]]);
      if (sl < 0) { planes_ok = false; break; }
      idx[i] |= (uint32_t)sl << (4 * k);
    }
  }
  if (planes_ok && cnt[0] + cnt[1] + cnt[2] > 0 && !fi.no_plane_table) {
    for (int i = 0; i < num_objects; i++) {
      OldInst& in = h.insts[i];
      if (in.kind == RPT_SHAPE_MESH && !in.has_xf) { in.plane_idx = idx[i]; in.plane_use = 1; }
    }
    for (int i = num_objects - 1; i >= 0; i--) {
      OldInst& in = h.insts[i];
      if (!in.plane_use) continue;
      uint32_t next = (i + 1 < num_objects) ? h.insts[i + 1].plane_use : 0u;
      in.plane_use = std::min<uint32_t>((uint32_t)RPT_FLAT_RUN, 1u + next);
    }
    lay.plane_cnt = cnt[0] | (cnt[1] << 4) | (cnt[2] << 8);
    const uint32_t base[3] = {0u, cnt[0], cnt[0] + cnt[1]};
    for (int i = 0; i < num_objects; i++) {
      OldInst& in = h.insts[i];
      if (!in.plane_use) continue;
      uint32_t packed = 0;
      for (int k = 0; k < 6; k++) {
        const uint32_t sl = (in.plane_idx >> (4 * k)) & 15u;
        packed |= (base[sl >> 2] + (sl & 3u)) << (4 * k);
      }
      in.plane_idx = packed;
    }
    const uint64_t qtab_bytes = (uint64_t)(cnt[0] + cnt[1] + cnt[2]) * 64 * sizeof(double);
    lay.off_qtab = (uint32_t)off; off = up16(off + qtab_bytes);
    const bool second = RPT_FUSE_QUERY && RPT_RAY_STASH >= 2 && lay.n_tris && fi.n_lights == 1 && fi.light0_kind != RPT_LIGHT_AMBIENT;
    if (second) h.margin[1] = spare(up16(off + qtab_bytes) + RPT_PATHS_STASH_MAX_LDS);
    if (second && up16(off + qtab_bytes) + RPT_PATHS_STASH_MAX_LDS <= WAVE_LDS) {
      lay.fuse_query = 1;
      off = up16(off + qtab_bytes);
    }
    if (RPT_SCENE_CONSTS && lay.fuse_query) {
      uint64_t light_tris = 0, cubes = 0;
      const uint64_t mats = (RPT_SCENE_CONSTS & 1) ? (uint64_t)num_objects : 0u;
      if ((RPT_SCENE_CONSTS & 2) && fi.light0_plain_mesh) light_tris = fi.light0_tris;
      auto xf_cube = [&](int i) { return i < num_objects && h.insts[i].kind == RPT_SHAPE_CUBE && h.insts[i].has_xf; };
      for (int i = 0; (RPT_SCENE_CONSTS & 4) && i < num_objects;) {
        if (xf_cube(i) && xf_cube(i + 1)) { cubes += 2; i += 2; }
        else i++;
      }
      const uint64_t base = off + cubes * RPT_CUBE_NORMALS_BYTES;
      const uint64_t end = up16(base + mats * RPT_MAT_CONSTS_BYTES + light_tris * sizeof(double));
      h.margin[2] = spare(end + RPT_PATHS_STASH_MAX_LDS);
      if (end + RPT_PATHS_STASH_MAX_LDS <= WAVE_LDS) {
        lay.scene_consts = 1;
        lay.off_consts = (uint32_t)base;
        off = end;
      }
    }
    h.planes_uploaded = true;
    if (RPT_PRETRACE_CULL && lay.fuse_query && fi.obj_filter_ok) {
      const uint64_t every = num_objects >= 64 ? ~0ull : (1ull << num_objects) - 1ull;
      lay.cull_always = (fi.obj_always | old_plane_users(h.insts, (size_t)num_objects)) & every;
      lay.pretrace_cull = 1;
    }
  }
  {
    const int min_objects = fi.object_filter_min;
    const uint64_t every = num_objects >= 64 ? ~0ull : (1ull << num_objects) - 1ull;
    if (!lay.plane_cnt && min_objects > 0 && num_objects >= min_objects && fi.obj_filter_ok && (fi.obj_always & every) != every) {
      const FlatLayout keep = lay;
      const uint64_t keep_off = off;
      if (lay.n_tris) assign(false);
      const uint64_t with_boxes = up16(off + (uint64_t)num_objects * 6 * sizeof(double));
      h.margin[3] = spare(with_boxes);
      if (with_boxes <= WAVE_LDS) {
        lay.obj_filter = 1;
        lay.obj_always = fi.obj_always & every;
        lay.off_obox = (uint32_t)off; off = with_boxes;
        h.filter_uploaded = true;
      } else {
        lay = keep;
        off = keep_off;
      }
    }
  }
  lay.off_end = (uint32_t)off;
  h.margin[4] = spare(off);
  h.lay = lay;
  h.planes = planes;
  if (off > WAVE_LDS) h.all_flat = false;
  else h.flat_layout = lay;
  return h;
}

static bool same_layout(const FlatLayout& a, const FlatLayout& b) {
  bool ok = a.off_tris == b.off_tris && a.off_refs == b.off_refs && a.off_mat == b.off_mat && a.off_leaf == b.off_leaf &&
            a.off_end == b.off_end && a.n_refs == b.n_refs && a.n_tris == b.n_tris && a.off_qtab == b.off_qtab &&
            a.plane_cnt == b.plane_cnt && a.obj_filter == b.obj_filter && a.off_obox == b.off_obox && a.obj_always == b.obj_always &&
            a.fuse_query == b.fuse_query && a.pretrace_cull == b.pretrace_cull && a.cull_n == b.cull_n &&
            a.cull_always == b.cull_always && a.scene_consts == b.scene_consts && a.off_consts == b.off_consts;
  for (int j = 0; j < RPT_CULL_MAX; j++) ok = ok && a.cull_obj[j] == b.cull_obj[j] && a.cull_lo[j] == b.cull_lo[j] && a.cull_ext[j] == b.cull_ext[j];
  return ok && !a.plane_vals && !b.plane_vals && !a.obj_box && !b.obj_box && !a.obj_grid && !b.obj_grid;
}
// the new planner against the old block on one input; -> the old block's result
static OldLayout compare_layout(const FlatInput& fi) {
  const OldLayout old = old_layout(fi);
  const FlatPlan pl = plan_flat(fi);
  CHECK(pl.flat == old.all_flat);
  CHECK(same_layout(pl.lay, old.lay));
  if (pl.flat) CHECK(same_layout(pl.lay, old.flat_layout));
  CHECK(std::memcmp(pl.planes, old.planes.data(), 12 * sizeof(double)) == 0); // (bit for bit: -0.0 is not 0.0)
  CHECK((pl.lay.plane_cnt != 0) == old.planes_uploaded && pl.upload_filter == old.filter_uploaded);
  bool same = pl.plane_idx.size() == fi.objects.size() && pl.plane_use.size() == fi.objects.size();
  for (size_t i = 0; same && i < fi.objects.size(); i++) {
    same = pl.plane_use[i] == old.insts[i].plane_use;
    if (pl.plane_use[i]) same = same && pl.plane_idx[i] == old.insts[i].plane_idx; // (as creation writes them: users only)
  }
  CHECK(same);
  return old;
}

static FlatObject object(int kind, int has_xf, double x0 = 0, double y0 = 0, double z0 = 0, double x1 = 1, double y1 = 1, double z1 = 1) {
  return FlatObject{kind, has_xf, {x0, y0, z0, x1, y1, z1}};
}
static FlatObject mesh(double x0, double y0, double z0, double x1, double y1, double z1) { return object(RPT_SHAPE_MESH, 0, x0, y0, z0, x1, y1, z1); }
static const FlatObject XF_CUBE = object(RPT_SHAPE_CUBE, 1), CUBE = object(RPT_SHAPE_CUBE, 0), SPHERE = object(RPT_SHAPE_SPHERE, 0),
                        XF_MESH = object(RPT_SHAPE_MESH, 1);
// the Cornell box of rpt_amd/scenes.py: floor, ceiling, back, left and right wall (two triangles each), two placed cubes,
// and a two-triangle mesh light
static FlatInput cornell() {
  FlatInput fi;
  fi.objects = {mesh(0, 0, 0, 556, 0, 559.2), mesh(0, 548.9, 0, 556, 548.9, 559.2), mesh(0, 0, 559.2, 556, 548.9, 559.2),
                mesh(556, 0, 0, 556, 548.9, 559.2), mesh(0, 0, 0, 0, 548.9, 559.2), XF_CUBE, XF_CUBE};
  fi.n_refs = 12; fi.n_tris = 12;
  fi.n_lights = 1; fi.light0_kind = RPT_LIGHT_OBJECT; fi.light0_plain_mesh = true; fi.light0_tris = 2;
  fi.obj_filter_ok = true; fi.obj_always = 0;
  fi.object_filter_min = 5;
  return fi;
}

static void planes() {
  // 4 distinct planes on the x axis, then a fifth: the table stays off
  FlatInput fi = cornell();
  fi.objects = {mesh(0, 0, 0, 1, 1, 1), mesh(2, 0, 0, 3, 1, 1)};
  OldLayout o = compare_layout(fi);
  CHECK(o.lay.plane_cnt == (4u | 2u << 4 | 2u << 8));
  fi.objects.push_back(mesh(3, 0, 0, 4, 1, 1));
  o = compare_layout(fi);
  CHECK(o.lay.plane_cnt == 0 && !o.insts[0].plane_use);
  for (int axis = 1; axis < 3; axis++) { // ... and on the other axes
    fi.objects = {mesh(0, 0, 0, 1, 1, 1), mesh(0, 0, 0, 1, 1, 1), mesh(0, 0, 0, 1, 1, 1)};
    fi.objects[1].bounds[axis] = 2; fi.objects[1].bounds[3 + axis] = 3;
    compare_layout(fi);
    fi.objects[2].bounds[axis] = 4;
    CHECK(compare_layout(fi).lay.plane_cnt == 0);
  }
  // -0.0 and 0.0 are two planes
  fi.objects = {mesh(0.0, 0, 0, 1, 1, 1), mesh(-0.0, 0, 0, 1, 1, 1)};
  o = compare_layout(fi);
  CHECK(o.lay.plane_cnt == (3u | 2u << 4 | 2u << 8) && std::signbit(o.planes[2]) && !std::signbit(o.planes[0]));
  // only transformed meshes, only primitives: no table; the switch
  fi.objects = {XF_MESH, XF_MESH, SPHERE};
  CHECK(compare_layout(fi).lay.plane_cnt == 0);
  fi = cornell();
  fi.no_plane_table = true;
  CHECK(compare_layout(fi).lay.plane_cnt == 0);
  // runs of table users: 1, RPT_FLAT_RUN, RPT_FLAT_RUN + 1, and a run broken by a cube
  for (int run : {1, RPT_FLAT_RUN, RPT_FLAT_RUN + 1}) {
    fi = cornell();
    fi.objects.assign(run, mesh(0, 0, 0, 1, 1, 1));
    fi.objects.push_back(SPHERE);
    o = compare_layout(fi);
    CHECK(o.insts[0].plane_use == (uint32_t)std::min(run, RPT_FLAT_RUN) && o.insts[run - 1].plane_use == 1 && !o.insts[run].plane_use);
  }
  fi.objects = {mesh(0, 0, 0, 1, 1, 1), mesh(0, 0, 0, 1, 1, 1), CUBE, mesh(0, 0, 0, 1, 1, 1), XF_MESH, mesh(0, 0, 0, 1, 1, 1)};
  o = compare_layout(fi);
  CHECK(o.insts[0].plane_use == 2 && o.insts[1].plane_use == 1 && o.insts[2].plane_use == 0 && o.insts[3].plane_use == 1 &&
        o.insts[4].plane_use == 0 && o.insts[5].plane_use == 1);
  // more than 64 objects, users beyond the mask
  fi.objects.assign(70, mesh(0, 0, 0, 1, 1, 1));
  fi.n_refs = 0; fi.n_tris = 2;
  compare_layout(fi);
}

// every (entries, triangles) pair that can matter to a fit check, over scenes that reach each of them; the sweep has to
// meet every limit exactly, one 16-byte step below it and one above (all offsets are multiples of 16)
static void fits() {
  std::vector<FlatInput> scenes;
  scenes.push_back(cornell());                                             // the table, the second table, the constants
  { FlatInput fi = cornell(); fi.light0_tris = 1; scenes.push_back(fi); }  // (the constants' end on the other 8-byte phase)
  { FlatInput fi = cornell(); fi.objects.push_back(SPHERE); scenes.push_back(fi); }
  { FlatInput fi = cornell(); fi.objects = {XF_MESH, SPHERE, SPHERE, XF_CUBE, SPHERE, CUBE}; fi.obj_always = 2; scenes.push_back(fi); } // the object filter
  { FlatInput fi = cornell(); fi.objects.assign(64, SPHERE); fi.obj_always = 1; scenes.push_back(fi); }
  // seven planes: the second table is larger than the room the first check leaves (with six they need the same)
  { FlatInput fi = cornell(); fi.objects[3].bounds[0] = 555; scenes.push_back(fi); }
  for (int n = 5; n <= 24; n++) { FlatInput fi = cornell(); fi.objects.assign(n, SPHERE); fi.obj_always = 1; scenes.push_back(fi); } // (the boxes' end at every phase)
  bool seen[5][3] = {};
  for (const FlatInput& base : scenes)
    for (uint64_t refs = 0; refs <= 142; refs++)
      for (uint64_t tris = 0; tris <= 126; tris++) {
        FlatInput fi = base;
        fi.n_refs = refs; fi.n_tris = tris;
        const OldLayout o = compare_layout(fi);
        for (int c = 0; c < 5; c++)
          for (int s = 0; s < 3; s++)
            if (o.margin[c] == 0x100000 + 16 * (s - 1)) seen[c][s] = true;
      }
  for (int c = 0; c < 5; c++) CHECK(seen[c][0] && seen[c][1] && seen[c][2]);
}

static void lights_and_cubes() {
  // 0, 1 and 2 lights, an ambient single light, a mesh light with and without a transform, a point light
  for (size_t n_lights : {0u, 1u, 2u})
    for (int kind : {RPT_LIGHT_POINT, RPT_LIGHT_AMBIENT, RPT_LIGHT_DIRECTIONAL, RPT_LIGHT_OBJECT})
      for (int plain = 0; plain < 2; plain++)
        for (int ok = 0; ok < 2; ok++)
          for (uint64_t always : {0ull, 0x20ull, ~0ull}) {
            FlatInput fi = cornell();
            fi.n_lights = n_lights; fi.light0_kind = kind;
            fi.light0_plain_mesh = kind == RPT_LIGHT_OBJECT && plain; fi.light0_tris = fi.light0_plain_mesh ? 2 : 0;
            fi.obj_filter_ok = ok != 0; fi.obj_always = always;
            const OldLayout o = compare_layout(fi);
            CHECK(o.lay.fuse_query == (n_lights == 1 && kind != RPT_LIGHT_AMBIENT ? 1u : 0u));
            CHECK(o.lay.pretrace_cull == (o.lay.fuse_query && ok ? 1u : 0u));
          }
  FlatInput fi = cornell();
  fi.tris_global = true; // (the triangles in global memory: the one-ray kernels)
  CHECK(compare_layout(fi).lay.fuse_query == 0);
  // two-cube blocks: at the start, at the end, three cubes in a row, cubes that are not placed
  const FlatObject wall = mesh(0, 0, 0, 1, 1, 1);
  const std::vector<std::vector<FlatObject>> rows = {
      {XF_CUBE, XF_CUBE, wall}, {wall, XF_CUBE, XF_CUBE}, {wall, XF_CUBE, XF_CUBE, XF_CUBE}, {XF_CUBE, wall, XF_CUBE},
      {XF_CUBE, XF_CUBE, XF_CUBE, XF_CUBE, wall}, {CUBE, CUBE, wall}, {XF_CUBE, CUBE, wall}, {wall, XF_CUBE}};
  const uint32_t blocks[8] = {1, 1, 1, 0, 2, 0, 0, 0};
  for (size_t r = 0; r < rows.size(); r++) {
    fi = cornell();
    fi.objects = rows[r];
    const OldLayout o = compare_layout(fi);
    CHECK(o.lay.scene_consts == 1 && o.lay.off_consts == o.lay.off_qtab + 2 * 6 * 512 + blocks[r] * 2 * RPT_CUBE_NORMALS_BYTES);
  }
}

static void filter() {
  for (int min : {0, 5, 6, -1})
    for (int n : {4, 5, 6, 63, 64, 65})
      for (int ok = 0; ok < 2; ok++)
        for (int which = 0; which < 4; which++) {
          FlatInput fi = cornell();
          fi.objects.assign(n, SPHERE);
          fi.objects[0] = XF_MESH;
          fi.n_refs = 2; fi.n_tris = 2;
          fi.object_filter_min = min;
          fi.obj_filter_ok = ok != 0;
          const uint64_t every = n >= 64 ? ~0ull : (1ull << n) - 1ull;
          fi.obj_always = which == 0 ? 0ull : which == 1 ? 1ull : which == 2 ? every : ~0ull; // (2, 3: covering every object)
          const OldLayout o = compare_layout(fi);
          CHECK(o.lay.obj_filter == (min > 0 && n >= min && ok && which < 2 ? 1u : 0u));
          if (o.lay.obj_filter) CHECK(o.lay.n_tris == 0 && o.lay.obj_always == (which ? 1ull : 0ull));
        }
  // the boxes do not fit: the rollback keeps the offsets of before
  FlatInput fi = cornell();
  fi.objects.assign(64, SPHERE); // 64 x 80 bytes of tables, 64 x 48 of boxes
  fi.obj_always = 1;
  fi.n_refs = 40; fi.n_tris = 40;
  OldLayout o = compare_layout(fi);
  CHECK(o.lay.obj_filter == 1 && o.lay.n_tris == 0);
  fi.n_refs = 75; fi.n_tris = 2; // 75 x 128 + up16(75 x 4) + 5120 = 15024 (the triangles went with the first fit check), + 3072 > 17920
  o = compare_layout(fi);
  CHECK(o.all_flat && o.lay.obj_filter == 0 && o.lay.n_tris == 0 && o.lay.off_end == 9600 + 304 + 5120);
  // the tables exceed the wave's share: not flat
  fi.n_refs = 141;
  o = compare_layout(fi);
  CHECK(!o.all_flat && o.flat_layout.off_end == 0);
}

// layouts derived by hand: sizeof(TriX) = 128, Tri 144, Material 64, 16 bytes of leaf record and 48 of boxes per object,
// 512 bytes of quotients per plane, MatConsts 88, a cube's normals 144; the wave's share is 20480 - 2560 = 17920 bytes, of
// which the stash takes 6656
static void literal() {
  static_assert(sizeof(rptdev::TriX) == 128 && sizeof(rptdev::Tri) == 144 && sizeof(rptdev::Material) == 64, "the literals below");
  static_assert(RPT_PATHS_WAVE_LDS - RPT_PATHS_WALKER_LDS == 17920 && RPT_PATHS_STASH_MAX_LDS == 6656 && RPT_FLAT_RUN == 6, "the literals below");
  // three spheres under a point light: materials at 0, leaf records behind them, nothing else
  FlatInput fi;
  fi.objects = {SPHERE, SPHERE, SPHERE};
  fi.n_lights = 1; fi.light0_kind = RPT_LIGHT_POINT;
  fi.obj_filter_ok = true; fi.obj_always = 0; fi.object_filter_min = 5;
  FlatPlan pl = plan_flat(fi);
  CHECK(pl.flat && pl.lay.off_tris == 0 && pl.lay.off_refs == 0 && pl.lay.off_mat == 0 && pl.lay.off_leaf == 192 && pl.lay.off_end == 240);
  CHECK(!pl.lay.plane_cnt && !pl.lay.obj_filter && !pl.lay.fuse_query && !pl.lay.pretrace_cull && !pl.lay.scene_consts && !pl.upload_filter);
  // six primitives, the first one exempt: the object filter, its boxes behind the leaf records
  fi.objects = {object(RPT_SHAPE_PLANE, 0), SPHERE, SPHERE, XF_CUBE, SPHERE, SPHERE};
  fi.obj_always = 1 | 1ull << 40;
  pl = plan_flat(fi);
  CHECK(pl.flat && pl.lay.off_mat == 0 && pl.lay.off_leaf == 384 && pl.lay.off_obox == 480 && pl.lay.off_end == 768);
  CHECK(pl.lay.obj_filter == 1 && pl.lay.obj_always == 1 && pl.upload_filter && !pl.lay.plane_cnt);
  compare_layout(fi);
  // the Cornell box: 12 entries and 12 triangles in LDS, six planes, both quotient tables, the constants of 7 objects,
  // 2 light triangles and one two-cube block
  fi = cornell();
  pl = plan_flat(fi);
  CHECK(pl.flat && pl.lay.n_refs == 12 && pl.lay.n_tris == 12);
  CHECK(pl.lay.off_tris == 1536 && pl.lay.off_refs == 3264 && pl.lay.off_mat == 3312 && pl.lay.off_leaf == 3760 && pl.lay.off_qtab == 3872);
  CHECK(pl.lay.plane_cnt == 0x222 && pl.lay.fuse_query == 1 && pl.lay.scene_consts == 1 && pl.lay.off_consts == 10304 && pl.lay.off_end == 10944);
  CHECK(pl.lay.pretrace_cull == 1 && pl.lay.cull_always == 0x1f && pl.lay.obj_filter == 0 && !pl.upload_filter);
  const double want[12] = {0, 556, 0, 0, 0, 548.9, 0, 0, 0, 559.2, 0, 0};
  CHECK(std::memcmp(pl.planes, want, sizeof want) == 0);
  const uint32_t idx[7] = {0x542210, 0x543310, 0x553210, 0x543211, 0x543200, 0, 0}, use[7] = {5, 4, 3, 2, 1, 0, 0};
  for (int i = 0; i < 7; i++) CHECK(pl.plane_idx[i] == idx[i] && pl.plane_use[i] == use[i]);
  compare_layout(fi);
  // the masks commit_update shares with the planner
  CHECK(every_object(0) == 0 && every_object(5) == 31 && every_object(63) == ~0ull >> 1 && every_object(64) == ~0ull && every_object(65) == ~0ull);
  CHECK(plane_users(7, [&](size_t i) { return pl.plane_use[i]; }) == 0x1f && cull_always(0x60 | 1ull << 9, 0x3, 7) == 0x63);
}

// ---- one live rebuild, for tests/test_update_cases_host.py: scene_plan_check live <kind> <depth> <regular> <deep_depth>
// <fast_max_depth> <new depth> <new regular> prints the creation's route of such a tree under the default options with these
// two depths (deep tris tree_kids gen_all), then what reroute_object makes of it after the rebuild (deep tris gen_all
// tree_kids) and rebuilt_too_deep; a tree is one leaf where its depth is 0
static int live(int argc, char** argv) {
  if (argc != 9) { std::printf("FAIL live takes 7 numbers\n"); return 2; }
  RptSceneOptions o = options();
  ObjectFacts f;
  f.kind = std::atoi(argv[2]); f.depth = (uint32_t)std::atoi(argv[3]); f.regular = std::atoi(argv[4]) != 0; f.root_leaf = f.depth == 0;
  o.deep_depth = (uint32_t)std::atoi(argv[5]); o.fast_max_depth = (uint32_t)std::atoi(argv[6]);
  const uint32_t depth = (uint32_t)std::atoi(argv[7]);
  const bool regular = std::atoi(argv[8]) != 0;
  const ObjectRoute r = route_object(f, o);
  const Reroute n = reroute_object(r.deep, r.tris, regular, depth == 0, depth, o.fast_max_depth);
  std::printf("ok %d %d %d %d %d %d %d %d %d\n", r.deep, r.tris, (int)r.tree_kids, (int)r.gen_all, n.deep, n.tris, (int)n.gen_all,
              (int)n.tree_kids, (int)rebuilt_too_deep(r.deep, depth, o.fast_max_depth));
  return 0;
}

int main(int argc, char** argv) {
  const char* s = argc > 1 ? argv[1] : "";
  if (!std::strcmp(s, "live")) return live(argc, argv);
  if (!std::strcmp(s, "routing")) routing();
  else if (!std::strcmp(s, "rerouting")) rerouting();
  else if (!std::strcmp(s, "planes")) planes();
  else if (!std::strcmp(s, "fits")) fits();
  else if (!std::strcmp(s, "lights")) lights_and_cubes();
  else if (!std::strcmp(s, "filter")) filter();
  else if (!std::strcmp(s, "literal")) literal();
  else { std::printf("FAIL unknown section '%s'\n", s); return 2; }
  if (failures) return 1;
  std::printf("ok %ld\n", checks);
  return 0;
}
