// Host-side view of the routing of a scene (no GPU): the PRODUCT's flattener (rpt_amd/csrc/host_scene.cpp) on a scene handed
// over as its ABI structs, then the product's planner (rpt_amd/csrc/scene_plan.h route_object, fold_routes) on what the
// flattener made — the two steps of rptgpu_scene_create_opts between "validate" and "open the device".  Built as a shared
// library next to host_scene.cpp and called through ctypes by tests/test_routes_matrix_host.py, which lowers the scenes of
// tests/small_scenes.py exactly as GpuScene does.  routes_of writes, as text:
//   scene rc <code> ext <0|1> objects <n> has_deep <0|1> tree_kids <0|1> gen_all <0|1> path_reorder <0|1> all_flat <0|1>
//   object <i> shape <RPT_SHAPE_*> trace <RPT_TRACE_*> deep <route byte> generic_only <0|1> depth <levels> kids <tree_kids bits>
// Two pieces of api_scene.cpp live in its anonymous namespace beside HIP calls and are transcribed here: object_facts (what
// the planner reads of a flattened object) and the defaults of the options the planner reads; `ext` is its two lines that set
// rptgpu_scene::ext_shapes.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rpt_amd/csrc/host_scene.h"
#include "../../rpt_amd/csrc/scene_plan.h"

namespace rpthost { // the device builder is not linked into this test: the host builder makes the same tree
bool kd_build_device(const std::vector<Box>&, KdBuild&, int, std::string& why) { why = "not linked"; return false; }
}

namespace {
RptSceneOptions options() { // options_default_full's values of the fields the planner reads
  RptSceneOptions o;
  std::memset(&o, 0, sizeof o);
  o.struct_size = (uint32_t)sizeof o;
  o.deep_depth = 8;
  o.fast_max_depth = (uint32_t)rptdev::KD_MAX_STACK;
  o.sort_rays = -1;
  o.sort_min_bytes = 8ull << 20;
  o.sort_shadow_min_bytes = 8ull << 20;
  o.nest_trace = 1;
  o.object_filter_min = 5;
  return o;
}

rptscene::ObjectFacts object_facts(const rpthost::FlatScene& fs, int i) { // api_scene.cpp's
  const rptdev::Inst& in = fs.insts[i];
  rptscene::ObjectFacts f;
  f.kind = in.kind;
  if (in.kind != RPT_SHAPE_MESH && in.kind != RPT_SHAPE_GROUP) return f;
  const rptdev::Tree& tr = fs.trees[in.tree];
  const bool last = (size_t)in.tree + 1 >= fs.trees.size();
  const uint64_t nodes = (last ? fs.nodes.size() : fs.trees[in.tree + 1].node_base) - tr.node_base;
  const uint64_t refs = (last ? fs.refs.size() : fs.trees[in.tree + 1].ref_base) - tr.ref_base;
  f.depth = fs.tree_depth[in.tree];
  f.regular = tr.regular != 0;
  f.root_leaf = tr.root_leaf != 0;
  f.bytes = nodes * sizeof(rptdev::KdNode) + refs * (sizeof(uint32_t) + (in.kind == RPT_SHAPE_MESH ? sizeof(rptdev::TriX) : 0));
  if (in.kind == RPT_SHAPE_GROUP) {
    f.tree_kids = fs.tree_kids[in.tree];
    for (uint32_t k = 0; k < tr.num_prims; k++) {
      const rptdev::Inst& kid = fs.insts[tr.prim_base + k];
      if (kid.kind != RPT_SHAPE_MESH) continue;
      f.kids_depth = std::max(f.kids_depth, fs.tree_depth[kid.tree]);
      f.kids_regular = f.kids_regular && fs.trees[kid.tree].regular;
    }
  }
  return f;
}
} // namespace

extern "C" int routes_of(const RptScene* scene, char* out, uint64_t cap) {
  if (!scene || !out || !cap) return -1;
  std::string text;
  char line[256];
  rpthost::FlatScene fs;
  std::string err;
  int rc;
  try {
    rc = rpthost::flatten_scene(*scene, fs, err, nullptr);
  } catch (...) {
    rc = -2;
  }
  if (rc != RPTGPU_OK) {
    std::snprintf(line, sizeof line, "scene rc %d %s\n", rc, err.c_str());
    text = line;
  } else {
    const RptSceneOptions opt = options();
    std::vector<rptscene::ObjectRoute> routes;
    std::vector<rptscene::ObjectFacts> facts;
    for (int i = 0; i < fs.num_objects; i++) {
      facts.push_back(object_facts(fs, i));
      routes.push_back(rptscene::route_object(facts.back(), opt));
    }
    bool all_root_leaf = true;
    for (const rptdev::Tree& tr : fs.trees) all_root_leaf = all_root_leaf && tr.root_leaf != 0;
    const rptscene::SceneRoute sr = rptscene::fold_routes(routes, fs.max_tree_depth, fs.scene_bounds_ok, fs.trees.size(), all_root_leaf, true);
    bool ext = fs.nested_mesh;
    for (const rptdev::Inst& in : fs.insts) ext = ext || in.kind == RPT_SHAPE_MONOMIAL;
    std::snprintf(line, sizeof line, "scene rc 0 ext %d objects %d has_deep %d tree_kids %d gen_all %d path_reorder %d all_flat %d\n", ext ? 1 : 0,
                  (int)fs.num_objects, sr.has_deep ? 1 : 0, sr.tree_kids ? 1 : 0, sr.gen_all ? 1 : 0, sr.path_reorder ? 1 : 0, sr.all_flat ? 1 : 0);
    text = line;
    for (int i = 0; i < fs.num_objects; i++) {
      std::snprintf(line, sizeof line, "object %d shape %d trace %d deep %d generic_only %d depth %u kids %u\n", i, (int)facts[i].kind,
                    (int)(routes[i].tris & RPT_TRACE_KIND), (int)routes[i].deep, routes[i].generic_only ? 1 : 0, facts[i].depth, facts[i].tree_kids);
      text += line;
    }
  }
  if (text.size() + 1 > cap) return -3;
  std::memcpy(out, text.c_str(), text.size() + 1);
  return rc;
}
