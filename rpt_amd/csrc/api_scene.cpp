// api_scene.cpp — RptSceneOptions (defaults, sized access, validation, environment overrides), rptgpu_scene_create[_opts]
// (flattening, kd builds, the plan of scene_plan.h into the handle, upload), rptgpu_scene_set_objects / _lights, the kd-tree
// entry points (see api_internal.h)
#include "api_internal.h"
#include "scene_plan.h"

extern "C" {

namespace {
// the sizes RptSceneOptions has had under this ABI's headers: the first v6 header (before env_park / paths_batch) and today's
constexpr uint32_t OPT_SIZE_V6_FIRST = 104u, OPT_SIZE_NOW = (uint32_t)sizeof(RptSceneOptions);
static_assert(sizeof(RptSceneOptions) == 112, "a grown RptSceneOptions is a new known size: add it to known_opt_size");
bool known_opt_size(uint32_t n) { return n == OPT_SIZE_V6_FIRST || n == OPT_SIZE_NOW; }
void options_default_full(RptSceneOptions* o) {
  std::memset(o, 0, sizeof *o);
  o->struct_size = (uint32_t)sizeof *o;
  o->deep_depth = 8;              // a tree this deep pays for compaction + its own launches
  o->fast_max_depth = (uint32_t)rptdev::KD_MAX_STACK;
  o->sort_rays = -1;
  o->rays_in_kernel = 0;
  o->sort_min_bytes = 8ull << 20;
  o->sort_shadow_min_bytes = 8ull << 20; // (32 MiB until the visibility queries were sized for the shadow rays there are: sorting 40 % fewer keys, the 16k-triangle glass gains from its shadow sort what it lost before — 756 -> 775 Msamples/s)
  o->sort_min_rays = 1u << 19;
  o->nest_trace = 1;
  o->leaf_boxes = 1;
  o->object_filter_min = 5;
  o->device_build_min = 32768;
  o->build_threads = 0;
  o->paths_chunk = 0;
  o->workspace_bytes = 240ull << 30; // (96 GiB until round 6: a 288 GB device ran passes sized for a third of it)
  o->lbuf_bytes = 32ull << 30;
  o->target_paths = 0;
  o->comm_timeout_s = 300.0;
  o->env_park = 1;
}
// the caller's struct may be the smaller one of an older header: never write past ITS size
void copy_options_out(const RptSceneOptions& full, RptSceneOptions* out, uint32_t out_size) {
  std::memcpy(out, &full, out_size);
  out->struct_size = out_size;
}
const char* options_out_of_range(const RptSceneOptions& opt) {
  if (opt.sort_rays < -1 || opt.sort_rays > 1 || opt.deep_depth < 1u || opt.lbuf_bytes < 24u ||
      opt.workspace_bytes < (1ull << 20) || !(opt.comm_timeout_s > 0.0) || (opt.target_paths && opt.target_paths < 1024u) ||
      opt.paths_batch > RPT_PATHS_BATCH_MAX)
    return "RptSceneOptions: a field is out of range";
  return nullptr;
}
} // namespace

void rptgpu_scene_options_default(RptSceneOptions* o) {
  if (!o) return;
  options_default_full(o); // (this header's struct: the full size)
}

int rptgpu_scene_options_default_sized(RptSceneOptions* o, uint32_t struct_size) {
  if (!o) return RPTGPU_E_INVALID_ARGUMENT;
  if (!known_opt_size(struct_size))
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "rptgpu_scene_options_default_sized: struct_size is not a size RptSceneOptions has had under this ABI (104, 112)");
  RptSceneOptions full;
  options_default_full(&full);
  copy_options_out(full, o, struct_size);
  return RPTGPU_OK;
}

namespace {
// the environment's overrides of the options (the variables' names: include/rpt_gpu.h, RptSceneOptions), read HERE and
// nowhere else: once per handle, while it is made
void apply_env_overrides(RptSceneOptions& o, bool user_set_build_min) {
  auto ll = [](const char* name, long long& v) { if (const char* e = std::getenv(name)) { v = std::atoll(e); return true; } return false; };
  long long v;
  // several ranks on one node share the host's cores (host_scene.cpp usable_cpus): the device build pays earlier
  for (const char* name : {"RPTGPU_LOCAL_RANKS", "LOCAL_WORLD_SIZE"})
    if (const char* e = std::getenv(name)) {
      if (std::atoi(e) > 1 && !user_set_build_min) o.device_build_min = 4096; // (a default only: a caller's own 32768 stands)
      break;
    }
  if (ll("RPTGPU_DEVICE_BUILD_MIN", v)) o.device_build_min = (uint64_t)std::max(0ll, v);
  if (ll("RPTGPU_BUILD_THREADS", v)) o.build_threads = (uint32_t)std::max(1ll, v);
  if (ll("RPTGPU_FAST_MAX_DEPTH", v)) o.fast_max_depth = (uint32_t)std::max(0ll, v);
  if (ll("RPTGPU_DEEP_DEPTH", v)) o.deep_depth = (uint32_t)std::max(1ll, v);
  if (ll("RPTGPU_RAYS_IN_KERNEL", v)) o.rays_in_kernel = v != 0 ? 1 : 0;
  if (ll("RPTGPU_SORT_RAYS", v)) o.sort_rays = v < 0 ? -1 : (v != 0 ? 1 : 0); // (-1, the documented default: by the tree's footprint)
  if (ll("RPTGPU_SORT_MIN_BYTES", v)) o.sort_min_bytes = (uint64_t)std::max(0ll, v);
  if (ll("RPTGPU_SORT_SHADOW_MIN_BYTES", v)) o.sort_shadow_min_bytes = (uint64_t)std::max(0ll, v);
  if (ll("RPTGPU_SORT_MIN_RAYS", v)) o.sort_min_rays = (uint32_t)std::max(0ll, std::min(v, 0xffffffffll));
  if (ll("RPTGPU_NEST_TRACE", v)) o.nest_trace = v != 0 ? 1 : 0;
  if (ll("RPTGPU_LEAF_BOXES", v)) o.leaf_boxes = v != 0 ? 1 : 0;
  if (ll("RPTGPU_OBJECT_FILTER_MIN", v)) o.object_filter_min = (int32_t)v;
  if (ll("RPTGPU_PATHS_CHUNK", v)) o.paths_chunk = (uint32_t)std::max(0ll, v);
  if (ll("RPTGPU_ENV_PARK", v)) o.env_park = v != 0 ? 1 : 0;
  if (ll("RPTGPU_PATHS_BATCH", v)) o.paths_batch = (uint32_t)std::max(0ll, std::min(v, (long long)RPT_PATHS_BATCH_MAX));
  if (ll("RPTGPU_LBUF_BYTES", v) && v >= 24) o.lbuf_bytes = (uint64_t)v;
  if (const char* e = std::getenv("RPTGPU_TARGET_PATHS")) { uint64_t u = std::strtoull(e, nullptr, 10); if (u >= 1024) o.target_paths = u; }
  if (const char* e = std::getenv("RPTGPU_WS_BYTES")) { uint64_t u = std::strtoull(e, nullptr, 10); if (u >= (1ull << 20)) o.workspace_bytes = u; }
  if (const char* e = std::getenv("RPTGPU_COMM_TIMEOUT_S")) { double d = std::atof(e); if (d > 0.0) o.comm_timeout_s = d; }
}
} // namespace

int rptgpu_scene_get_options(const rptgpu_scene* h, RptSceneOptions* out) {
  if (!h || !out) return RPTGPU_E_INVALID_ARGUMENT;
  // the CALLER says how large its struct is (out->struct_size, set before the call — rptgpu_scene_options_default[_sized]
  // does): a caller built against the 104-byte first v6 header gets 104 bytes, not an overrun of eight
  if (!known_opt_size(out->struct_size))
    return fail(const_cast<rptgpu_scene*>(h), RPTGPU_E_INVALID_ARGUMENT, "rptgpu_scene_get_options: set out->struct_size to sizeof(RptSceneOptions) of your header first (rptgpu_scene_options_default does)");
  copy_options_out(h->opt, out, out->struct_size);
  return RPTGPU_OK;
}

} // extern "C"

namespace {
// what the routing reads of top-level object i (scene_plan.h route_object)
rptscene::ObjectFacts object_facts(const rpthost::FlatScene& fs, int i) {
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
// what the flat layout reads of the scene (scene_plan.h plan_flat)
rptscene::FlatInput flat_input(const rpthost::FlatScene& fs, const RptSceneOptions& opt) {
  rptscene::FlatInput in;
  in.n_refs = fs.refs.size(); in.n_tris = fs.tris.size();
  for (int i = 0; i < fs.num_objects; i++) {
    rptscene::FlatObject o{fs.insts[i].kind, fs.insts[i].has_xf, {}};
    std::memcpy(o.bounds, fs.insts[i].bounds, sizeof o.bounds);
    if (o.kind == RPT_SHAPE_MESH) { // a single-leaf tree's records, for the shadow window's mark (axis_flat_mesh)
      const rptdev::Tree& tr = fs.trees[fs.insts[i].tree];
      o.single_leaf = tr.root_leaf != 0;
      const size_t first = (size_t)tr.ref_base + tr.root_first; // (kernels/shapes.inc kd_leaf: lrec + ref_base + the leaf's first entry)
      if (o.single_leaf && first + (tr.root_leaf - 1u) <= fs.lrec.size()) {
        o.recs = fs.lrec.data() + first;
        o.n_recs = tr.root_leaf - 1u;
      }
    }
    in.objects.push_back(o);
  }
  in.n_lights = fs.lights.size();
  if (!fs.lights.empty()) {
    const rptdev::Light& l0 = fs.lights[0];
    in.light0_kind = l0.kind;
    if (l0.kind == RPT_LIGHT_OBJECT && fs.insts[l0.inst].kind == RPT_SHAPE_MESH && !fs.insts[l0.inst].has_xf) {
      in.light0_plain_mesh = true;
      in.light0_tris = fs.trees[fs.insts[l0.inst].tree].num_prims;
    }
  }
  in.obj_filter_ok = fs.obj_filter_ok; in.obj_always = fs.obj_always;
  in.object_filter_min = opt.object_filter_min;
  in.tris_global = std::getenv("RPTGPU_FLAT_TRIS_GLOBAL") != nullptr;
  in.no_plane_table = std::getenv("RPTGPU_NO_PLANE_TABLE") != nullptr;
  return in;
}
} // namespace

extern "C" {

int rptgpu_scene_create(const RptScene* scene, int device, rptgpu_scene** out) {
  return rptgpu_scene_create_opts(scene, device, nullptr, out);
}

int rptgpu_scene_create_opts(const RptScene* scene, int device, const RptSceneOptions* user_opts, rptgpu_scene** out) {
  if (!scene || !out) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  // ---- the options: defaults, the caller's struct, the environment, the ranges
  RptSceneOptions opt;
  options_default_full(&opt);
  bool user_set_build_min = false;
  if (user_opts) { // a caller built against the older (smaller) struct: the fields it does not know keep their defaults
    if (!known_opt_size(user_opts->struct_size)) // (only whole structs: a size in between would cut a field in half)
      return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "RptSceneOptions::struct_size does not belong to this ABI version (use rptgpu_scene_options_default)");
    std::memcpy(&opt, user_opts, user_opts->struct_size);
    opt.struct_size = (uint32_t)sizeof opt;
    if (const char* why = options_out_of_range(opt)) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, why);
    user_set_build_min = true;
  }
  apply_env_overrides(opt, user_set_build_min);
  if (const char* why = options_out_of_range(opt)) // the overrides are held to the same ranges as the fields
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, std::string(why) + " (after the RPTGPU_* environment overrides)");
  opt.fast_max_depth = std::min(opt.fast_max_depth, (uint32_t)rptdev::KD_MAX_STACK);
  // ---- flatten
  rpthost::FlatScene fs;
  std::string err;
  int rc;
  // RPTGPU_PRINT_CREATE=1: where the hand-off's time goes (stderr), for the scene-per-frame use case
  const bool print_create = std::getenv("RPTGPU_PRINT_CREATE") != nullptr;
  auto tc0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!print_create) return;
    auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "scene_create %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - tc0).count());
    tc0 = t;
  };
  // Trees of at least RPTGPU_DEVICE_BUILD_MIN primitives (default 32768; 0 = never) are built on the device when there
  // is one — the same tree, an order of magnitude sooner for large meshes (kdbuild.hip); everything else of the
  // flattening, and every validation, is host work.
  rpthost::BuildOptions bopt;
  {
    int nd = 0;
    bopt.device_build_min = (size_t)opt.device_build_min;
    bopt.build_threads = (int)opt.build_threads;
    if (bopt.device_build_min && hipGetDeviceCount(&nd) == hipSuccess && device >= 0 && device < nd) bopt.device = device;
    else (void)hipGetLastError();
  }
  try {
    rc = rpthost::flatten_scene(*scene, fs, err, &bopt); // validates shapes
  } catch (const std::bad_alloc&) {
    return fail(nullptr, RPTGPU_E_OUT_OF_MEMORY, "host allocation failed");
  } catch (...) {
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "unexpected exception while flattening");
  }
  if (rc != RPTGPU_OK) return fail(nullptr, rc, err);
  lap(fs.trees_built_on_device ? "flatten + kd build (device)" : "flatten + kd build");
  // ---- open the device
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, RPTGPU_E_NO_DEVICE, "no HIP device is visible (hipGetDeviceCount); there is no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "device index out of range");
  rptgpu_scene* h = new (std::nothrow) rptgpu_scene();
  if (!h) return fail(nullptr, RPTGPU_E_OUT_OF_MEMORY, "host allocation failed");
  h->device = device;
  try {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    h->num_cus = prop.multiProcessorCount;
    lap("device, stream, properties");
    h->opt = opt;
    h->qtune.sort_min_rays = opt.sort_min_rays;
    // ---- the plan (scene_plan.h): every object's route, the scene's flags, the flat kernel's LDS layout
    std::vector<rptscene::ObjectRoute> routes;
    for (int i = 0; i < fs.num_objects; i++) routes.push_back(rptscene::route_object(object_facts(fs, i), opt));
    bool all_root_leaf = true;
    for (const rptdev::Tree& tr : fs.trees) all_root_leaf = all_root_leaf && tr.root_leaf != 0;
    const char* env = std::getenv("RPTGPU_PATH_REORDER");
    const rptscene::SceneRoute sr =
        rptscene::fold_routes(routes, fs.max_tree_depth, fs.scene_bounds_ok, fs.trees.size(), all_root_leaf, !env || std::atoi(env) != 0);
    if ((env = std::getenv("RPTGPU_PATH_REORDER_MIN"))) h->path_reorder_min = (uint32_t)std::max(1, std::atoi(env));
    rptscene::FlatPlan flat;
    if (sr.all_flat) flat = rptscene::plan_flat(flat_input(fs, opt));
    // ---- the plan into the handle and the records that go to the device
    for (int i = 0; i < fs.num_objects; i++) {
      h->obj_deep.push_back(routes[i].deep);
      h->obj_tris.push_back(routes[i].tris);
      if (routes[i].generic_only) fs.trees[fs.insts[i].tree].generic_only = 1u;
      if (sr.all_flat && flat.plane_use[i]) { fs.insts[i].plane_idx = flat.plane_idx[i]; fs.insts[i].plane_use = flat.plane_use[i]; }
    }
    h->has_deep = sr.has_deep; h->tree_kids = sr.tree_kids; h->sort_rays = sr.sort_rays; h->gen_all = sr.gen_all;
    h->prefer_wavefront = sr.prefer_wavefront;
    h->path_reorder = sr.path_reorder;
    h->all_flat = sr.all_flat && flat.flat;
    h->max_tree_depth = fs.max_tree_depth;
    h->gen_levels = fs.generic_levels; h->gen_frames = fs.generic_frames;
    std::memcpy(h->scene_bounds, fs.scene_bounds, sizeof h->scene_bounds);
    lap("pipeline choice, flat layout");
    h->ext_shapes = fs.nested_mesh;
    for (const rptdev::Inst& in : fs.insts) h->ext_shapes = h->ext_shapes || in.kind == RPT_SHAPE_MONOMIAL;
    for (const rptdev::Light& l : fs.lights) h->light_casts.push_back(l.kind != RPT_LIGHT_AMBIENT ? 1 : 0);
    h->host_lights = fs.lights;
    h->top_insts.assign(fs.insts.begin(), fs.insts.begin() + fs.num_top_insts);
    h->host_materials = fs.materials;
    h->obj_geom = std::move(fs.obj_geom);
    // (rptgpu_scene_set_mesh, api_mesh.cpp)
    h->host_trees = fs.trees;
    h->tree_depth = fs.tree_depth;
    h->tree_shared.assign(fs.trees.size(), 0);
    for (size_t i = (size_t)fs.num_objects; i < fs.insts.size(); i++)
      if (fs.insts[i].kind == RPT_SHAPE_MESH || fs.insts[i].kind == RPT_SHAPE_GROUP) h->tree_shared[fs.insts[i].tree] = 1;
    for (const rptdev::Inst& in : fs.insts) h->inst_sig.push_back((uint8_t)((in.kind & 0x7f) | (in.has_xf ? 0x80 : 0))); // (rptgpu_scene_set_group, api_group.cpp)
    h->n_insts = fs.insts.size(); h->n_nodes = fs.nodes.size(); h->n_refs = fs.refs.size(); h->n_tris = fs.tris.size();
    // ---- upload: the scene and the plan's tables, then the one synchronisation
    h->insts.upload(fs.insts, h->stream);
    h->trees.upload(fs.trees, h->stream);
    h->nodes.upload(fs.nodes, h->stream);
    h->refs.upload(fs.refs, h->stream);
    h->tris.upload(fs.tris, h->stream);
    h->trix.upload(fs.lrec, h->stream);
    h->lbox.upload(fs.lbox, h->stream);
    h->materials.upload(fs.materials, h->stream);
    h->lights.upload(fs.lights, h->stream);
    h->env_texels.upload(fs.env_texels, h->stream);
    const std::vector<double> planes(flat.planes, flat.planes + 12), grid(fs.obj_grid, fs.obj_grid + 12);
    if (flat.lay.plane_cnt) h->plane_vals.upload(planes, h->stream);
    if (flat.upload_filter) { h->obj_box.upload(fs.obj_lbox, h->stream); h->obj_grid.upload(grid, h->stream); }
    HIP_TRY(hipStreamSynchronize(h->stream)); // (every source above lives until here)
    lap("device allocation + upload");
    // ---- the device's view: the flat layout's pointers, dscene
    if (h->all_flat) {
      h->flat_layout = flat.lay;
      h->flat_layout.plane_vals = flat.lay.plane_cnt ? h->plane_vals.p : nullptr;
      if (flat.upload_filter) { h->flat_layout.obj_box = h->obj_box.p; h->flat_layout.obj_grid = h->obj_grid.p; }
    }
    rptdev::Scene& d = h->dscene;
    d.insts = h->insts.p; d.trees = h->trees.p; d.nodes = h->nodes.p; d.refs = h->refs.p; d.tris = h->tris.p; d.lrec = h->trix.p; d.lbox = h->lbox.p;
    d.materials = h->materials.p; d.lights = h->lights.p; d.env_texels = h->env_texels.p;
    std::memcpy(d.env_color, fs.env_color, sizeof d.env_color);
    d.env_width = fs.env_width; d.env_height = fs.env_height; d.env_kind = fs.env_kind;
    d.num_objects = fs.num_objects; d.num_lights = (int32_t)fs.lights.size();
    d.num_shadow_lights = fs.num_shadow_lights;
    d.use_leaf_boxes = opt.leaf_boxes != 0 ? 1 : 0;
  } catch (const HipError& e) {
    int code = hip_fail(nullptr, e);
    delete h;
    return code;
  }
  *out = h;
  return RPTGPU_OK;
}

void rptgpu_scene_destroy(rptgpu_scene* h) { delete h; }

// ---- live updates: new placements and materials for a handle's objects and lights.  Geometry, counts, the environment,
// the routing and the workspace stay; every record that creation derives from a placement or a material is derived
// again by the same functions (host_scene.h: set_transform, convert_material, convert_light, fill_object_boxes) and
// uploaded, so the handle then holds the bits a fresh handle of the updated scene would.  Audit of what else creation
// derives from the records these calls change:
//   * the flat kernel's object filter (boxes, grid, obj_always) — recomputed; stale boxes would drop pixels.  Whether
//     the filter is on stays as decided at creation (scheduling only; objects it must not filter are in obj_always);
//   * the fused flat kernel's pre-trace cull — its exemptions (FlatLayout::cull_always) recomputed with the filter's; its
//     screen rectangles are made per render from top_insts (api_render.cpp), so they follow by construction;
//   * scene_bounds, the path re-order's key grid — recomputed (kept when the new union is not finite: scheduling only);
//   * StackSpill::zeros_common (directional lights along an axis) — recomputed (scheduling only);
//   * the plane table (untransformed meshes only: `transformed` may not change), trees, leaf boxes of group children
//     (in their group's frame: rptgpu_scene_set_group moves those, api_group.cpp), light_casts and num_shadow_lights (by kind: kinds may not change) — unchanged by
//     construction.
// ... and of what the entry points added since read that an update (these two, rptgpu_scene_set_mesh, _set_group) changes
// (tests/test_gpu_update_matrix.py holds each to a fresh handle's bits after every kind of update):
//   * rptgpu_occluded, rptgpu_bake_ao — insts through rpt_shadow_rays or the per-tree query; per call has_deep, tree_kids and
//     gen_all choose between them; their one-column workspace request re-sizes a warm handle only through ws_stale;
//   * rptgpu_first_hits, rptgpu_render_views_aov — the same route (query_by_object) and request; materials for the albedo;
//   * rptgpu_render_views[_seeded] — insts, materials and lights through the wavefront kernels; rec_ratio, measured on the
//     scene as it was, sizes the record pool (a pass that runs out starts over); view_recs, view_seeds and ray_seeds are
//     written per call;
//   * rptgpu_render_views_denoised — both of the above into vd_* arrays sized per call;
//   * rptgpu_buffer_features, _denoise, _sample_adaptive — a Buffer renders through the handle as it is at the call: on a flat
//     scene the path kernel with the filter's boxes, grid and obj_always above.
// ... and of the entry points added after those (tests/test_gpu_update_newer.py holds each to a fresh handle's bits over the
// same cases, warm before every update; none needed a change):
//   * rptgpu_hit_surface — rptgpu_first_hits' query, then rpt_hit_surface on columns of its own (surf_cols, surf_defer /
//     surf_frame).  They are sized from gen_levels, which swap_spare raises with a deeper tree: ensure_surface_columns compares
//     per call and makes them again, so no stale flag is needed; the walk reads insts, trees and lrec through dscene;
//   * rptgpu_bake_lightmap — the raster reads the caller's triangles only (its raw channels do not change with the scene); the
//     gathers run rptgpu_bake_probes' and rptgpu_bake_ao's drivers over the compacted arrays the handle keeps (lm_compact,
//     lm_scan): written per call, sized by the map, and the drivers' workspace follows ws_stale like every other;
//   * rptgpu_bake_direct, rptgpu_bake_lightmap_direct — lights and num_shadow_lights per call; the shadow queues lie in the
//     workspace (Occlusion::workspace: ensure_workspace, so ws_stale) and are walked by the route has_deep picks at the call;
//   * rptgpu_filter_lightmap — reads its arguments and scratch of its own (lf_stage, lf_ws, sized per call): nothing of the
//     scene, and none of the arrays a rebuild swaps;
//   * RPT_FLAG_RAYS_PERSISTENT (rays, probes), RPT_FLAG_VIEWS_PERSISTENT, RPT_FLAG_VERTICES_PERSISTENT — piece_persistent reads
//     tree_kids per call: once reroute_object has raised it (a rebuilt tree beyond fast_max_depth) the request is dropped and
//     the wavefront pipeline runs, as on a fresh handle of that scene; tree_kids never falls, so it stays dropped.
} // extern "C"

namespace {
// the checks both calls make before reading an entry; nullptr when they pass
const char* update_refusal(const rptgpu_scene* h, uint64_t n, const uint32_t* index, const void* entries) {
  if (h->abandoned) return ABANDONED_TAKES_NO_UPDATE;
  if (n && (!index || !entries)) return "null index or entry array";
  return nullptr;
}
// entry k names record i of `count`: in range and not named before in this call; "" when fine
std::string index_refusal(uint64_t k, uint32_t i, size_t count, std::vector<char>& seen, const char* what) {
  if (i >= count)
    return "entry " + std::to_string(k) + ": " + what + " index " + std::to_string(i) + " is out of range (the scene has " +
           std::to_string(count) + ")";
  if (seen[i]) return "entry " + std::to_string(k) + ": " + what + " " + std::to_string(i) + " is named twice in one call";
  seen[i] = 1;
  return "";
}
// the shape of entry k against the record it replaces: same kind, same `transformed`
std::string shape_refusal(uint64_t k, uint32_t i, const RptShape& s, const rptdev::Inst& was, const char* what) {
  const std::string at = "entry " + std::to_string(k) + " (" + what + " " + std::to_string(i) + "): ";
  if (s.kind != was.kind)
    return at + "shape kind " + std::to_string(s.kind) + " differs from the kind at creation (" + std::to_string(was.kind) +
           "): new geometry needs a new handle";
  if ((s.transformed ? 1 : 0) != was.has_xf)
    return at + "the shape is " + (s.transformed ? "" : "not ") + "Transformed and was " + (was.has_xf ? "" : "not ") +
           "at creation: an untransformed mesh lives in the flat kernel's plane table, so this needs a new handle";
  return "";
}
// upload what an update changed, wait for the copies, then make the host copies the handle's
void commit_update(rptgpu_scene* h, std::vector<rptdev::Inst>& insts, std::vector<rptdev::Material>* mats,
                   std::vector<rptdev::Light>* lights) {
  HIP_TRY(hipSetDevice(h->device));
  const hipStream_t st = h->stream;
  if (!insts.empty())
    HIP_TRY(hipMemcpyAsync(h->insts.p, insts.data(), insts.size() * sizeof(rptdev::Inst), hipMemcpyHostToDevice, st));
  if (mats && !mats->empty())
    HIP_TRY(hipMemcpyAsync(h->materials.p, mats->data(), mats->size() * sizeof(rptdev::Material), hipMemcpyHostToDevice, st));
  if (lights && !lights->empty())
    HIP_TRY(hipMemcpyAsync(h->lights.p, lights->data(), lights->size() * sizeof(rptdev::Light), hipMemcpyHostToDevice, st));
  rpthost::ObjectBounds ob;
  const bool cull = h->all_flat && h->flat_layout.pretrace_cull; // (the fused kernel's pre-trace pass: its exemptions follow too)
  const bool filter = h->all_flat && h->flat_layout.obj_filter;
  if (mats) { // the objects moved: the object filter and the scene bounds follow them
    rpthost::fill_object_boxes(insts, h->obj_geom, ob);
    if (filter) {
      HIP_TRY(hipMemcpyAsync(h->obj_box.p, ob.obj_lbox.data(), ob.obj_lbox.size() * sizeof(rptdev::LeafBox),
                             hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(h->obj_grid.p, ob.obj_grid, sizeof ob.obj_grid, hipMemcpyHostToDevice, st));
    }
  }
  HIP_TRY(hipStreamSynchronize(st)); // (the sources are this call's)
  h->top_insts.swap(insts);
  if (mats) {
    h->host_materials.swap(*mats);
    const size_t n = h->obj_geom.size();
    // (the filter's LDS layout does not depend on the boxes: only the exemptions change)
    if (filter) h->flat_layout.obj_always = ob.obj_always & rptscene::every_object(n);
    if (cull) // (the rectangles themselves are made per render from top_insts: api_render.cpp)
      h->flat_layout.cull_always = rptscene::cull_always(ob.obj_always, rptscene::plane_users(n, [&](size_t i) { return h->top_insts[i].plane_use; }), n);
    if (ob.scene_bounds_ok) std::memcpy(h->scene_bounds, ob.scene_bounds, sizeof h->scene_bounds);
  }
  if (lights) {
    h->host_lights.swap(*lights);
    h->spill.zeros_common = zeros_common(h->host_lights);
  }
}
} // namespace

extern "C" {

int rptgpu_scene_set_objects(rptgpu_scene* h, uint64_t n, const uint32_t* index, const RptObject* objects) {
  if (!h) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "rptgpu_scene_set_objects: null handle");
  const std::string fn = "rptgpu_scene_set_objects: ";
  if (const char* why = update_refusal(h, n, index, objects)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + why);
  try {
    const size_t count = h->obj_geom.size();
    std::vector<rptdev::Inst> insts = h->top_insts;
    std::vector<rptdev::Material> mats = h->host_materials;
    std::vector<char> seen(count, 0);
    for (uint64_t k = 0; k < n; k++) { // everything is checked before anything changes
      const uint32_t i = index[k];
      std::string why = index_refusal(k, i, count, seen, "object");
      if (why.empty()) why = shape_refusal(k, i, objects[k].shape, insts[i], "object");
      if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + why);
      std::string err;
      if (rpthost::convert_material(objects[k].material, i, mats[i], err) != RPTGPU_OK)
        return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "entry " + std::to_string(k) + ": " + err);
      rpthost::set_transform(insts[i], objects[k].shape);
    }
    commit_update(h, insts, &mats, nullptr);
  } catch (const HipError& e) {
    return hip_fail(h, e);
  } catch (const std::bad_alloc&) {
    return fail(h, RPTGPU_E_OUT_OF_MEMORY, fn + "host allocation failed");
  }
  return RPTGPU_OK;
}

int rptgpu_scene_set_lights(rptgpu_scene* h, uint64_t n, const uint32_t* index, const RptLight* lights) {
  if (!h) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "rptgpu_scene_set_lights: null handle");
  const std::string fn = "rptgpu_scene_set_lights: ";
  if (const char* why = update_refusal(h, n, index, lights)) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + why);
  try {
    const size_t count = h->host_lights.size();
    std::vector<rptdev::Inst> insts = h->top_insts;
    std::vector<rptdev::Light> recs = h->host_lights;
    std::vector<char> seen(count, 0);
    for (uint64_t k = 0; k < n; k++) {
      const uint32_t i = index[k];
      std::string why = index_refusal(k, i, count, seen, "light");
      if (why.empty() && lights[k].kind != recs[i].kind)
        why = "entry " + std::to_string(k) + " (light " + std::to_string(i) + "): light kind " + std::to_string(lights[k].kind) +
              " differs from the kind at creation (" + std::to_string(recs[i].kind) + ")";
      if (why.empty() && recs[i].kind == RPT_LIGHT_OBJECT)
        why = shape_refusal(k, i, lights[k].object.shape, insts[recs[i].inst], "light");
      if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + why);
      rptdev::Light dl;
      std::string err;
      if (rpthost::convert_light(lights[k], dl, err) != RPTGPU_OK)
        return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "entry " + std::to_string(k) + ": " + err);
      dl.inst = recs[i].inst;
      if (dl.kind == RPT_LIGHT_OBJECT) rpthost::set_transform(insts[dl.inst], lights[k].object.shape);
      recs[i] = dl;
    }
    commit_update(h, insts, nullptr, &recs);
  } catch (const HipError& e) {
    return hip_fail(h, e);
  } catch (const std::bad_alloc&) {
    return fail(h, RPTGPU_E_OUT_OF_MEMORY, fn + "host allocation failed");
  }
  return RPTGPU_OK;
}

// KdBuild -> the malloc'ed arrays of RptKdTree
static int kdtree_export(const rpthost::KdBuild& kb, RptKdTree* out) {
  size_t nn = kb.nodes.size(), nr = kb.refs.size();
  out->split = (double*)std::malloc(std::max<size_t>(nn, 1) * sizeof(double));
  out->info = (uint32_t*)std::malloc(std::max<size_t>(nn, 1) * sizeof(uint32_t));
  out->a = (uint32_t*)std::malloc(std::max<size_t>(nn, 1) * sizeof(uint32_t));
  out->b = (uint32_t*)std::malloc(std::max<size_t>(nn, 1) * sizeof(uint32_t));
  out->refs = (uint32_t*)std::malloc(std::max<size_t>(nr, 1) * sizeof(uint32_t));
  if (!out->split || !out->info || !out->a || !out->b || !out->refs) {
    rptgpu_kdtree_free(out);
    return RPTGPU_E_OUT_OF_MEMORY;
  }
  for (size_t i = 0; i < nn; i++) {
    out->split[i] = kb.nodes[i].split;
    out->info[i] = kb.nodes[i].ib & 3u;
    out->a[i] = kb.nodes[i].a;
    out->b[i] = kb.nodes[i].ib >> 2;
  }
  std::memcpy(out->refs, kb.refs.data(), nr * sizeof(uint32_t));
  out->num_nodes = nn;
  out->num_refs = nr;
  out->max_depth = kb.max_depth;
  out->regular = kb.regular ? 1u : 0u;
  return RPTGPU_OK;
}

int rptgpu_kdtree_build(const double* boxes, uint64_t n, RptKdTree* out) {
  if (!out || (n && !boxes)) return RPTGPU_E_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof *out);
  try {
    std::vector<rpthost::Box> b(n);
    for (uint64_t i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) {
        b[i].lo[k] = boxes[6 * i + k];
        b[i].hi[k] = boxes[6 * i + 3 + k];
      }
    rpthost::KdBuild kb;
    rpthost::kd_build(b, kb);
    return kdtree_export(kb, out);
  } catch (...) {
    return RPTGPU_E_OUT_OF_MEMORY;
  }
}

int rptgpu_kdtree_build_device(const double* boxes, uint64_t n, int device, RptKdTree* out) {
  if (!out || (n && !boxes)) return RPTGPU_E_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof *out);
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
    return fail(nullptr, RPTGPU_E_NO_DEVICE, "no HIP device is visible (hipGetDeviceCount); there is no CPU fallback");
  if (device < 0 || device >= nd) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "device index out of range");
  try {
    std::vector<rpthost::Box> b(n);
    for (uint64_t i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) {
        b[i].lo[k] = boxes[6 * i + k];
        b[i].hi[k] = boxes[6 * i + 3 + k];
      }
    rpthost::KdBuild kb;
    std::string why;
    if (!rpthost::kd_build_device(b, kb, device, why))
      return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "the device kd build does not take this input: " + why);
    return kdtree_export(kb, out);
  } catch (...) {
    return RPTGPU_E_OUT_OF_MEMORY;
  }
}

void rptgpu_kdtree_free(RptKdTree* t) {
  if (!t) return;
  std::free(t->split); std::free(t->info); std::free(t->a); std::free(t->b); std::free(t->refs);
  std::memset(t, 0, sizeof *t);
}

} // extern "C"
