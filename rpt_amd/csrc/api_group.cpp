// api_group.cpp — rptgpu_scene_set_group[_device]: new placements for the children of one KdTree<Box<dyn Bounded>> of a
// live handle (instanced bodies that move: the count, the kinds and the `transformed` flags stay).  The children's records
// and boxes are made on the device (group_update.hip), the tree by the builder scene creation would use (host_scene.h
// build_kd: kdbuild.hip from device_build_min boxes on, else the host), and what creation derives from the tree by the
// same functions (derive_tree, mesh_records.h grid_over, shape_records.h quadric_too_small, fill_object_boxes).
// DESIGN.md §9.2 has the contract and the audit of what follows from the tree.
//
// Storage: the spare set of the geometry arrays, written whole and swapped in at the end (tree_splice.h, shared with
// api_mesh.cpp).  The group's child region of insts keeps its size and place; nodes, refs, lrec and lbox of later trees
// shift with node_base and ref_base.
#include "api_internal.h"
#include "group_update.h"
#include "mesh_records.h"
#include "tree_splice.h"

namespace {

static_assert(sizeof(RptTransform) == rptgroup::XF_WORDS * sizeof(double), "RptTransform is 51 f64 words");

// the host entry: children (d_xf: nullptr); the device entry: d_xf, [n] RptTransform on the device (children: nullptr)
int set_group(rptgpu_scene* h, uint32_t object, uint64_t n, const RptShape* children, const void* d_xf, bool on_device,
              hipStream_t user_stream, const std::string& fn) {
  if (!h) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, fn + "null handle");
  if (h->abandoned)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "an aborted batch's device work never drained on this handle: it takes no update (destroy it)");
  const size_t count = h->obj_geom.size();
  const std::string obj = "object " + std::to_string(object);
  if (object >= count)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + obj + " is out of range (the scene has " + std::to_string(count) + ")");
  const rptdev::Inst was = h->top_insts[object];
  if (was.kind != RPT_SHAPE_GROUP)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + obj + " is not a group (shape kind " + std::to_string(was.kind) + ")");
  const size_t t = (size_t)was.tree;
  const rptdev::Tree old = h->host_trees[t];
  if (n != old.num_prims)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "n = " + std::to_string(n) + " differs from the child count of " + obj +
                                                 " at creation (" + std::to_string(old.num_prims) + "): moving the children keeps the count, other children need a new handle");
  if (n && !(on_device ? d_xf : (const void*)children))
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + (on_device ? "null transform array" : "null children array"));
  for (uint64_t i = 0; i < n && !on_device; i++) { // every child is checked before anything changes
    const uint8_t sig = h->inst_sig[old.prim_base + i];
    const int32_t kind = sig & 0x7f, has_xf = sig >> 7;
    const std::string at = "child " + std::to_string(i) + " of " + obj + ": ";
    if (children[i].kind != kind)
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + at + "shape kind " + std::to_string(children[i].kind) + " differs from the kind at creation (" +
                                                   std::to_string(kind) + "): new geometry needs a new handle");
    if ((children[i].transformed ? 1 : 0) != has_xf)
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + at + "the shape is " + (children[i].transformed ? "" : "not ") + "Transformed and was " +
                                                   (has_xf ? "" : "not ") + "at creation (its record has no placement to replace): this needs a new handle");
  }
  for (uint64_t i = 0; i < n; i++) {
    const int32_t kind = h->inst_sig[old.prim_base + i] & 0x7f;
    if (kind != RPT_SHAPE_SPHERE && kind != RPT_SHAPE_CUBE)
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "child " + std::to_string(i) + " of " + obj + " is a mesh, a monomial surface or a group (shape kind " +
                                                   std::to_string(kind) + "): its box comes from more than a placement, and only groups of spheres and cubes are moved — this needs a new handle");
  }
  if (h->all_flat)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + obj + " is walked inside the flat path kernel, whose LDS layout and plane table are "
                                                 "derived from the coordinates at creation: this needs a new handle");
  if (!n) return RPTGPU_OK; // (an empty group has nothing to move)
  return guarded(h, h->device, [&]() -> int {
    const hipStream_t st = h->stream;
    const bool print = std::getenv("RPTGPU_PRINT_UPDATE") != nullptr; // where the hand-off's time goes (stderr; adds synchronisations)
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!print) return;
      HIP_TRY(hipStreamSynchronize(st));
      auto t1 = std::chrono::steady_clock::now();
      std::fprintf(stderr, "scene_set_group %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    };
    const uint32_t nk = (uint32_t)n;
    const double* src = (const double*)d_xf;
    std::vector<double> staged; // (alive until the stream has drained below)
    if (on_device) {
      if (user_stream) HIP_TRY(hipStreamSynchronize(user_stream)); // the producer's work
    } else { // the host entry point uploads the records and joins the device path
      staged.resize(n * rptgroup::XF_WORDS);
      for (uint64_t i = 0; i < n; i++)
        if (children[i].transformed) std::memcpy(&staged[i * rptgroup::XF_WORDS], &children[i].xf, sizeof(RptTransform));
      h->mesh_src.alloc(staged.size());
      HIP_TRY(hipMemcpyAsync(h->mesh_src.p, staged.data(), staged.size() * sizeof(double), hipMemcpyHostToDevice, st));
      src = h->mesh_src.p;
    }
    // ---- the children's records into the spare insts' region, their boxes by child index
    pack_spare_insts(h, st);
    h->mesh_boxes.alloc(n);
    HIP_TRY(rptgroup::child_records(st, src, nk, h->insts.p + old.prim_base, h->alt_insts.p + old.prim_base, h->mesh_boxes.p));
    lap("upload, child records");
    // ---- the tree: the 48-byte boxes come to the host, where both builders take them, and the bounds are folded in
    // index order as KdTree::new folds them
    std::vector<rpthost::Box> boxes(n);
    HIP_TRY(hipMemcpyAsync(boxes.data(), h->mesh_boxes.p, n * sizeof(rpthost::Box), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lap("boxes to the host");
    rpthost::BuildOptions bopt;
    bopt.device_build_min = (size_t)h->opt.device_build_min;
    bopt.build_threads = (int)h->opt.build_threads;
    if (bopt.device_build_min) bopt.device = h->device;
    rpthost::KdBuild kb;
    rpthost::build_kd(boxes, &bopt, kb);
    HIP_TRY(hipSetDevice(h->device));
    rptdev::Tree tr = old;
    rpthost::derive_tree(kb, boxes, tr);
    rptgroup::LeafGrid grid;
    rptrec::grid_over(tr.bounds, tr.qlo, tr.qscale);
    std::memcpy(grid.qlo, tr.qlo, sizeof grid.qlo);
    std::memcpy(grid.qscale, tr.qscale, sizeof grid.qscale);
    const uint32_t depth = kb.max_depth;
    lap("kd build");
    // a group the handle walks inside the path kernels keeps that route; their stacks hold fast_max_depth levels
    if (!h->obj_deep[object] && depth > h->opt.fast_max_depth)
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the rebuilt tree is " + std::to_string(depth) + " levels deep and " + obj +
                                                   " is walked inside the path kernels, whose stacks hold " +
                                                   std::to_string(h->opt.fast_max_depth) + ": this needs a new handle");
    // ---- the spare set, packed as a fresh handle packs it
    TreeSplice sp;
    if (!plan_splice(h, t, kb, sp))
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the scene's trees would outgrow 32-bit node or entry indices");
    pack_spare_tree(h, sp, kb, st);
    // (a group's lrec slots are unused: zeros, as a fresh handle's)
    if (sp.nr) HIP_TRY(hipMemsetAsync(h->alt_trix.p + old.ref_base, 0, sp.nr * sizeof(rptdev::TriX), st));
    lap("copies, nodes and entries");
    HIP_TRY(rptgroup::leaf_boxes(st, h->alt_refs.p + old.ref_base, (uint32_t)sp.nr, nk, h->alt_insts.p + old.prim_base, h->mesh_boxes.p,
                                 grid, h->alt_lbox.p + old.ref_base));
    lap("leaf boxes");
    // the tree records (the later trees' regions moved) and the group object itself (Inst::bounds copies Tree::bounds)
    std::vector<rptdev::Tree> trees = spliced_trees(h, sp, tr);
    std::vector<rptdev::Inst> insts = h->top_insts;
    std::vector<rpthost::ObjectGeom> geom = h->obj_geom;
    std::memcpy(insts[object].bounds, tr.bounds, sizeof tr.bounds);
    for (int k = 0; k < 3; k++) { geom[object].local.lo[k] = tr.bounds[k]; geom[object].local.hi[k] = tr.bounds[3 + k]; }
    rpthost::ObjectBounds ob;
    rpthost::fill_object_boxes(insts, geom, ob);
    pack_spare_records(h, trees, insts, st);
    HIP_TRY(hipStreamSynchronize(st));
    lap("tree and object records");
    // ---- the swap: from here on nothing fails
    swap_spare(h, sp, trees, insts, geom, ob, depth, false);
    reroute_object(h, object, tr, depth); // what the routing took from the tree at creation (api_scene.cpp)
    return RPTGPU_OK;
  });
}

} // namespace

extern "C" {

int rptgpu_scene_set_group(rptgpu_scene* h, uint32_t object, uint64_t n, const RptShape* children) {
  return set_group(h, object, n, children, nullptr, false, nullptr, "rptgpu_scene_set_group: ");
}

int rptgpu_scene_set_group_device(rptgpu_scene* h, uint32_t object, uint64_t n, const void* d_transforms, void* stream) {
  return set_group(h, object, n, nullptr, d_transforms, true, (hipStream_t)stream, "rptgpu_scene_set_group_device: ");
}

} // extern "C"
