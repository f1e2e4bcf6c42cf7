// api_mesh.cpp — rptgpu_scene_set_mesh[_device]: new triangles for one mesh of a live handle (deformation: the count
// stays).  The triangles' records are made on the device (mesh_update.hip), the tree by the builder scene creation would
// use (host_scene.h build_kd: kdbuild.hip from device_build_min boxes on, else the host), and what creation derives from
// the tree by the same functions (derive_tree, mesh_records.h grid_over, fill_object_boxes).  DESIGN.md §9 has the
// contract, the storage scheme and the audit of what follows from a tree.
//
// Storage: the spare set of the geometry arrays, written whole and swapped in at the end (tree_splice.h, shared with
// api_group.cpp).
#include "api_internal.h"
#include "mesh_records.h"
#include "mesh_update.h"
#include "tree_splice.h"

namespace {

int set_mesh(rptgpu_scene* h, uint32_t object, uint64_t n, const void* tris, bool on_device, hipStream_t user_stream,
             const std::string& fn) {
  if (!h) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, fn + "null handle");
  if (h->abandoned)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "an aborted batch's device work never drained on this handle: it takes no update (destroy it)");
  const size_t count = h->obj_geom.size();
  const std::string obj = "object " + std::to_string(object);
  if (object >= count)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + obj + " is out of range (the scene has " + std::to_string(count) + ")");
  const rptdev::Inst was = h->top_insts[object];
  if (was.kind != RPT_SHAPE_MESH)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + obj + " is not a mesh (shape kind " + std::to_string(was.kind) + ")");
  const size_t t = (size_t)was.tree;
  const rptdev::Tree old = h->host_trees[t];
  if (n != old.num_prims)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "n = " + std::to_string(n) + " differs from the triangle count of " + obj +
                                                 " at creation (" + std::to_string(old.num_prims) + "): a deformation keeps the count, re-topology needs a new handle");
  if (n && !tris) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "null triangle array");
  if (h->tree_shared[t])
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the mesh of " + obj + " is also a Light::Object's shape or a group's child (their "
                                                 "records are derived from it at creation): this needs a new handle");
  if (h->all_flat)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + obj + " is walked inside the flat path kernel, whose LDS layout and plane table are "
                                                 "derived from the coordinates at creation: this needs a new handle");
  if (!n) return RPTGPU_OK; // (an empty mesh has nothing to deform)
  return guarded(h, h->device, [&]() -> int {
    const hipStream_t st = h->stream;
    const bool print = std::getenv("RPTGPU_PRINT_UPDATE") != nullptr; // where the hand-off's time goes (stderr; adds synchronisations)
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!print) return;
      HIP_TRY(hipStreamSynchronize(st));
      auto t1 = std::chrono::steady_clock::now();
      std::fprintf(stderr, "scene_set_mesh %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    };
    const uint32_t nt = (uint32_t)n;
    const double* src = (const double*)tris;
    if (on_device) {
      if (user_stream) HIP_TRY(hipStreamSynchronize(user_stream)); // the producer's work
    } else { // the host entry point uploads and joins the device path
      h->mesh_src.alloc(n * 18u);
      HIP_TRY(hipMemcpyAsync(h->mesh_src.p, tris, n * 18u * sizeof(double), hipMemcpyHostToDevice, st));
      src = h->mesh_src.p;
    }
    // ---- the triangles' records: Tri into the spare array's region, TriX and boxes by triangle index
    h->alt_tris.alloc(h->n_tris);
    copy_around(h->alt_tris.p, h->tris.p, old.prim_base, n, n, h->n_tris, st);
    h->mesh_trix.alloc(n); h->mesh_boxes.alloc(n); h->mesh_flag.alloc(1);
    HIP_TRY(hipMemsetAsync(h->mesh_flag.p, 0, sizeof(uint32_t), st));
    HIP_TRY(rptmesh::tri_records(st, src, nt, h->alt_tris.p + old.prim_base, h->mesh_trix.p, h->mesh_boxes.p, h->mesh_flag.p));
    lap("upload, triangle records");
    // ---- the tree: the 48-byte boxes come to the host, where both builders take them (kdbuild.hip numbers its nodes on
    // the host as well), and the bounds are folded in index order as KdTree::new folds them
    std::vector<rpthost::Box> boxes(n);
    uint32_t any_sliver = 0;
    HIP_TRY(hipMemcpyAsync(boxes.data(), h->mesh_boxes.p, n * sizeof(rpthost::Box), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&any_sliver, h->mesh_flag.p, sizeof any_sliver, hipMemcpyDeviceToHost, st));
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
    rptmesh::LeafGrid grid;
    rptrec::grid_over(tr.bounds, tr.qlo, tr.qscale);
    std::memcpy(grid.qlo, tr.qlo, sizeof grid.qlo);
    std::memcpy(grid.qscale, tr.qscale, sizeof grid.qscale);
    const uint32_t depth = kb.max_depth;
    lap("kd build");
    // an object the handle walks inside the path kernels keeps that route; their stacks hold fast_max_depth levels
    for (size_t i = 0; i < count; i++)
      if (h->top_insts[i].kind == RPT_SHAPE_MESH && (size_t)h->top_insts[i].tree == t && !h->obj_deep[i] && depth > h->opt.fast_max_depth)
        return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the deformed tree is " + std::to_string(depth) + " levels deep and object " +
                                                     std::to_string(i) + " is walked inside the path kernels, whose stacks hold " +
                                                     std::to_string(h->opt.fast_max_depth) + ": this needs a new handle");
    // ---- the spare set, packed as a fresh handle packs it
    TreeSplice sp;
    if (!plan_splice(h, t, kb, sp))
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the scene's trees would outgrow 32-bit node or entry indices");
    pack_spare_tree(h, sp, kb, st);
    lap("copies, nodes and entries");
    HIP_TRY(rptmesh::leaf_records(st, h->alt_refs.p + old.ref_base, (uint32_t)sp.nr, nt, h->mesh_trix.p, h->mesh_boxes.p, grid,
                                  h->alt_trix.p + old.ref_base, h->alt_lbox.p + old.ref_base));
    lap("leaf records");
    // the tree records (the later trees' regions moved) and every instance of this tree (Inst::bounds copies Tree::bounds)
    std::vector<rptdev::Tree> trees = spliced_trees(h, sp, tr);
    std::vector<rptdev::Inst> insts = h->top_insts;
    std::vector<rpthost::ObjectGeom> geom = h->obj_geom;
    for (size_t i = 0; i < count; i++) {
      if (insts[i].kind != RPT_SHAPE_MESH || (size_t)insts[i].tree != t) continue;
      std::memcpy(insts[i].bounds, tr.bounds, sizeof tr.bounds);
      for (int k = 0; k < 3; k++) { geom[i].local.lo[k] = tr.bounds[k]; geom[i].local.hi[k] = tr.bounds[3 + k]; }
      if (count <= 64) geom[i].sliver = any_sliver != 0; // (as flatten_scene: read by the object filter only, which takes <= 64 objects)
    }
    rpthost::ObjectBounds ob;
    rpthost::fill_object_boxes(insts, geom, ob);
    pack_spare_insts(h, st);
    pack_spare_records(h, trees, insts, st);
    HIP_TRY(hipStreamSynchronize(st));
    lap("tree and object records");
    // ---- the swap: from here on nothing fails
    swap_spare(h, sp, trees, insts, geom, ob, depth, true);
    // what the routing and the workspace took from the tree at creation (api_scene.cpp)
    for (size_t i = 0; i < count; i++)
      if (h->top_insts[i].kind == RPT_SHAPE_MESH && (size_t)h->top_insts[i].tree == t) reroute_object(h, i, tr, depth);
    return RPTGPU_OK;
  });
}

} // namespace

extern "C" {

int rptgpu_scene_set_mesh(rptgpu_scene* h, uint32_t object, uint64_t n, const RptTriangle* tris) {
  return set_mesh(h, object, n, tris, false, nullptr, "rptgpu_scene_set_mesh: ");
}

int rptgpu_scene_set_mesh_device(rptgpu_scene* h, uint32_t object, uint64_t n, const void* d_tris, void* stream) {
  return set_mesh(h, object, n, d_tris, true, (hipStream_t)stream, "rptgpu_scene_set_mesh_device: ");
}

} // extern "C"
