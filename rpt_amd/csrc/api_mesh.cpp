// api_mesh.cpp — rptgpu_scene_set_mesh[_device]: new triangles for one mesh of a live handle (deformation: the count
// stays).  The triangles' records are made on the device (mesh_update.hip), the tree by the builder scene creation would
// use (host_scene.h build_kd: kdbuild.hip from device_build_min boxes on, else the host), and what creation derives from
// the tree by the same functions (derive_tree, mesh_records.h grid_over, fill_object_boxes).  DESIGN.md §9 has the
// contract, the storage scheme and the audit of what follows from a tree.
//
// The call's frame — first refusals, lap timer, the tree's rebuild, the spare set of the geometry arrays (written whole
// and swapped in at the end), the re-route — is tree_splice.h's, shared with api_group.cpp; here is what a mesh adds.
#include "api_internal.h"
#include "mesh_update.h"
#include "tree_splice.h"

namespace {

const RebuildWords MESH_WORDS = {RPT_SHAPE_MESH, "a mesh", "triangle", "a deformation keeps the count, re-topology needs a new handle", "deformed"};

int set_mesh(rptgpu_scene* h, uint32_t object, uint64_t n, const void* tris, bool on_device, hipStream_t user_stream,
             const std::string& fn) {
  RebuildTarget tg;
  if (int rc = rebuild_target(h, object, n, MESH_WORDS, fn, tg)) return rc;
  const size_t count = tg.count, t = tg.t;
  const rptdev::Tree& old = tg.old;
  if (n && !tris) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "null triangle array");
  if (h->tree_shared[t])
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the mesh of " + tg.obj + " is also a Light::Object's shape or a group's child (their "
                                                 "records are derived from it at creation): this needs a new handle");
  if (int rc = refuse_all_flat(h, fn, tg)) return rc;
  if (!n) return RPTGPU_OK; // (an empty mesh has nothing to deform)
  return guarded(h, h->device, [&]() -> int {
    const hipStream_t st = h->stream;
    UpdateLap lap{st, "scene_set_mesh"};
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
    // ---- the tree
    uint32_t any_sliver = 0;
    RebuiltTree rb;
    rebuild_tree(h, n, old, &any_sliver, lap, rb);
    const rptdev::Tree& tr = rb.tr;
    auto uses_tree = [&](size_t i) { return h->top_insts[i].kind == RPT_SHAPE_MESH && (size_t)h->top_insts[i].tree == t; };
    for (size_t i = 0; i < count; i++)
      if (uses_tree(i)) {
        const std::string why = depth_refusal(h, i, rb.depth, MESH_WORDS);
        if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + why);
      }
    // ---- the spare set, packed as a fresh handle packs it
    TreeSplice sp;
    if (!plan_splice(h, t, rb.kb, sp))
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the scene's trees would outgrow 32-bit node or entry indices");
    pack_spare_tree(h, sp, rb.kb, st);
    lap("copies, nodes and entries");
    HIP_TRY(rptmesh::leaf_records(st, h->alt_refs.p + old.ref_base, (uint32_t)sp.nr, nt, h->mesh_trix.p, h->mesh_boxes.p,
                                  leaf_grid<rptmesh::LeafGrid>(tr), h->alt_trix.p + old.ref_base, h->alt_lbox.p + old.ref_base));
    lap("leaf records");
    // the tree records (the later trees' regions moved) and every instance of this tree
    std::vector<rptdev::Tree> trees = spliced_trees(h, sp, tr);
    std::vector<rptdev::Inst> insts = h->top_insts;
    std::vector<rpthost::ObjectGeom> geom = h->obj_geom;
    for (size_t i = 0; i < count; i++) {
      if (!uses_tree(i)) continue;
      set_object_bounds(insts[i], geom[i], tr);
      // the shadow window's mark (scene_plan.h axis_flat_mesh) speaks of the triangles at creation: a deformed mesh loses
      // it.  (Only the flat path kernel reads it, and refuse_all_flat keeps this call off its handles: the mark of a
      // scene that did not fit the kernel's LDS is what is cleared here, so that no record keeps a statement that is stale.)
      insts[i].plane_idx &= ~RPT_PLANE_AXIS_FLAT;
      if (count <= 64) geom[i].sliver = any_sliver != 0; // (as flatten_scene: read by the object filter only, which takes <= 64 objects)
    }
    rpthost::ObjectBounds ob;
    rpthost::fill_object_boxes(insts, geom, ob);
    pack_spare_insts(h, st);
    pack_spare_records(h, trees, insts, st);
    HIP_TRY(hipStreamSynchronize(st));
    lap("tree and object records");
    // ---- the swap: from here on nothing fails
    swap_spare(h, sp, trees, insts, geom, ob, rb.depth, true);
    for (size_t i = 0; i < count; i++)
      if (uses_tree(i)) reroute_object(h, i, tr, rb.depth);
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
