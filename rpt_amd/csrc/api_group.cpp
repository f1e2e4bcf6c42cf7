// api_group.cpp — rptgpu_scene_set_group[_device]: new placements for the children of one KdTree<Box<dyn Bounded>> of a
// live handle (instanced bodies that move: the count, the kinds and the `transformed` flags stay).  The children's records
// and boxes are made on the device (group_update.hip), the tree by the builder scene creation would use (host_scene.h
// build_kd: kdbuild.hip from device_build_min boxes on, else the host), and what creation derives from the tree by the
// same functions (derive_tree, mesh_records.h grid_over, shape_records.h quadric_too_small, fill_object_boxes).
// DESIGN.md §9.2 has the contract and the audit of what follows from the tree.
//
// The call's frame — first refusals, lap timer, the tree's rebuild, the spare set of the geometry arrays (written whole
// and swapped in at the end), the re-route — is tree_splice.h's, shared with api_mesh.cpp.  The group's child region of
// insts keeps its size and place; nodes, refs, lrec and lbox of later trees shift with node_base and ref_base.
#include "api_internal.h"
#include "group_update.h"
#include "tree_splice.h"

namespace {

static_assert(sizeof(RptTransform) == rptgroup::XF_WORDS * sizeof(double), "RptTransform is 51 f64 words");

const RebuildWords GROUP_WORDS = {RPT_SHAPE_GROUP, "a group", "child", "moving the children keeps the count, other children need a new handle", "rebuilt"};

// the host entry: children (d_xf: nullptr); the device entry: d_xf, [n] RptTransform on the device (children: nullptr)
int set_group(rptgpu_scene* h, uint32_t object, uint64_t n, const RptShape* children, const void* d_xf, bool on_device,
              hipStream_t user_stream, const std::string& fn) {
  RebuildTarget tg;
  if (int rc = rebuild_target(h, object, n, GROUP_WORDS, fn, tg)) return rc;
  const size_t t = tg.t;
  const rptdev::Tree& old = tg.old;
  const std::string& obj = tg.obj;
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
  if (int rc = refuse_all_flat(h, fn, tg)) return rc;
  if (!n) return RPTGPU_OK; // (an empty group has nothing to move)
  return guarded(h, h->device, [&]() -> int {
    const hipStream_t st = h->stream;
    UpdateLap lap{st, "scene_set_group"};
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
    // ---- the tree
    RebuiltTree rb;
    rebuild_tree(h, n, old, nullptr, lap, rb);
    const rptdev::Tree& tr = rb.tr;
    const std::string why = depth_refusal(h, object, rb.depth, GROUP_WORDS);
    if (!why.empty()) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + why);
    // ---- the spare set, packed as a fresh handle packs it
    TreeSplice sp;
    if (!plan_splice(h, t, rb.kb, sp))
      return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "the scene's trees would outgrow 32-bit node or entry indices");
    pack_spare_tree(h, sp, rb.kb, st);
    // (a group's lrec slots are unused: zeros, as a fresh handle's)
    if (sp.nr) HIP_TRY(hipMemsetAsync(h->alt_trix.p + old.ref_base, 0, sp.nr * sizeof(rptdev::TriX), st));
    lap("copies, nodes and entries");
    HIP_TRY(rptgroup::leaf_boxes(st, h->alt_refs.p + old.ref_base, (uint32_t)sp.nr, nk, h->alt_insts.p + old.prim_base, h->mesh_boxes.p,
                                 leaf_grid<rptgroup::LeafGrid>(tr), h->alt_lbox.p + old.ref_base));
    lap("leaf boxes");
    // the tree records (the later trees' regions moved) and the group object itself
    std::vector<rptdev::Tree> trees = spliced_trees(h, sp, tr);
    std::vector<rptdev::Inst> insts = h->top_insts;
    std::vector<rpthost::ObjectGeom> geom = h->obj_geom;
    set_object_bounds(insts[object], geom[object], tr);
    rpthost::ObjectBounds ob;
    rpthost::fill_object_boxes(insts, geom, ob);
    pack_spare_records(h, trees, insts, st);
    HIP_TRY(hipStreamSynchronize(st));
    lap("tree and object records");
    // ---- the swap: from here on nothing fails
    swap_spare(h, sp, trees, insts, geom, ob, rb.depth, false);
    reroute_object(h, object, tr, rb.depth);
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
