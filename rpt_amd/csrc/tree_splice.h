// tree_splice.h — what the live updates that rebuild ONE tree of a handle share (api_mesh.cpp: a deformed mesh;
// api_group.cpp: a group's moved children), one copy for both: the refusals they make first, the lap timer, the tree's
// rebuild from its primitives' boxes, the spare-set storage, the swap and the re-route (scene_plan.h).
//
// insts, trees, nodes, refs, tris, lrec and lbox exist twice on a handle that has been updated: the set the kernels read
// and a spare.  An update writes the WHOLE new scene into the spare — the other trees' nodes, entries and records copied
// device to device, packed in tree order exactly as a fresh handle packs them, the updated tree's region in between at
// its new size — waits for the stream, and only then swaps the two sets and the host copies.  Nothing the kernels read is
// written before the swap, so a refusal or a failure leaves the handle as it was; the spare keeps its allocation (grown
// by an eighth beyond need when it must grow) for the next update.
#pragma once
#include "api_internal.h"
#include "mesh_records.h"
#include "scene_plan.h"

namespace rptapi {

// ---- the frame of a rebuild

// the words in which the two calls' shared refusals differ
struct RebuildWords {
  int32_t kind;           // RPT_SHAPE_MESH / RPT_SHAPE_GROUP
  const char* a_kind;     // "a mesh"
  const char* counted;    // "triangle": what n counts
  const char* count_rule; // why n may not change
  const char* rebuilt;    // "deformed": the new tree, in the depth refusal
};
struct RebuildTarget {
  size_t count = 0, t = 0; // top-level objects; the object's tree
  rptdev::Tree old{};      // that tree's record
  std::string obj;         // "object <index>"
};
// The refusals both calls make first, in this order: a null handle, an abandoned one, the object's index, its kind, n
// against the count at creation.  -> RPTGPU_OK and `tg`, or the failure's code
inline int rebuild_target(rptgpu_scene* h, uint32_t object, uint64_t n, const RebuildWords& w, const std::string& fn, RebuildTarget& tg) {
  if (!h) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, fn + "null handle");
  if (h->abandoned) return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + ABANDONED_TAKES_NO_UPDATE);
  tg.count = h->obj_geom.size();
  tg.obj = "object " + std::to_string(object);
  if (object >= tg.count)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + tg.obj + " is out of range (the scene has " + std::to_string(tg.count) + ")");
  const rptdev::Inst& was = h->top_insts[object];
  if (was.kind != w.kind)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + tg.obj + " is not " + w.a_kind + " (shape kind " + std::to_string(was.kind) + ")");
  tg.t = (size_t)was.tree;
  tg.old = h->host_trees[tg.t];
  if (n != tg.old.num_prims)
    return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + "n = " + std::to_string(n) + " differs from the " + w.counted + " count of " + tg.obj +
                                                 " at creation (" + std::to_string(tg.old.num_prims) + "): " + w.count_rule);
  return RPTGPU_OK;
}
// ... and last, behind their own checks of the input: a handle whose scene the flat path kernel walks
inline int refuse_all_flat(rptgpu_scene* h, const std::string& fn, const RebuildTarget& tg) {
  if (!h->all_flat) return RPTGPU_OK;
  return fail(h, RPTGPU_E_INVALID_ARGUMENT, fn + tg.obj + " is walked inside the flat path kernel, whose LDS layout and plane table are "
                                               "derived from the coordinates at creation: this needs a new handle");
}

// RPTGPU_PRINT_UPDATE=1: where the hand-off's time goes (stderr; adds synchronisations)
struct UpdateLap {
  hipStream_t st;
  const char* call; // "scene_set_mesh"
  bool print = std::getenv("RPTGPU_PRINT_UPDATE") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    if (!print) return;
    HIP_TRY(hipStreamSynchronize(st));
    auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "%s %-28s %8.3f ms\n", call, what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

// The tree over the n boxes in h->mesh_boxes (made on the handle's stream): the 48-byte boxes come to the host, where both
// builders take them (kdbuild.hip numbers its nodes on the host as well) — the builder scene creation would use, by
// h->opt — and the bounds are folded in index order as KdTree::new folds them.  flag (may be null): receives
// h->mesh_flag[0] with the same synchronisation.  tr: `old` with what creation derives from a built tree, its leaf grid
// included
struct RebuiltTree {
  rpthost::KdBuild kb;
  rptdev::Tree tr{};
  uint32_t depth = 0;
};
inline void rebuild_tree(rptgpu_scene* h, uint64_t n, const rptdev::Tree& old, uint32_t* flag, UpdateLap& lap, RebuiltTree& out) {
  const hipStream_t st = h->stream;
  std::vector<rpthost::Box> boxes(n);
  HIP_TRY(hipMemcpyAsync(boxes.data(), h->mesh_boxes.p, n * sizeof(rpthost::Box), hipMemcpyDeviceToHost, st));
  if (flag) HIP_TRY(hipMemcpyAsync(flag, h->mesh_flag.p, sizeof *flag, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  lap("boxes to the host");
  rpthost::BuildOptions bopt;
  bopt.device_build_min = (size_t)h->opt.device_build_min;
  bopt.build_threads = (int)h->opt.build_threads;
  if (bopt.device_build_min) bopt.device = h->device;
  rpthost::build_kd(boxes, &bopt, out.kb);
  HIP_TRY(hipSetDevice(h->device));
  out.tr = old;
  rpthost::derive_tree(out.kb, boxes, out.tr);
  rptrec::grid_over(out.tr.bounds, out.tr.qlo, out.tr.qscale);
  out.depth = out.kb.max_depth;
  lap("kd build");
}
// the tree's leaf grid as the record kernels take it (rptmesh::LeafGrid, rptgroup::LeafGrid: the kernels' symbols carry
// the type's name, so each keeps its own)
template <class Grid> Grid leaf_grid(const rptdev::Tree& tr) {
  Grid g;
  std::memcpy(g.qlo, tr.qlo, sizeof g.qlo);
  std::memcpy(g.qscale, tr.qscale, sizeof g.qscale);
  return g;
}
// An object the handle walks inside the path kernels keeps that route (scene_plan.h rebuilt_too_deep); "" when object i
// may take the tree
inline std::string depth_refusal(const rptgpu_scene* h, size_t i, uint32_t depth, const RebuildWords& w) {
  if (!rptscene::rebuilt_too_deep(h->obj_deep[i], depth, h->opt.fast_max_depth)) return "";
  return std::string("the ") + w.rebuilt + " tree is " + std::to_string(depth) + " levels deep and object " + std::to_string(i) +
         " is walked inside the path kernels, whose stacks hold " + std::to_string(h->opt.fast_max_depth) + ": this needs a new handle";
}
// object i's copy of its tree's bounds (Inst::bounds copies Tree::bounds) and its local box
inline void set_object_bounds(rptdev::Inst& in, rpthost::ObjectGeom& g, const rptdev::Tree& tr) {
  std::memcpy(in.bounds, tr.bounds, sizeof tr.bounds);
  for (int k = 0; k < 3; k++) { g.local.lo[k] = tr.bounds[k]; g.local.hi[k] = tr.bounds[3 + k]; }
}

// ---- the spare set

// dst[0, at) = src[0, at); dst[at + new_len, ...) = src[at + old_len, total): the arrays of the other trees around the
// updated tree's region, device to device
template <class T> void copy_around(T* dst, const T* src, uint64_t at, uint64_t old_len, uint64_t new_len, uint64_t total, hipStream_t st) {
  if (at) HIP_TRY(hipMemcpyAsync(dst, src, at * sizeof(T), hipMemcpyDeviceToDevice, st));
  const uint64_t tail = total - (at + old_len);
  if (tail) HIP_TRY(hipMemcpyAsync(dst + at + new_len, src + at + old_len, tail * sizeof(T), hipMemcpyDeviceToDevice, st));
}
template <class T> void reserve(DevBuf<T>& b, uint64_t need) {
  if (b.p && b.n >= need) return;
  b.alloc(need + need / 8); // (slack: a rebuilt tree's node and entry counts wander from frame to frame)
}

// tree t's region of nodes[] and refs[] (lrec, lbox) before and after an update, and the arrays' new totals
struct TreeSplice {
  size_t t = 0;
  uint64_t node_at = 0, ref_at = 0; // Tree::node_base / ref_base of t: they stay
  uint64_t old_nn = 0, old_nr = 0, nn = 0, nr = 0;
  uint64_t nodes_total = 0, refs_total = 0;
};

// -> false: the scene's trees would outgrow 32-bit node or entry indices
inline bool plan_splice(const rptgpu_scene* h, size_t t, const rpthost::KdBuild& kb, TreeSplice& sp) {
  const rptdev::Tree& old = h->host_trees[t];
  const bool last = t + 1 >= h->host_trees.size();
  sp.t = t;
  sp.node_at = old.node_base; sp.ref_at = old.ref_base;
  sp.old_nn = (last ? h->n_nodes : h->host_trees[t + 1].node_base) - old.node_base;
  sp.old_nr = (last ? h->n_refs : h->host_trees[t + 1].ref_base) - old.ref_base;
  sp.nn = kb.nodes.size(); sp.nr = kb.refs.size();
  sp.nodes_total = h->n_nodes - sp.old_nn + sp.nn; sp.refs_total = h->n_refs - sp.old_nr + sp.nr;
  return sp.nodes_total < 0xffffffffull && sp.refs_total + RPT_LBOX_PAD < 0xffffffffull;
}

// the spare nodes, refs, lrec and lbox, packed as a fresh handle packs them: the other trees' regions copied around tree
// t's, whose nodes and entries are uploaded; its lrec and lbox regions are the caller's to fill
inline void pack_spare_tree(rptgpu_scene* h, const TreeSplice& sp, const rpthost::KdBuild& kb, hipStream_t st) {
  reserve(h->alt_nodes, sp.nodes_total); reserve(h->alt_refs, sp.refs_total); reserve(h->alt_trix, sp.refs_total);
  reserve(h->alt_lbox, sp.refs_total + RPT_LBOX_PAD);
  copy_around(h->alt_nodes.p, h->nodes.p, sp.node_at, sp.old_nn, sp.nn, h->n_nodes, st);
  copy_around(h->alt_refs.p, h->refs.p, sp.ref_at, sp.old_nr, sp.nr, h->n_refs, st);
  copy_around(h->alt_trix.p, h->trix.p, sp.ref_at, sp.old_nr, sp.nr, h->n_refs, st);
  copy_around(h->alt_lbox.p, h->lbox.p, sp.ref_at, sp.old_nr, sp.nr, h->n_refs + RPT_LBOX_PAD, st); // (with the padding behind the last entry)
  HIP_TRY(hipMemcpyAsync(h->alt_nodes.p + sp.node_at, kb.nodes.data(), sp.nn * sizeof(rptdev::KdNode), hipMemcpyHostToDevice, st));
  if (sp.nr) HIP_TRY(hipMemcpyAsync(h->alt_refs.p + sp.ref_at, kb.refs.data(), sp.nr * sizeof(uint32_t), hipMemcpyHostToDevice, st));
}

// the tree records with t's replaced and the later trees' regions moved
inline std::vector<rptdev::Tree> spliced_trees(const rptgpu_scene* h, const TreeSplice& sp, const rptdev::Tree& tr) {
  std::vector<rptdev::Tree> trees = h->host_trees;
  trees[sp.t] = tr;
  for (size_t u = sp.t + 1; u < trees.size(); u++) {
    trees[u].node_base = (uint32_t)((uint64_t)trees[u].node_base - sp.old_nn + sp.nn);
    trees[u].ref_base = (uint32_t)((uint64_t)trees[u].ref_base - sp.old_nr + sp.nr);
  }
  return trees;
}

// the spare insts: a copy of the set the kernels read
inline void pack_spare_insts(rptgpu_scene* h, hipStream_t st) {
  h->alt_insts.alloc(h->n_insts);
  HIP_TRY(hipMemcpyAsync(h->alt_insts.p, h->insts.p, h->n_insts * sizeof(rptdev::Inst), hipMemcpyDeviceToDevice, st));
}

// the spare trees, and the top-level and light-shape records in front of the spare insts
inline void pack_spare_records(rptgpu_scene* h, const std::vector<rptdev::Tree>& trees, const std::vector<rptdev::Inst>& top, hipStream_t st) {
  h->alt_trees.upload(trees, st);
  HIP_TRY(hipMemcpyAsync(h->alt_insts.p, top.data(), top.size() * sizeof(rptdev::Inst), hipMemcpyHostToDevice, st));
}

// The swap, after the stream has drained: nothing here fails.  with_tris: the update wrote alt_tris as well.  The host
// copies follow; depths only grow — a column higher than a fresh handle's holds the same traversal — and make the
// workspace stale when they do
inline void swap_spare(rptgpu_scene* h, const TreeSplice& sp, std::vector<rptdev::Tree>& trees, std::vector<rptdev::Inst>& top,
                       std::vector<rpthost::ObjectGeom>& geom, const rpthost::ObjectBounds& ob, uint32_t depth, bool with_tris) {
  std::swap(h->insts, h->alt_insts); std::swap(h->trees, h->alt_trees); std::swap(h->nodes, h->alt_nodes);
  std::swap(h->refs, h->alt_refs); std::swap(h->trix, h->alt_trix); std::swap(h->lbox, h->alt_lbox);
  if (with_tris) std::swap(h->tris, h->alt_tris);
  rptdev::Scene& d = h->dscene;
  d.insts = h->insts.p; d.trees = h->trees.p; d.nodes = h->nodes.p; d.refs = h->refs.p; d.tris = h->tris.p; d.lrec = h->trix.p; d.lbox = h->lbox.p;
  h->n_nodes = sp.nodes_total; h->n_refs = sp.refs_total;
  h->host_trees.swap(trees);
  h->tree_depth[sp.t] = depth;
  h->top_insts.swap(top);
  h->obj_geom.swap(geom);
  if (ob.scene_bounds_ok) std::memcpy(h->scene_bounds, ob.scene_bounds, sizeof h->scene_bounds);
  if (depth > h->max_tree_depth) { h->max_tree_depth = depth; h->ws_stale = true; }                  // the spill columns' height
  if (depth + 1u > h->gen_levels) { h->gen_levels = depth + 1u; h->gen_threads = 0; h->ws_stale = true; } // rpt_tree_generic's
}

// What the routing took from object i's tree at creation, after the swap: scene_plan.h reroute_object into the handle
// (a flag that rises makes the workspace stale where it sizes a grid)
inline void reroute_object(rptgpu_scene* h, size_t i, const rptdev::Tree& tr, uint32_t depth) {
  const rptscene::Reroute r = rptscene::reroute_object(h->obj_deep[i], h->obj_tris[i], tr.regular != 0, tr.root_leaf != 0, depth, h->opt.fast_max_depth);
  h->obj_deep[i] = r.deep;
  h->obj_tris[i] = r.tris;
  if (r.gen_all && !h->gen_all) { h->gen_all = true; h->ws_stale = true; }
  if (r.tree_kids) { h->tree_kids = true; h->prefer_wavefront = true; }
}

} // namespace rptapi
