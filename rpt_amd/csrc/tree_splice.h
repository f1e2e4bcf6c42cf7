// tree_splice.h — the spare-set storage of the live updates that rebuild ONE tree of a handle (api_mesh.cpp: a deformed
// mesh; api_group.cpp: a group's moved children), one copy for both.
//
// insts, trees, nodes, refs, tris, lrec and lbox exist twice on a handle that has been updated: the set the kernels read
// and a spare.  An update writes the WHOLE new scene into the spare — the other trees' nodes, entries and records copied
// device to device, packed in tree order exactly as a fresh handle packs them, the updated tree's region in between at
// its new size — waits for the stream, and only then swaps the two sets and the host copies.  Nothing the kernels read is
// written before the swap, so a refusal or a failure leaves the handle as it was; the spare keeps its allocation (grown
// by an eighth beyond need when it must grow) for the next update.
#pragma once
#include "api_internal.h"

namespace rptapi {

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

// What the routing took from object i's tree at creation (api_scene.cpp), after the swap.  A per-tree object: the
// all-generic bit of obj_deep follows `regular` (gen_all sizes a grid and only grows), and a tree beyond fast_max_depth
// is for the per-tree pipeline only.  An object walked inside the path kernels: the single-leaf bit of obj_tris follows
// root_leaf (the lean build of rpt_rays_objects takes single leaves only)
inline void reroute_object(rptgpu_scene* h, size_t i, const rptdev::Tree& tr, uint32_t depth) {
  if (h->obj_deep[i]) {
    h->obj_deep[i] = (uint8_t)((h->obj_deep[i] & ~4) | (tr.regular ? 0 : 4)); // an irregular tree: every ray through rpt_tree_generic
    if (!tr.regular && !h->gen_all) { h->gen_all = true; h->ws_stale = true; }
    if (depth > h->opt.fast_max_depth) { h->tree_kids = true; h->prefer_wavefront = true; } // only the per-tree pipeline walks it
  } else {
    h->obj_tris[i] = (uint8_t)((h->obj_tris[i] & ~16) | (tr.root_leaf ? 16 : 0));
  }
}

} // namespace rptapi
