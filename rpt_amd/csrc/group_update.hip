// group_update.hip — a group's moved children on gfx950, for rptgpu_scene_set_group[_device] (api_group.cpp; DESIGN.md
// §9.2).  Compiled with -ffp-contract=off like every other object; f64 division and square root are the correctly rounded
// ones (no fast-math flag anywhere), so the records are bit for bit what host_scene.cpp computes at creation from the same
// expressions (shape_records.h, mesh_records.h).
//
//  * rpt_group_child_records: one thread per child.  The child's record goes from the set the kernels read to the spare
//    with the five Transformed fields replaced by the caller's 408-byte RptTransform; the child's box is derived from the
//    forward matrix while it is in registers.  The record is streamed field by field, never held whole (512 bytes).
//  * rpt_group_leaf_boxes: one thread per entry of the new tree's refs[]: the child's 16-bit box on the tree's grid.
// The kd build between the two is kdbuild.hip's or the host's (api_group.cpp decides as scene creation does).
#include "group_update.h"

#include "shape_records.h"

namespace rptgroup {

namespace {

constexpr int BLOCK = 256;

__global__ __launch_bounds__(BLOCK) void rpt_group_child_records(const double* __restrict__ xf, uint32_t n,
                                                                 const rptdev::Inst* __restrict__ was,
                                                                 rptdev::Inst* __restrict__ out, rpthost::Box* __restrict__ boxes) {
  const uint32_t i = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
  if (i >= n) return;
  const rptdev::Inst& w = was[i];
  rptdev::Inst& o = out[i];
  const int32_t kind = w.kind, has_xf = w.has_xf;
  o.kind = kind; o.has_xf = has_xf; o.tree = w.tree; o.material = w.material;
  for (int k = 0; k < 4; k++) o.plane[k] = w.plane[k];
  for (int k = 0; k < 6; k++) o.bounds[k] = w.bounds[k];
  o.plane_idx = w.plane_idx; o.plane_use = w.plane_use;
  double m[16];
  if (has_xf) { // set_transform (host_scene.cpp): RptTransform's fields into the record's
    const double* x = xf + (size_t)i * XF_WORDS;
    for (int k = 0; k < 16; k++) { m[k] = x[k]; o.fwd[k] = m[k]; }
    for (int k = 0; k < 9; k++) o.lin[k] = x[16 + k];
    for (int k = 0; k < 16; k++) o.inv[k] = x[25 + k];
    for (int k = 0; k < 9; k++) o.nrm[k] = x[41 + k];
    o.scale = x[50];
  } else { // (zeros since creation)
    for (int k = 0; k < 16; k++) { m[k] = 0.0; o.fwd[k] = w.fwd[k]; }
    for (int k = 0; k < 9; k++) o.lin[k] = w.lin[k];
    for (int k = 0; k < 16; k++) o.inv[k] = w.inv[k];
    for (int k = 0; k < 9; k++) o.nrm[k] = w.nrm[k];
    o.scale = w.scale;
  }
  rpthost::Box local, b;
  if (!rptrec::local_box(kind, local.lo, local.hi)) // (the host refuses groups with other children before this runs)
    for (int k = 0; k < 3; k++) { local.lo[k] = INFINITY; local.hi[k] = -INFINITY; }
  if (has_xf) rptrec::transformed_box(local.lo, local.hi, m, b.lo, b.hi);
  else b = local;
  boxes[i] = b;
}

__global__ __launch_bounds__(BLOCK) void rpt_group_leaf_boxes(const uint32_t* __restrict__ refs, uint32_t nrefs, uint32_t n,
                                                              const rptdev::Inst* __restrict__ kids,
                                                              const rpthost::Box* __restrict__ boxes, LeafGrid grid,
                                                              rptdev::LeafBox* __restrict__ lbox) {
  const uint32_t j = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
  if (j >= nrefs) return;
  const uint32_t child = refs[j];
  if (child >= n) return; // (the builders only emit indices of the boxes they were given)
  const rpthost::Box b = boxes[child];
  lbox[j] = rptrec::quantise_box(b.lo, b.hi, grid.qlo, grid.qscale, rptrec::quadric_too_small(kids[child], grid.qscale));
}

uint32_t blocks(uint32_t n) { return (n + (uint32_t)BLOCK - 1u) / (uint32_t)BLOCK; }

} // namespace

hipError_t child_records(hipStream_t st, const double* xf, uint32_t n, const rptdev::Inst* was, rptdev::Inst* out,
                         rpthost::Box* boxes) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(rpt_group_child_records, dim3(blocks(n)), dim3(BLOCK), 0, st, xf, n, was, out, boxes);
  return hipGetLastError();
}

hipError_t leaf_boxes(hipStream_t st, const uint32_t* refs, uint32_t nrefs, uint32_t n, const rptdev::Inst* kids,
                      const rpthost::Box* boxes, const LeafGrid& grid, rptdev::LeafBox* lbox) {
  if (!nrefs) return hipSuccess;
  hipLaunchKernelGGL(rpt_group_leaf_boxes, dim3(blocks(nrefs)), dim3(BLOCK), 0, st, refs, nrefs, n, kids, boxes, grid, lbox);
  return hipGetLastError();
}

} // namespace rptgroup
