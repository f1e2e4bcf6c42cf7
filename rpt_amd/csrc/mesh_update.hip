// mesh_update.hip — a deformed mesh's records on gfx950, for rptgpu_scene_set_mesh[_device] (api_mesh.cpp).
// Compiled with -ffp-contract=off like every other object; f64 division and square root are the correctly rounded ones
// (no fast-math flag anywhere), so the records are bit for bit what host_scene.cpp computes at creation from the same
// expressions (mesh_records.h).
//
//  * rpt_mesh_tri_records: one thread per triangle.  The caller's 144-byte triangle is read once, copied to the handle's
//    Tri array, and TriX, the bounding box and the sliver flag are derived from the registers.
//  * rpt_mesh_leaf_records: one thread per entry of the new tree's refs[]: the leaf-ordered copy of the triangle's TriX
//    and its 16-bit box on the tree's grid.
// The kd build between the two is kdbuild.hip's or the host's (api_mesh.cpp decides as scene creation does).
#include "mesh_update.h"

#include "mesh_records.h"

namespace rptmesh {

namespace {

constexpr int BLOCK = 256;

__global__ __launch_bounds__(BLOCK) void rpt_mesh_tri_records(const double* __restrict__ src, uint32_t n,
                                                              rptdev::Tri* __restrict__ tris, rptdev::TriX* __restrict__ trix,
                                                              rpthost::Box* __restrict__ boxes, uint32_t* __restrict__ any_sliver) {
  const uint32_t i = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
  if (i >= n) return;
  double v[18];
  const double* t = src + (size_t)i * 18u;
  for (int k = 0; k < 18; k++) v[k] = t[k];
  rptdev::Tri out;
  for (int k = 0; k < 18; k++) out.v[k] = v[k];
  tris[i] = out;
  rptdev::TriX x;
  rptrec::fill_trix(v, x);
  trix[i] = x;
  rpthost::Box b;
  rptrec::tri_box(v, b.lo, b.hi);
  boxes[i] = b;
  if (rptrec::sliver(x)) atomicOr(any_sliver, 1u);
}

__global__ __launch_bounds__(BLOCK) void rpt_mesh_leaf_records(const uint32_t* __restrict__ refs, uint32_t nrefs, uint32_t n,
                                                               const rptdev::TriX* __restrict__ trix,
                                                               const rpthost::Box* __restrict__ boxes, LeafGrid grid,
                                                               rptdev::TriX* __restrict__ lrec, rptdev::LeafBox* __restrict__ lbox) {
  const uint32_t j = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
  if (j >= nrefs) return;
  const uint32_t tri = refs[j];
  if (tri >= n) return; // (the builders only emit indices of the boxes they were given)
  const rptdev::TriX x = trix[tri];
  lrec[j] = x;
  const rpthost::Box b = boxes[tri];
  lbox[j] = rptrec::quantise_box(b.lo, b.hi, grid.qlo, grid.qscale, rptrec::sliver(x));
}

uint32_t blocks(uint32_t n) { return (n + (uint32_t)BLOCK - 1u) / (uint32_t)BLOCK; }

} // namespace

hipError_t tri_records(hipStream_t st, const double* src, uint32_t n, rptdev::Tri* tris, rptdev::TriX* trix,
                       rpthost::Box* boxes, uint32_t* any_sliver) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(rpt_mesh_tri_records, dim3(blocks(n)), dim3(BLOCK), 0, st, src, n, tris, trix, boxes, any_sliver);
  return hipGetLastError();
}

hipError_t leaf_records(hipStream_t st, const uint32_t* refs, uint32_t nrefs, uint32_t n, const rptdev::TriX* trix,
                        const rpthost::Box* boxes, const LeafGrid& grid, rptdev::TriX* lrec, rptdev::LeafBox* lbox) {
  if (!nrefs) return hipSuccess;
  hipLaunchKernelGGL(rpt_mesh_leaf_records, dim3(blocks(nrefs)), dim3(BLOCK), 0, st, refs, nrefs, n, trix, boxes, grid, lrec, lbox);
  return hipGetLastError();
}

} // namespace rptmesh
