// mesh_update.h — the device half of rptgpu_scene_set_mesh[_device] (mesh_update.hip): the records of a deformed mesh's
// triangles and of its new tree's leaf entries, made on gfx950 from mesh_records.h's expressions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "host_scene.h"

namespace rptmesh {

// One thread per triangle of src ([n][18] f64: v1 v2 v3 n1 n2 n3, on the device): tris[i] the triangle as it is, trix[i]
// its intersection record, boxes[i] its bounding box; *any_sliver (zeroed by the caller) becomes 1 when some triangle is
// a sliver.  Enqueued on st; -> hipGetLastError() of the launch
hipError_t tri_records(hipStream_t st, const double* src, uint32_t n, rptdev::Tri* tris, rptdev::TriX* trix,
                       rpthost::Box* boxes, uint32_t* any_sliver);

struct LeafGrid {
  double qlo[3], qscale[3]; // Tree::qlo / qscale (mesh_records.h grid_over on the tree's new bounds)
};
// One thread per leaf entry j of refs[0, nrefs) (triangle indices below n): lrec[j] = trix[refs[j]] and lbox[j] its
// conservative box on `grid` (the whole grid for a sliver)
hipError_t leaf_records(hipStream_t st, const uint32_t* refs, uint32_t nrefs, uint32_t n, const rptdev::TriX* trix,
                        const rpthost::Box* boxes, const LeafGrid& grid, rptdev::TriX* lrec, rptdev::LeafBox* lbox);

} // namespace rptmesh
