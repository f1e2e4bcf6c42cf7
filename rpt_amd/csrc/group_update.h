// group_update.h — the device half of rptgpu_scene_set_group[_device] (group_update.hip): the records of a group's moved
// children and of its new tree's leaf entries, made on gfx950 from shape_records.h's expressions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "host_scene.h"

namespace rptgroup {

constexpr uint32_t XF_WORDS = 51; // RptTransform as f64 words: transform[16] linear[9] inverse_transform[16] normal_transform[9] scale

// One thread per child i of xf ([n][51] f64, RptTransform records, on the device): out[i] = was[i] with inv, nrm, fwd, lin
// and scale replaced as set_transform writes them (a child that is not Transformed keeps its record: xf[i] is not read),
// boxes[i] = the kind's local box through Transformed::bounding_box, or the local box itself.  was / out: the group's
// child regions of the set the kernels read and of the spare.  Enqueued on st; -> hipGetLastError() of the launch
hipError_t child_records(hipStream_t st, const double* xf, uint32_t n, const rptdev::Inst* was, rptdev::Inst* out,
                         rpthost::Box* boxes);

struct LeafGrid {
  double qlo[3], qscale[3]; // Tree::qlo / qscale (mesh_records.h grid_over on the tree's new bounds)
};
// One thread per leaf entry j of refs[0, nrefs) (child indices below n): lbox[j] = the conservative box of
// boxes[refs[j]] on `grid` — the whole grid for a sphere quadric_too_small names (kids: the children's new records)
hipError_t leaf_boxes(hipStream_t st, const uint32_t* refs, uint32_t nrefs, uint32_t n, const rptdev::Inst* kids,
                      const rpthost::Box* boxes, const LeafGrid& grid, rptdev::LeafBox* lbox);

} // namespace rptgroup
