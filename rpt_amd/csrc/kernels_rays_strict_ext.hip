// rpt_paths_rays, rpt_rays_ids and rpt_project_probes of the parity build with the extended shape set: -ffp-contract=off.
#define RPT_NS rpt_strict_ext_rays
#define RPT_EXT_SHAPES 1
#define RPT_RAYS_TU 1
#include "kernels.inc"
