// rpt_paths_rays, rpt_rays_ids and rpt_project_probes of the parity build (kernels/paths_rays.inc), in a translation unit of
// their own: -ffp-contract=off.
#define RPT_NS rpt_strict_rays
#define RPT_RAYS_TU 1
#include "kernels.inc"
