// rpt_paths_vertices of the parity build with the extended shape set: -ffp-contract=off.  (The ray stash is off:
// kernels_vertices_strict.hip says why.)
#define RPT_NS rpt_strict_ext_vertices
#define RPT_EXT_SHAPES 1
#define RPT_VERTICES_TU 1
#define RPT_RAY_STASH 0
#include "kernels.inc"
