// rpt_paths_vertices of the parity build (kernels/paths_vertices.inc), in a translation unit of its own: -ffp-contract=off.
// The ray stash is off here: the pre-traced, fused and pooled hand-outs keep a hit's position but not its t, which a vertex
// exports, so this form instantiates the plain fetch of every scene class.
#define RPT_NS rpt_strict_vertices
#define RPT_VERTICES_TU 1
#define RPT_RAY_STASH 0
#include "kernels.inc"
