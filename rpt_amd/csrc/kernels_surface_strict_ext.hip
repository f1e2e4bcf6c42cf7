// rpt_hit_surface of the parity build with the extended shape set (kernels/hit_surface.inc), in a translation unit of
// its own: -ffp-contract=off.  The code objects of the other translation units stay what they were without it.
#define RPT_NS rpt_strict_ext_surface
#define RPT_SURFACE_TU 1
#define RPT_EXT_SHAPES 1
#include "kernels.inc"
