// rpt_paths_views of the parity build with the extended shape set: -ffp-contract=off.
#define RPT_NS rpt_strict_ext_views
#define RPT_EXT_SHAPES 1
#define RPT_VIEWS_TU 1
#include "kernels.inc"
