// rpt_paths_views of the parity build (kernels/paths_views.inc), in a translation unit of its own: -ffp-contract=off.
#define RPT_NS rpt_strict_views
#define RPT_VIEWS_TU 1
#include "kernels.inc"
