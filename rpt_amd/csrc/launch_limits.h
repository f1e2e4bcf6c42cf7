// launch_limits.h — what the launchers (kernels.h) share with the host's planners: the bounds of the render planner
// (render_plan.h) and the route bytes the scene planner (scene_plan.h) hands to launch_query; free of HIP.
#pragma once
#include <stdint.h>

// The per-tree pipeline's two route bytes per top-level object (rptgpu_scene::obj_deep / obj_tris, KernelTable::query):
// scene_plan.h route_object makes them at creation, reroute_object after a live rebuild; kernels/launch.inc reads them.
// obj_deep: 0 = walked inside the path kernels.  Else PER_TREE or SORTED (exactly one of the two: the object's rays go
// through the per-tree kernels, with the ray sort in front when SORTED), and
//   ALL_GENERIC   every ray of it goes through rpt_tree_generic (an irregular tree, an object only that kernel is built for)
//   SORT_CLOSEST  the sort serves the closest-hit query only, not the shadow rays
enum : uint8_t { RPT_DEEP_PER_TREE = 1, RPT_DEEP_SORTED = 2, RPT_DEEP_ROUTE = 3, RPT_DEEP_ALL_GENERIC = 4, RPT_DEEP_SORT_CLOSEST = 8 };
// obj_tris, low nibble: which traversal kernel of the per-tree pipeline — GROUP rpt_tree_trace over a group of simple
// shapes, MESH rpt_tree_trace<TRIS>, NEST a group with mesh children whose two regular levels fit one traversal stack
// (rpt_nest_trace; RPTGPU_NEST_TRACE=0: rpt_tree_generic instead), GENERIC rpt_tree_generic alone (Tree::generic_only).
// ONE_LEAF (objects walked inside the path kernels): a primitive or a tree that is ONE leaf — runs of such objects take
// the lean build of rpt_rays_objects (kernels/tree_query.inc)
enum : uint8_t { RPT_TRACE_GROUP = 0, RPT_TRACE_MESH = 1, RPT_TRACE_NEST = 2, RPT_TRACE_GENERIC = 3, RPT_TRACE_KIND = 15, RPT_TRIS_ONE_LEAF = 16 };

// slots (of REC_FIELDS doubles) per thread of the persistent path kernel's record ring (kernels/paths.inc says why)
static inline uint32_t rpt_fold_ring_slots(uint32_t max_bounces) { return 3u * max_bounces + 2u; }
// rpt_paths's 32-bit work counter: a wave's last claim may overshoot the end by its batch (kernels/paths.inc fetch_item), so
// a caller's RptSceneOptions::paths_batch is capped, and render_plan.h's item_limit leaves WAVES_PER_CU_MAX x (64 + BATCH_MAX)
// items of room per CU (one-wave blocks: the occupancy query's answer is clamped to the same bound)
#define RPT_PATHS_BATCH_MAX 1024u
#define RPT_PATHS_WAVES_PER_CU_MAX 32u
// the wavefront pipeline's passes: at most this many paths in flight (32-bit slot indices, queue counters and grids have
// room for 2^31), and at most this share of the device's free memory for their state
#ifndef RPT_MAX_PATHS_PER_PASS
#define RPT_MAX_PATHS_PER_PASS (512ull << 20)
#endif
#ifndef RPT_WS_FREE_PERCENT
#define RPT_WS_FREE_PERCENT 85
#endif
