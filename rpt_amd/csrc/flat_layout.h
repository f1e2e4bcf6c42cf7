// flat_layout.h — the dynamic LDS of the flat path kernel (rpt_paths<KdFlat...>): the build switches and sizes its layout
// depends on, and the layout itself.  Shared by the launchers (kernels.h), the kernels and the scene planner (scene_plan.h,
// which decides every field but the device pointers); free of HIP.
#pragma once
#include <stdint.h>

#include "device_types.h"

// meshes per batched run of the flat path kernel (kernels/paths_flat.inc flat_query; scene_plan.h plan_flat caps Inst::plane_use with it)
#ifndef RPT_FLAT_RUN
#define RPT_FLAT_RUN 6
#endif

// LDS of one wave of rpt_paths: 160 KB per CU / (2 waves per SIMD x 4 SIMDs); the fold walker's static share of it
#define RPT_PATHS_WAVE_LDS 20480u
#define RPT_PATHS_WALKER_LDS 2560u
// rpt_paths<KdFlat> (a flat scene WITH its triangles in LDS) also keeps the lanes' stashed camera rays there
// (kernels/paths.inc RayStash).  RPT_RAY_STASH=2: rpt_paths<KdFlat, false> traces them ahead and stashes their hits
// as well (RayStashHit); 1: rays only; 0: no stash (A/B builds)
#ifndef RPT_RAY_STASH
#define RPT_RAY_STASH 2
#endif
// RPT_FUSE_QUERY=1: rpt_paths<KdFlat, false, true> traces a hit's shadow ray and bounce ray in one two-ray query
// (kernels/paths_flat.inc flat_query2) for a flat scene with a plane table and exactly one light, a non-ambient one (C2);
// the host then keeps a second quotient table behind the first (FlatLayout::fuse_query).  0: the one-ray passes (A/B)
#ifndef RPT_FUSE_QUERY
#define RPT_FUSE_QUERY 1
#endif
// RPT_PRETRACE_CULL=1: in rpt_paths<KdFlat, false, true> under a pinhole camera, the pass that pre-traces a refill's
// camera rays skips, for the whole wave, the exact test of an object outside the plane table when none of the wave's
// pending pixels lies inside the object's screen rectangle (host_scene.cpp pinhole_screen_rect, computed per render from
// the camera: FlatLayout::cull_*; kernels/paths_flat.inc flat_query<false, true>); 0: every object's test in every pass
// (A/B builds).  RPT_CULL_MAX: objects that can carry a rectangle (the first ones that qualify; the others always run)
#ifndef RPT_PRETRACE_CULL
#define RPT_PRETRACE_CULL 1
#endif
#define RPT_CULL_MAX 4
// RPT_SCENE_CONSTS=1: rpt_paths<KdFlat, false, true, true> reads what a hit's shading and the two-cube block derive from
// the scene alone — per object the material's m2, m2 * PI, f0 and 1 - f0, sample_f's lobe probability and gen_bool's
// integer; per triangle of the mesh light Shape::sample's pdf; per cube of a two-cube block its six world normals —
// from tables that every wave fills once, in its prologue, with the loop's own expressions (kernels/paths_consts.inc
// SceneConsts; FlatLayout::scene_consts when the wave's LDS share holds them, else the kernel without them);
// 0: every hit computes them, the parent's loop (A/B builds).  The value is a mask of the groups that are built:
// 1 = the materials' constants, 2 = the light's pdfs, 4 = the cubes' normals.  All three are built: the light's pdfs
// cost the kernel nine more spilled SGPRs (301 against 292), whichever way their table is addressed, and were first
// left out for that — but its spilled scalars are cold, and on top of the pool of pre-traced hits C2 gains 2.2 % with
// them (measured at RPT_POOL_REFILL=48), spreads disjoint (profiles/hit_pool_ab.txt; 1.4 % in profiles/scene_consts_ab.txt)
#ifndef RPT_SCENE_CONSTS
#define RPT_SCENE_CONSTS 7
#endif
// RPT_SHADOW_WINDOW=1: in the two-ray query (kernels/paths_flat.inc flat_query2) the shadow ray drops, right after a run's
// slab tests, every candidate that is an AXIS-FLAT plane-table user (scene_plan.h axis_flat_mesh: a single-leaf untransformed
// mesh that lies in one axis plane: the walls of C2) whose slab entry mm lies beyond the light:
// rpt_shadow_window_beyond(mm, t_stop) below, which implies mm > t_stop * (1 + 2^-40).  Such an object can only be hit
// beyond t_stop, which never changes `rts > t_stop` (the proof stands at scene_plan.h axis_flat_mesh).  The host marks the
// objects in bit 24 of Inst::plane_idx, above the six 4-bit slots.  0: every candidate is walked, the parent's kernels
// instruction for instruction (A/B builds)
#ifndef RPT_SHADOW_WINDOW
#define RPT_SHADOW_WINDOW 1
#endif
#define RPT_PLANE_AXIS_FLAT (1u << 24) // Inst::plane_idx: the object is axis-flat
#if defined(__HIPCC__)
#define RPT_LAYOUT_FN __host__ __device__ inline
#else
#define RPT_LAYOUT_FN inline
#endif
// The rule's comparison, one copy for the kernel and the host check (tests/cpp/shadow_window_check.cpp): mm, which is
// max(q, EPSILON) and so a positive double or +inf, lies more than 2^13 representable doubles above t_stop.  Doubles of one
// sign are ordered like their bit patterns, and 2^13 steps up from a normal t_stop > 0 are at least t_stop * 2^-40, so true
// implies  mm > t_stop * (1 + 2^-40)  for every t_stop that is not a NaN: a t_stop that is subnormal, a zero or negative is
// below EPSILON <= mm; t_stop = +inf and a NaN with a clear sign bit have the larger pattern (false); for DBL_MAX, true needs
// a pattern above +inf's.  A NaN t_stop with its sign bit set may give true: `rts > t_stop` is then false whatever rts is.
// The comparison is made on the patterns because the product t_stop * (1 + 2^-40), one more double alive across the run's
// slab tests, cost the extended views kernel 24 VGPR spills (profiles/shadow_window_ab.txt); this form keeps no value.
RPT_LAYOUT_FN bool rpt_shadow_window_beyond(double mm, double t_stop) {
  uint64_t a, b;
  __builtin_memcpy(&a, &mm, 8);
  __builtin_memcpy(&b, &t_stop, 8);
  return (int64_t)(a - b) > (int64_t)8192;
}
#define RPT_MAT_CONSTS_BYTES 88u   // per object (kernels/paths_consts.inc MatConsts)
#define RPT_CUBE_NORMALS_BYTES 144u // per cube of a two-cube block: [face][3] doubles
#define RPT_PATHS_STASH_LDS 4864u
#define RPT_PATHS_STASH_HIT_LDS 6656u
// RPT_HIT_POOL=1: the fused kernels (rpt_paths<KdFlat, false, true[, true]>) keep their pre-traced camera hits in a
// wave-level FIFO of RPT_POOL_CAP self-contained entries in the place of the per-lane RayStashHit (kernels/paths.inc
// HitPool, index arithmetic: hit_pool.h): any lane shades any hit, and the wave generates and pre-traces only once
// RPT_POOL_REFILL slots are free, or when it must, so a pre-trace pass runs at that many lanes instead of half of them.
// 0: the per-lane stash (A/B builds).  An entry is 100 bytes; the default pool is smaller than the stash it replaces, so
// a scene that fits the per-lane form fits this one (static_assert below: a larger RPT_POOL_CAP has to go through
// the three fit checks of scene_plan.h plan_flat, and a scene without the room has to keep the per-lane form)
#ifndef RPT_HIT_POOL
#define RPT_HIT_POOL 1
#endif
#ifndef RPT_POOL_CAP
#define RPT_POOL_CAP 64u
#endif
#ifndef RPT_POOL_REFILL
#define RPT_POOL_REFILL 56u
#endif
#define RPT_PATHS_POOL_LDS (RPT_POOL_CAP * 100u)
static_assert(RPT_POOL_CAP >= 64u && RPT_POOL_REFILL >= 1u && RPT_POOL_REFILL <= RPT_POOL_CAP,
              "a refill of 64 lanes has to fit an empty pool, and a full pool has to fall to the refill mark");
static_assert(RPT_PATHS_POOL_LDS <= RPT_PATHS_STASH_HIT_LDS, "the host's fit checks leave room for RayStashHit only");
// what the host leaves room for in a KdFlat scene's LDS layout (scene_plan.h plan_flat)
#define RPT_PATHS_STASH_MAX_LDS (RPT_RAY_STASH >= 2 ? RPT_PATHS_STASH_HIT_LDS : RPT_PATHS_STASH_LDS)

// layout of the flat path kernel's dynamic LDS (byte offsets; lrec at 0), see kernels.inc
struct FlatLayout {
  uint32_t off_tris, off_refs, off_mat, off_leaf;
  uint32_t off_end;              // end of the scene's tables (0 for scenes that are not flat)
  uint32_t n_refs, n_tris;
  // distinct bounding-plane coordinates of the untransformed meshes, at most 4 per axis: the quotient
  // (value - o) / d of each is computed ONCE per ray into off_qtab ([distinct planes][64 lanes] doubles) and shared
  // by every mesh whose box uses that plane (the walls of C2 have 30 faces on 6 distinct planes)
  uint32_t off_qtab, plane_cnt;  // plane_cnt: 4 bits per axis; 0 = feature off
  const double* plane_vals;      // [3][4] in device memory
  // the object filter of flat scenes with many objects and no plane table (kernels/paths_flat.inc flat_query_filtered): a
  // conservative 16-bit box per top-level object on a grid over all of them, tested in f32 before the object's own
  // (exact) test; bit k of obj_always = object k is never filtered (a Plane, a mesh with a sliver, ...)
  uint32_t obj_filter;           // 0 = off
  uint32_t off_obox;             // [objects][6] doubles in LDS: the bounds of MESH objects (their exact slab test)
  const rptdev::LeafBox* obj_box; // [objects] in device memory
  const double* obj_grid;        // qlo[3], qscale[3], bounds[6] of the grid, device memory
  uint64_t obj_always;
  // rpt_paths<KdFlat, false, true> (RPT_FUSE_QUERY): the quotient table is doubled, the shadow ray's half right behind
  // the bounce ray's (scene_plan.h plan_flat; kernels/launch.inc selects the fused kernel by it)
  uint32_t fuse_query;
  // rpt_paths<KdFlat, false, true> (RPT_PRETRACE_CULL).  Per scene (scene_plan.h plan_flat): pretrace_cull = some object may be
  // skipped by the pre-trace pass, cull_always = bit k: object k never is (a plane-table user, or exempt from the object
  // filter).  Per render (api_render.cpp, a pinhole camera): cull_n rectangles, cull_obj[j] the object of rectangle j,
  // cull_lo[j] = x0 | y0 << 16 its first pixel and cull_ext[j] = (x1 - x0) | (y1 - y0) << 16 its extent beyond that one
  // (off screen: lo = 0xffffffff, ext = 0, which no pixel of a frame of at most 65535 a side satisfies)
  uint32_t pretrace_cull, cull_n;
  uint64_t cull_always;
  uint32_t cull_obj[RPT_CULL_MAX], cull_lo[RPT_CULL_MAX], cull_ext[RPT_CULL_MAX];
  // rpt_paths<KdFlat, false, true, true> (RPT_SCENE_CONSTS): the wave's tables of per-launch constants behind the quotient
  // tables (scene_plan.h plan_flat; kernels/launch.inc selects the kernel by scene_consts).  off_consts: [objects] MatConsts from
  // there on and [triangles of the light's mesh] doubles behind them; in front of it, back to front, [cubes in two-cube
  // blocks, in object order][6][3] doubles (kernels/paths_consts.inc FlatLds::consts)
  uint32_t scene_consts, off_consts;
};
