// kernels.inc — the gfx950 path tracer.  Compiled twice, each time inside its own namespace RPT_NS, both with
// -ffp-contract=off (IEEE f64, no FMA contraction — the arithmetic of the reference): kernels_strict.hip, and
// kernels_strict_ext.hip with the extended shape set (RPT_EXT_SHAPES: MonomialSurface; rpt_nest_trace for groups with
// mesh children).  api_common.cpp (table_for) picks the table per scene.  The code lives in kernels/:
//
//   vec.inc        3-vectors, divisions, matrix products in nalgebra's operation order
//   prof.inc       -DRPT_PROF builds: wave time, lane time and iteration counts per phase (nothing otherwise)
//   rng.inc        Philox4x32-10 stream + the rand 0.8 / rand_distr 0.4 distributions restated on it
//   shapes.inc     Sphere / Plane / Cube / MonomialSurface / Triangle::intersect, kd-leaf tests
//   traversal.inc  KdTree::intersect (kdtree.rs:129-223) of ONE tree, instance dispatch, closest hit, visibility
//   sampling.inc   Shape::sample, Transformed::sample
//   material.inc   Material::bsdf / sample_f (material.rs:125-313)
//   light.inc      Light::illuminate (light.rs:23-47), Environment / Hdri (environment.rs:25-52)
//   paths*.inc     the DEFAULT pipeline for scenes without deep trees: one persistent kernel,
//                  rpt_paths<KdLds | KdFlat>, the whole path in registers (renderer.rs:117-174), in these files:
//     paths_consts.inc  what a flat scene keeps in the wave's LDS (FlatLds) and the tables of a hit's scene constants
//     paths_flat.inc    the flat scenes' queries: flat_query, flat_query2 (two rays in one walk), flat_query_filtered
//     paths_shade.inc   the fused form's draw-first shading: hit_draws, bsdf_opaque, sample_f_opaque, illuminate_mesh
//     paths.inc         the kernel's contract, work hand-out, record ring, parked lookups, ray stash; rpt_sum_samples
//     paths_loop.inc    the loop itself: one text, compiled once per form of the kernel (RPT_PATHS_FORM_*, kernels.h) — as
//                       rpt_paths by paths.inc and, each in a translation unit of its own, by the three files below
//     paths_views.inc   rpt_paths_views, the kernel over a piece of a batch of views: its ids, camera ray and per-lane key
//     paths_rays.inc    rpt_paths_rays, the kernel over a piece of the caller's rays or light probes: its ray; rpt_rays_ids,
//                       rpt_project_probes
//     paths_vertices.inc rpt_paths_vertices, rpt_paths_rays with the paths' vertices written where the loop has them: its
//                       ray and the three stores of a vertex
//     launch_paths.inc  the host side of a form: which instantiation, its occupancy, its launch — one text, included where
//                       the form's kernel is, with one signature for all forms (kernels.h PathsForm, KernelTable::paths)
//     probe_dir.inc     a light probe's direction and the SH9 basis, shared by both routes of rptgpu_bake_probes
//   the wavefront pipeline — scenes with deep trees; rptgpu_trace_rays and rptgpu_bake_probes for any scene (flat ones
//   query inside rpt_extend / rpt_shadow_rays) —: one kernel per step of a depth over SoA path state, in six files:
//     wf_state.inc      access to the SoA path state and the depth records; the queue appends of a wave and of a block
//     wf_sort_key.inc   the key queued rays and the paths of a depth are sorted by: RPT_SORT_PATTERN, ray_sort_key
//     tree_query.inc    the per-tree query — closest hit or visibility, object by object —: RayBatch, a shadow ray's stop,
//                       the slab interval, the entry row, a hit's epilogue; rpt_rays_objects, rpt_tree_enter
//     tree_trace.inc    its persistent walkers and the steps they share (write-out, queue claim, stack, node step):
//                       rpt_tree_trace, rpt_nest_trace (a kd-tree of kd-trees)
//     tree_generic.inc  rpt_tree_generic: any tree, trees inside trees to any depth
//     wavefront.inc     the path pipeline's kernels: rpt_raygen* / rpt_extend / rpt_shade / rpt_shadow_rays /
//                       rpt_shadow_sum / rpt_resolve* / rpt_finish* / rpt_path_permute
//   buffer.inc     device-resident Buffer (buffer.rs)
//   aov.inc        first-hit feature buffers: rpt_aov (fused) and rpt_aov_fold (behind the per-tree query), DESIGN.md §11
//   denoise.inc    the device Buffer's feature-guided à-trous filter (rpt_denoise_prepare / _level / _finish), DESIGN.md §12,
//                  and, from the same text, the filter over a batch of views (rpt_denoise_views_prepare / _level / _finish), §18
//   occlusion.inc  rptgpu_occluded / rptgpu_bake_ao: the caller's rays into a depth's shadow-ray state and their answers out of it
//                  (rpt_occ_load, rpt_raygen_ao, rpt_occ_store, rpt_ao_fold), DESIGN.md §16
//   direct.inc     rptgpu_bake_direct: sample_lights at the caller's points — every light's sample, contribution and shadow ray of a
//                  (sample, point) slot into a depth's shadow-ray state, and the fold over samples and lights (rpt_raygen_direct,
//                  rpt_direct_fold), DESIGN.md §23
//   hits.inc       rptgpu_first_hits / rptgpu_render_views_aov: the closest-hit record into the caller's layout (rpt_first_hits
//                  fused, rpt_hits_store behind the per-tree query, rpt_views_aov_fold), DESIGN.md §17
//   wf_vertices.inc rptgpu_trace_vertices: the vertices of a wavefront pass's paths into the caller's layout (rpt_vertices_store per
//                  depth, rpt_vertices_fold at the end of the pass), DESIGN.md §19
//   hit_surface.inc rptgpu_hit_surface: the triangle, barycentrics and group child behind a first hit — rpt_hit_surface, a
//                  resolve walk of the hit object alone, in translation units of its own (kernels_surface_strict[_ext].hip), §21
//   launch.inc     explicit instantiations, host-side launchers, the KernelTable the api_*.cpp files call through
//
// Wave64 throughout (gfx950): queue appends and work fetches use one 64-bit ballot + one atomic per wave.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <type_traits>

// a translation unit of one form of the persistent kernel alone (the views': RPT_VIEWS_TU; the caller's rays': RPT_RAYS_TU;
// the caller's rays' with their vertices: RPT_VERTICES_TU)
#if defined(RPT_VIEWS_TU) || defined(RPT_RAYS_TU) || defined(RPT_VERTICES_TU)
#define RPT_FORM_TU 1
#endif
#if !defined(RPT_FORM_TU) && !defined(RPT_SURFACE_TU)
#include <rocprim/device/device_radix_sort.hpp>
#endif

#include "../../include/rpt_gpu.h"
#include "../../include/rpt_math.h"
#include "math_converged.h"
#include "device_types.h"
#include "kernels.h"

namespace RPT_NS {

using namespace rptdev;

#define RPT_DEV __device__ __forceinline__
// the namespace of this build's views' translation unit: RPT_NS + _views (kernels.h declares what launch.inc takes from it)
#define RPT_CAT2_(a, b) a##b
#define RPT_CAT2(a, b) RPT_CAT2_(a, b)
#define RPT_NS_VIEWS RPT_CAT2(RPT_NS, _views)
#define RPT_NS_RAYS RPT_CAT2(RPT_NS, _rays) // ... and of its rays' translation unit
#define RPT_NS_VERTICES RPT_CAT2(RPT_NS, _vertices) // ... and of its vertices' translation unit
// Scene tables that a whole wave indexes uniformly (top-level instances, trees, lights) are read
// through the CONSTANT address space: the scene is immutable while a kernel runs, and only then
// does the compiler turn a uniform-address load into an s_load (SGPR destination, scalar cache)
// instead of a 64-lane vector load into VGPRs — the kernels store to global memory, so plain
// loads are treated as possibly clobbered.  (PMC before: 2.7e8 vector loads vs 2.7e4 scalar.)
#define RPT_C __attribute__((address_space(4)))
using CInst = const RPT_C Inst;
using CTree = const RPT_C Tree;
using CLight = const RPT_C Light;
RPT_DEV CInst& cinst(const Scene& sc, int i) { return *(CInst*)(sc.insts + i); }
RPT_DEV CTree& ctree(const Scene& sc, int i) { return *(CTree*)(sc.trees + i); }
RPT_DEV CLight& clight(const Scene& sc, int i) { return *(CLight*)(sc.lights + i); }

#ifndef RPT_WF_WAVES
#define RPT_WF_WAVES 3 // waves per SIMD of the in-kernel traversal kernels (rpt_extend / rpt_shadow / rpt_rays_objects): 168 VGPRs
                       // instead of 128 (which spilled 74) and 10 instead of 7 stack levels in LDS; 2 / 3 / 4 -> 219 / 261 / 247
                       // Msamples/s on the fractal spheres
#endif
#ifndef RPT_REFILL_BELOW
#define RPT_REFILL_BELOW 8 // persistent traversal: refill a wave when fewer lanes than this still have a ray (2 / 8 / 24 / 40 measured)
#endif
constexpr double INF = __builtin_huge_val();
constexpr double PI = 3.14159265358979323846264338327950288;
constexpr double FRAC_1_PI = 0.318309886183790671537767526745028724;
constexpr double TAU = 6.28318530717958647692528676655900577;
constexpr double EPSILON = 1e-12;       // renderer.rs:14
constexpr double FIREFLY_CLAMP = 100.0; // renderer.rs:15

#include "kernels/vec.inc"
#include "kernels/prof.inc"
#include "kernels/rng.inc"
#include "kernels/shapes.inc"
#include "kernels/traversal.inc"
#if defined(RPT_SURFACE_TU)
// the surface resolve's translation units (kernels_surface_strict[_ext].hip, RPT_NS = rpt_strict[_ext]_surface): the shapes, a
// tree's steps and rpt_hit_surface with its launcher — no path kernel, no table (DESIGN.md §21)
#include "kernels/wf_state.inc"
#include "kernels/wf_sort_key.inc"
#include "kernels/tree_query.inc"
#include "kernels/hit_surface.inc"
#else
#include "kernels/sampling.inc"
#include "kernels/material.inc"
#include "kernels/light.inc"
#ifndef RPT_FORM_TU
#include "kernels/wf_state.inc"
#include "kernels/wf_sort_key.inc"
#include "kernels/tree_query.inc"
#include "kernels/tree_trace.inc"
#include "kernels/tree_generic.inc"
#include "kernels/wavefront.inc"
#endif
#include "kernels/paths_consts.inc"
#include "kernels/paths_flat.inc"
#include "kernels/paths_shade.inc"
#include "kernels/paths.inc"
#if defined(RPT_VERTICES_TU)
// the vertices' translation units (kernels_vertices_strict[_ext].hip, RPT_NS = rpt_strict[_ext]_vertices, the ray stash off):
// rpt_paths_vertices and its launchers (DESIGN.md §19.1)
#include "kernels/paths_vertices.inc"
#elif defined(RPT_RAYS_TU)
// the rays' translation units (kernels_rays_strict[_ext].hip, RPT_NS = rpt_strict[_ext]_rays), in the same way: rpt_paths_rays,
// rpt_rays_ids, rpt_project_probes and their launchers (DESIGN.md §13.1)
#include "kernels/probe_dir.inc"
#include "kernels/paths_rays.inc"
#elif defined(RPT_VIEWS_TU)
// the views' translation units (kernels_views_strict[_ext].hip, RPT_NS = rpt_strict[_ext]_views): what rpt_paths needs, then
// rpt_paths_views, its instantiations and its launchers — and nothing else, so that the code objects of kernels_strict[_ext]
// stay what they were (DESIGN.md §15.2)
#include "kernels/paths_views.inc"
#else
#include "kernels/buffer.inc"
#include "kernels/aov.inc"
// the Buffer's filter kernels and rpt_denoise_views_*: kernels/denoise.inc, once per frame layout (RPT_DN_VIEWS 0: one camera's
// frame; 1: a batch of views, one launch for all of them)
#define RPT_DN_VIEWS 0
#include "kernels/denoise.inc"
#undef RPT_DN_VIEWS
#define RPT_DN_VIEWS 1
#include "kernels/denoise.inc"
#undef RPT_DN_VIEWS
#include "kernels/occlusion.inc"
#include "kernels/direct.inc"
#include "kernels/hits.inc"
#include "kernels/wf_vertices.inc"
#include "kernels/launch.inc"
#endif // RPT_FORM_TU
#endif // RPT_SURFACE_TU

} // namespace RPT_NS
