// kernels/launch.inc — explicit instantiations, host-side launchers and the KernelTable.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ launchers (host pass only)
// rocPRIM's radix sort is instantiated by this call, so the call has to be seen by the device pass as
// well as the host pass (the launchers below are host-pass only)
static hipError_t sort_pairs(void* tmp, size_t& bytes, uint32_t* kin, uint32_t* kout, uint32_t* vin, uint32_t* vout,
                             uint32_t n, hipStream_t st) {
  // all 24 key bits (three passes): sorting without the fine cell (19 bits) or without fine cell and octant (16 bits, 2
  // passes) saves less in the sort than the traversal loses (round 3: wine glass 632 -> 634 / 613, C3 stand-in 197 -> 195 / 193)
#ifndef RPT_SORT_BEGIN_BIT
#define RPT_SORT_BEGIN_BIT 0u // A/B builds: 6 = without the fine cell (18 bits), 8 = two 8-bit passes (coarse cell + the octant's top bit)
#endif
  return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, (unsigned)RPT_SORT_BEGIN_BIT, SORT_KEY_BITS, st);
}
size_t sort_temp_bytes(uint32_t n) {
  size_t bytes = 0;
  (void)sort_pairs(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, n, (hipStream_t)0);
  return bytes;
}

#if !defined(__HIP_DEVICE_COMPILE__)
static inline dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }
static inline dim3 grid_push(uint64_t n) { return dim3((unsigned)((n + PUSH_BLOCK - 1) / PUSH_BLOCK)); } // block_queue_push kernels

void launch_raygen(hipStream_t st, const Frame& fr, const Camera& cam, const PathState& ps, uint32_t n_paths) {
  hipLaunchKernelGGL(rpt_raygen, grid_for(n_paths), dim3(256), 0, st, fr, cam, ps, n_paths);
}
void launch_raygen_rays(hipStream_t st, const Frame& fr, const double* origins, const double* dirs, uint32_t first_draw,
                        uint32_t* ids_out, uint32_t id_base, const PathState& ps, uint32_t n_paths) {
  hipLaunchKernelGGL(rpt_raygen_rays, grid_for(n_paths), dim3(256), 0, st, fr, origins, dirs, first_draw, ids_out, id_base, ps, n_paths);
}
void launch_raygen_probes(hipStream_t st, const Frame& fr, const double* positions, const double* normals, uint32_t kind,
                          uint32_t* ids_out, uint32_t id_base, const PathState& ps, uint32_t n_paths) {
  hipLaunchKernelGGL(rpt_raygen_probes, grid_for(n_paths), dim3(256), 0, st, fr, positions, normals, kind, ids_out, id_base, ps, n_paths);
}
void launch_raygen_views(hipStream_t st, const Frame& fr, const View* views, uint32_t width, uint32_t height, uint64_t j_base,
                         uint32_t* ids_out, const PathState& ps, uint32_t n_paths) {
  hipLaunchKernelGGL(rpt_raygen_views, grid_for(n_paths), dim3(256), 0, st, fr, views, width, height, j_base, ids_out, ps, n_paths);
}
void launch_raygen_views_seeded(hipStream_t st, const Frame& fr, const View* views, uint32_t width, uint32_t height, uint64_t j_base,
                                uint32_t* ids_out, const uint64_t* view_seeds, uint64_t* seeds_out, uint32_t p_lo, uint32_t p_len,
                                const PathState& ps, uint32_t n_paths) {
  hipLaunchKernelGGL(rpt_raygen_views_seeded, grid_for(n_paths), dim3(256), 0, st, fr, views, width, height, j_base, ids_out,
                     view_seeds, seeds_out, p_lo, p_len, ps, n_paths);
}
void launch_extend(hipStream_t st, const Scene& sc, const PathState& ps, const uint32_t* queue, uint32_t n) {
  hipLaunchKernelGGL(rpt_extend, grid_for(n), dim3(256), 0, st, sc, ps, queue, n);
}
void launch_extend_rays(hipStream_t st, const Scene& sc, const double* o, const double* d, uint64_t n,
                        double* out_t, double* out_n, int32_t* out_obj) {
  hipLaunchKernelGGL(rpt_extend_rays, grid_for(n), dim3(256), 0, st, sc, o, d, n, out_t, out_n, out_obj);
}
void launch_shade(hipStream_t st, const Scene& sc, const Frame& fr, const PathState& ps, const uint32_t* queue,
                  uint32_t n, uint32_t depth, uint32_t* next_queue, uint32_t* counters, uint32_t* sq, uint32_t* zero_next,
                  uint32_t zero_n, uint32_t rec_off) {
  hipLaunchKernelGGL(rpt_shade, dim3((unsigned)((n + SHADE_BLOCK - 1) / SHADE_BLOCK)), dim3(SHADE_BLOCK), 0, st, sc, fr, ps, queue, n, depth,
                     next_queue, counters, sq, zero_next, zero_n, rec_off);
}
void launch_shade_seeded(hipStream_t st, const Scene& sc, const Frame& fr, const PathState& ps, const uint32_t* queue,
                         uint32_t n, uint32_t depth, uint32_t* next_queue, uint32_t* counters, uint32_t* sq, uint32_t* zero_next,
                         uint32_t zero_n, uint32_t rec_off, const uint64_t* seeds) {
  hipLaunchKernelGGL(rpt_shade_seeded, dim3((unsigned)((n + SHADE_BLOCK - 1) / SHADE_BLOCK)), dim3(SHADE_BLOCK), 0, st, sc, fr, ps, queue, n,
                     depth, next_queue, counters, sq, zero_next, zero_n, rec_off, seeds);
}
// visibility of ONE light for the paths in its shadow-ray queue, whole scene in the kernel (n: host-side bound of the queue length)
void launch_shadow_rays(hipStream_t st, const Scene& sc, const PathState& ps, const uint32_t* sq_all, const uint32_t* sq_counts,
                        uint32_t n_max, int num_lights, double* srt) {
  hipLaunchKernelGGL(rpt_shadow_rays, dim3(grid_for(n_max).x, (unsigned)num_lights), dim3(256), 0, st, sc, ps, sq_all, sq_counts, srt);
}
void launch_resolve(hipStream_t st, const Frame& fr, const PathState& ps, uint32_t n_samples) {
  hipLaunchKernelGGL(rpt_resolve, grid_for(fr.npix), dim3(256), 0, st, fr, ps, n_samples);
}
void launch_resolve_probes(hipStream_t st, const Frame& fr, const PathState& ps, uint32_t n_samples, uint32_t kind) {
  hipLaunchKernelGGL(rpt_resolve_probes, grid_for(fr.npix), dim3(256), 0, st, fr, ps, n_samples, kind);
}
void launch_finish_probes(hipStream_t st, const Frame& fr, uint32_t width, double scale, double* out) {
  hipLaunchKernelGGL(rpt_finish_probes, grid_for((uint64_t)fr.npix * width), dim3(256), 0, st, fr, width, scale, out);
}
void launch_finish(hipStream_t st, const Frame& fr, double iterations, double ev_scale, void* out, bool f32, bool packed) {
  if (f32)
    hipLaunchKernelGGL(rpt_finish<float>, grid_for(fr.npix), dim3(256), 0, st, fr, iterations, ev_scale, (float*)out, packed ? 1 : 0);
  else
    hipLaunchKernelGGL(rpt_finish<double>, grid_for(fr.npix), dim3(256), 0, st, fr, iterations, ev_scale, (double*)out, packed ? 1 : 0);
}
void launch_scatter_f32(hipStream_t st, const float* src, const uint32_t* pixels, uint32_t n, float* dst) {
  if (n) hipLaunchKernelGGL(rpt_scatter_f32, grid_for(n), dim3(256), 0, st, src, pixels, n, dst);
}

// paths_kernel, paths_max_blocks_per_cu, launch_paths: kernels/launch_paths.inc, shared with the other forms' translation
// units
#define RPT_PATHS_FORM RPT_PATHS_FORM_CAMERA
#include "launch_paths.inc"
#undef RPT_PATHS_FORM
void launch_sum_samples(hipStream_t st, const Frame& fr, const double* lbuf, uint32_t spp, bool first) {
  hipLaunchKernelGGL(rpt_sum_samples, grid_for(fr.npix), dim3(256), 0, st, fr, lbuf, spp, first ? 1 : 0);
}

static RayBatch make_batch(const PathState& ps, int light, double* srt, const uint32_t* n_dev) {
  RayBatch rb{};
  rb.o = ps.ray; rb.o_stride = ps.cap;
  if (light < 0) { // closest-hit rays of the depth
    rb.d = ps.ray + 3 * ps.cap; rb.d_stride = ps.cap;
    rb.rt = ps.hit; rb.rn = ps.hit + ps.cap; rb.n_stride = ps.cap; rb.obj = ps.hit_obj;
  } else { // shadow rays towards light `light`: origin = hit point, direction = wi, stop at dist
    const double* sh = ps.shadow + (uint64_t)light * SHADOW_FIELDS * ps.cap;
    rb.d = sh; rb.d_stride = ps.cap;
    rb.rt = srt + (uint64_t)light * ps.cap;
    rb.dist = sh + 3 * ps.cap;
    rb.n_dev = n_dev;
  }
  return rb;
}
// one query of the depth, object by object (light < 0: closest hit over the path queue; else: visibility of that light
// over ITS shadow-ray queue, whose length n_dev lives on the device and is at most n).
// Launches per query: one per run of shallow objects (rpt_rays_objects) and, per deep tree, rpt_tree_enter, the sort
// (rocPRIM: ~10 launches and memsets — only for queries of at least qt.sort_min_rays rays), the traversal launch (a second
// one, for the rays with a zero direction component, only in scenes where those are common) and rpt_tree_generic.  The records are initialised by the first kernel of the query
// (RayBatch::init) and each tree's five counters by the rpt_tree_generic launch of the pair before it: the pairs
// alternate between two sets (qt.ctr_set, carried from query to query by the caller; both sets start cleared).
void launch_query(hipStream_t st, const Scene& sc, const PathState& ps, const uint32_t* queue, uint32_t n, int light,
                  double* srt, const uint32_t* n_dev, const uint8_t* obj_deep, const uint8_t* obj_tris, int num_objects, uint32_t* tq,
                  uint32_t* tq_ctr, uint32_t trace_blocks, const SortBufs* sb, const QueryHook* hook, const StackSpill* spill,
                  QueryTuning* qt) {
  RayBatch rb = make_batch(ps, light, srt, n_dev);
  auto mark = [&](int kind, int end) { if (hook && hook->mark) hook->mark(hook->ctx, kind, end); };

  const bool shadow = light >= 0;
  dim3 g = grid_for(n), b(256);
  rb.init = 1u;
  int i = 0;
  while (i < num_objects) {
    if (obj_deep[i]) {
      // a tree larger than the L2s: sort its rays first (RPT_DEEP_SORT_CLOSEST: its closest-hit rays only, scene_plan.h route_object) — unless the query
      // is small: below ~10^6 rays rocPRIM sorts by merging, a dozen launches of 5 us each for a traversal of well
      // under a millisecond (the late depths of a long path: 42 of the wine glass's 68 sorts per step).  The default
      // threshold is 2^19 rays: with the queries sized for the rays there are (round 5), 2^20 left the 100k-triangle
      // mesh's mid-size shadow queries unsorted (215.9 -> 218.0 Msamples/s at 2^19; the 16k-triangle glass does not care)
      const SortBufs* sort = (obj_deep[i] & RPT_DEEP_ROUTE) == RPT_DEEP_SORTED && !(shadow && (obj_deep[i] & RPT_DEEP_SORT_CLOSEST)) && n >= qt->sort_min_rays ? sb : nullptr;
      uint32_t* keys = sort ? sort->keys_in : nullptr;
      uint32_t* enter_q = sort ? sort->vals_in : tq; // tree_enter fills (keys_in, vals_in), the sort fills tq
      mark(RPT_K_TREE_SORT, 0);
      // ctr: [0] count, [1] head of the tree's queue; [2] count, [3] head of the queue of its rays with a zero
      // direction component (zq, the second third of tq); [4] count of the rays handed on to rpt_tree_generic (fq, the last)
      uint32_t* ctr = tq_ctr + 8u * qt->ctr_set;
      uint32_t* ctr_next = tq_ctr + 8u * (qt->ctr_set ^ 1u);
      qt->ctr_set ^= 1u;
      uint32_t* zq = tq + ps.cap;
      uint32_t* fq = tq + 2 * ps.cap;
      // rays with a zero direction component: the tree's second queue and a launch of the ZEROS form where the scene
      // makes them common, else the general form's queue (kernels/tree_trace.inc, rpt_tree_trace).  A kd-tree of kd-trees
      // (rpt_nest_trace) takes them in its own loop, whose node step is the general compact one.
      const bool nest = (obj_tris[i] & RPT_TRACE_KIND) == RPT_TRACE_NEST && !sc.force_general; // (scene_plan.h route_object: which objects qualify; extended-shape builds only)
      const bool zeros_launch = spill->zeros_common || nest;
      const uint32_t ztg = zeros_launch ? 0u : 1u;
      if (shadow) hipLaunchKernelGGL(rpt_tree_enter<true>, grid_push(n), dim3(PUSH_BLOCK), 0, st, sc, rb, queue, n, i, enter_q, ctr, keys, zq, ctr + 2, fq, ctr + 4, spill->rays, ztg);
      else hipLaunchKernelGGL(rpt_tree_enter<false>, grid_push(n), dim3(PUSH_BLOCK), 0, st, sc, rb, queue, n, i, enter_q, ctr, keys, zq, ctr + 2, fq, ctr + 4, spill->rays, ztg);
      rb.init = 0u;
      if (sort) { // the entering rays' (key, position) pairs, as many as there are (the one host wait of a sorted query)
        uint32_t n_enter = 0;
        (void)hipMemcpyAsync(&n_enter, ctr, sizeof n_enter, hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
        size_t bytes = sort->tmp_bytes;
        if (n_enter) (void)sort_pairs(sort->tmp, bytes, sort->keys_in, sort->keys_out, sort->vals_in, tq, std::min(n_enter, n), st);
      }
      mark(RPT_K_TREE_SORT, 1);
      mark(RPT_K_TREE_TRACE, 0);
      dim3 tg(trace_blocks / 4 * RPT_TT_WAVES);
      if ((obj_tris[i] & RPT_TRACE_KIND) == RPT_TRACE_GENERIC) { // an object only rpt_tree_generic walks: rpt_tree_enter handed it every ray (fq)
      } else if ((obj_tris[i] & RPT_TRACE_KIND) == RPT_TRACE_MESH) {
        if (shadow) hipLaunchKernelGGL((rpt_tree_trace<true, true, false>), tg, b, 0, st, sc, rb, i, queue, tq, ctr, ctr + 1, nullptr, nullptr, *spill);
        else hipLaunchKernelGGL((rpt_tree_trace<true, false, false>), tg, b, 0, st, sc, rb, i, queue, tq, ctr, ctr + 1, nullptr, nullptr, *spill);
#ifdef RPT_EXT_SHAPES
      } else if (nest) { // a kd-tree of kd-trees: both levels in one loop, both queues in one launch (rpt_nest_trace)
        if (shadow) hipLaunchKernelGGL(rpt_nest_trace<true>, tg, b, 0, st, sc, rb, i, queue, tq, zq, ctr, fq, *spill);
        else hipLaunchKernelGGL(rpt_nest_trace<false>, tg, b, 0, st, sc, rb, i, queue, tq, zq, ctr, fq, *spill);
#endif
      } else {
        if (shadow) hipLaunchKernelGGL((rpt_tree_trace<false, true, false>), tg, b, 0, st, sc, rb, i, queue, tq, ctr, ctr + 1, nullptr, nullptr, *spill);
        else hipLaunchKernelGGL((rpt_tree_trace<false, false, false>), tg, b, 0, st, sc, rb, i, queue, tq, ctr, ctr + 1, nullptr, nullptr, *spill);
      }
      if (zeros_launch && !nest && (obj_tris[i] & RPT_TRACE_KIND) != RPT_TRACE_GENERIC) {
        if ((obj_tris[i] & RPT_TRACE_KIND) == RPT_TRACE_MESH) {
          if (shadow) hipLaunchKernelGGL((rpt_tree_trace<true, true, true>), tg, b, 0, st, sc, rb, i, queue, zq, ctr + 2, ctr + 3, fq, ctr + 4, *spill);
          else hipLaunchKernelGGL((rpt_tree_trace<true, false, true>), tg, b, 0, st, sc, rb, i, queue, zq, ctr + 2, ctr + 3, fq, ctr + 4, *spill);
        } else {
          if (shadow) hipLaunchKernelGGL((rpt_tree_trace<false, true, true>), tg, b, 0, st, sc, rb, i, queue, zq, ctr + 2, ctr + 3, fq, ctr + 4, *spill);
          else hipLaunchKernelGGL((rpt_tree_trace<false, false, true>), tg, b, 0, st, sc, rb, i, queue, zq, ctr + 2, ctr + 3, fq, ctr + 4, *spill);
        }
      }
      {
        // a handful of rays (0/0 splits) unless ALL the object's rays come here (RPT_DEEP_ALL_GENERIC: an irregular tree, an
        // object only rpt_tree_generic is built for) or the general form is forced
        const dim3 gg(((obj_deep[i] & RPT_DEEP_ALL_GENERIC) || sc.force_general) ? spill->gen_blocks_all : spill->gen_blocks_few);
        if (shadow) hipLaunchKernelGGL(rpt_tree_generic<true>, gg, b, 0, st, sc, rb, i, fq, ctr + 4, spill->gen, spill->gen_overflow, ctr_next);
        else hipLaunchKernelGGL(rpt_tree_generic<false>, gg, b, 0, st, sc, rb, i, fq, ctr + 4, spill->gen, spill->gen_overflow, ctr_next);
      }
      mark(RPT_K_TREE_TRACE, 1);
      i++;
    } else {
      int j = i;
      bool flat_run = !sc.force_general; // every object of the run is a primitive or a one-leaf tree (RPT_TRIS_ONE_LEAF)
      while (j < num_objects && !obj_deep[j]) { flat_run = flat_run && (obj_tris[j] & RPT_TRIS_ONE_LEAF) != 0; j++; }
      if (flat_run) {
        if (shadow) hipLaunchKernelGGL((rpt_rays_objects<true, KdFlat>), g, b, 0, st, sc, rb, queue, n, i, j);
        else hipLaunchKernelGGL((rpt_rays_objects<false, KdFlat>), g, b, 0, st, sc, rb, queue, n, i, j);
      } else {
        if (shadow) hipLaunchKernelGGL((rpt_rays_objects<true, KdLdsW>), g, b, 0, st, sc, rb, queue, n, i, j);
        else hipLaunchKernelGGL((rpt_rays_objects<false, KdLdsW>), g, b, 0, st, sc, rb, queue, n, i, j);
      }
      rb.init = 0u;
      i = j;
    }
  }
}
void launch_shadow_sum(hipStream_t st, const Scene& sc, const PathState& ps, const uint32_t* queue, uint32_t n,
                       uint32_t rec_off, const double* srt) {
  hipLaunchKernelGGL(rpt_shadow_sum, grid_for(n), dim3(256), 0, st, sc, ps, queue, n, rec_off, srt);
}

// the next depth's paths (rows and keys written by rpt_shade: PathState::next_rows / sort_keys, n of them) into the CURRENT
// state arrays — in the order of their keys (`sorted`), or as they stand.  `order`: n words of scratch for the sorted
// positions.  Enqueued behind the depth's shadow queries, which still read the current arrays.
void launch_path_reorder(hipStream_t st, const PathState& ps, uint32_t n, bool sorted, const SortBufs* sb, uint32_t* order) {
  if (sorted) {
    size_t bytes = sb->tmp_bytes;
    (void)sort_pairs(sb->tmp, bytes, sb->keys_in, sb->keys_out, sb->vals_in, order, n, st);
  }
  hipLaunchKernelGGL(rpt_path_permute, grid_for(n), dim3(256), 0, st, ps, n, sorted ? order : nullptr);
}

void launch_buffer_accumulate(hipStream_t st, double* total, double* frame, const double* packed, const uint32_t* list,
                              uint32_t n, uint32_t* counts, double* mean, double* m2) {
  if (n) hipLaunchKernelGGL(rpt_buffer_accumulate, grid_for(n), dim3(256), 0, st, total, frame, packed, list, n, counts, mean, m2);
}
void launch_buffer_retire(hipStream_t st, const uint32_t* list, uint32_t n, const uint32_t* counts, const double* mean,
                          const double* m2, uint32_t min_batches, double abs_tol, double rel_tol, uint8_t* keep,
                          uint32_t* block_cnt, uint32_t* out_list, uint32_t* out_n) {
  if (!n) return;
  const dim3 grid((n + RPT_RETIRE_TILE - 1) / RPT_RETIRE_TILE);
  hipLaunchKernelGGL(rpt_retire_count, grid, dim3(256), 0, st, list, n, counts, mean, m2, min_batches, abs_tol, rel_tol,
                     keep, block_cnt);
  hipLaunchKernelGGL(rpt_retire_scatter, grid, dim3(256), 0, st, list, n, (const uint8_t*)keep, (const uint32_t*)block_cnt,
                     out_list, out_n);
}
void launch_buffer_image(hipStream_t st, const double* total, const uint32_t* counts, uint32_t w, uint32_t h,
                         uint32_t radius, const double* thr, uint8_t* out) {
  hipLaunchKernelGGL(rpt_buffer_image, grid_for((uint64_t)w * h), dim3(256), 0, st, total, counts, w, h, radius, thr, out);
}
void launch_buffer_variance(hipStream_t st, const double* total, const double* const* batches, const uint32_t* counts,
                            uint64_t npix, double* out) {
  hipLaunchKernelGGL(rpt_buffer_variance, grid_for(npix), dim3(256), 0, st, total, batches, counts, npix, out);
}

void launch_eval_math(hipStream_t st, int fn, uint64_t n, const double* x, const double* y, double* out) {
  hipLaunchKernelGGL(rpt_eval_math, grid_for(n), dim3(256), 0, st, fn, n, x, y, out);
}

void launch_aov(hipStream_t st, const Scene& sc, const Frame& fr, const Camera& cam, const AovOut& out, uint32_t iterations) {
  hipLaunchKernelGGL(rpt_aov, grid_for(fr.npix), dim3(256), 0, st, sc, fr, cam, out, iterations);
}
void launch_aov_fold(hipStream_t st, const Scene& sc, const Frame& fr, const PathState& ps, const AovOut& out, uint32_t spp,
                     bool first) {
  hipLaunchKernelGGL(rpt_aov_fold, grid_for(fr.npix), dim3(256), 0, st, sc, fr, ps, out, spp, first ? 1 : 0);
}

// rptgpu_occluded / rptgpu_bake_ao (kernels/occlusion.inc): rays into light 0's shadow-ray state, answers out of srt
void launch_occ_load(hipStream_t st, const double* origins, const double* dirs, const double* max_t, const PathState& ps,
                     uint32_t* sq, uint32_t* sq_count, uint32_t n) {
  hipLaunchKernelGGL(rpt_occ_load, grid_for(n), dim3(256), 0, st, origins, dirs, max_t, ps, sq, sq_count, n);
}
void launch_raygen_ao(hipStream_t st, const Frame& fr, const double* positions, const double* normals, const uint32_t* ids,
                      uint32_t id_base, double max_distance, const PathState& ps, uint32_t* sq, uint32_t* sq_count, uint32_t n_slots) {
  hipLaunchKernelGGL(rpt_raygen_ao, grid_for(n_slots), dim3(256), 0, st, fr, positions, normals, ids, id_base, max_distance, ps, sq,
                     sq_count, n_slots);
}
void launch_occ_store(hipStream_t st, const PathState& ps, const double* srt, uint32_t n, uint8_t* out) {
  hipLaunchKernelGGL(rpt_occ_store, grid_for(n), dim3(256), 0, st, ps, srt, n, out);
}
void launch_ao_fold(hipStream_t st, const Frame& fr, const PathState& ps, const double* srt, uint32_t n_samples, bool first,
                    bool last, uint32_t samples, double* out_ao, double* out_bent) {
  hipLaunchKernelGGL(rpt_ao_fold, grid_for(fr.npix), dim3(256), 0, st, fr, ps, srt, n_samples, first ? 1 : 0, last ? 1 : 0, samples,
                     out_ao, out_bent);
}

// rptgpu_bake_direct (kernels/direct.inc): every light's sample of a slot into the shadow-ray state, the fold out of srt
void launch_raygen_direct(hipStream_t st, const Scene& sc, const Frame& fr, const double* positions, const double* normals,
                          const uint32_t* ids, uint32_t id_base, const PathState& ps, uint32_t* sq, uint32_t* counters,
                          uint32_t n_slots) {
  // (a thread takes DIRECT_GROUPS slots: its wave's runs of 64)
  hipLaunchKernelGGL(rpt_raygen_direct, grid_for(((uint64_t)n_slots + DIRECT_GROUPS - 1) / DIRECT_GROUPS), dim3(256), 0, st, sc, fr,
                     positions, normals, ids, id_base, ps, sq, counters, n_slots);
}
void launch_direct_fold(hipStream_t st, const Scene& sc, const Frame& fr, const PathState& ps, const double* srt,
                        uint32_t n_samples, bool first, bool last, uint32_t samples, double* out) {
  hipLaunchKernelGGL(rpt_direct_fold, grid_for(fr.npix), dim3(256), 0, st, sc, fr, ps, srt, n_samples, first ? 1 : 0,
                     last ? 1 : 0, samples, out);
}

// rptgpu_first_hits / rptgpu_render_views_aov (kernels/hits.inc): the closest-hit record into the caller's layout
void launch_first_hits(hipStream_t st, const Scene& sc, const double* origins, const double* dirs, uint32_t n, const HitOut& out) {
  hipLaunchKernelGGL(rpt_first_hits, grid_for(n), dim3(256), 0, st, sc, origins, dirs, n, out);
}
void launch_hits_store(hipStream_t st, const Scene& sc, const PathState& ps, uint32_t n, const HitOut& out) {
  hipLaunchKernelGGL(rpt_hits_store, grid_for(n), dim3(256), 0, st, sc, ps, n, out);
}
void launch_views_aov_fold(hipStream_t st, const Scene& sc, const PathState& ps, const AovOut& out, uint32_t n, uint32_t spp,
                           bool first) {
  hipLaunchKernelGGL(rpt_views_aov_fold, grid_for(n), dim3(256), 0, st, sc, ps, out, n, spp, first ? 1 : 0);
}

// rptgpu_trace_vertices (kernels/wf_vertices.inc): a pass's vertices into the caller's layout
void launch_vertices_store(hipStream_t st, const Frame& fr, const PathState& ps, uint32_t n, uint32_t depth, const VertexOut& out) {
  hipLaunchKernelGGL(rpt_vertices_store, grid_for(n), dim3(256), 0, st, fr, ps, n, depth, out);
}
void launch_vertices_fold(hipStream_t st, const Frame& fr, const PathState& ps, uint32_t n_paths, const VertexOut& out) {
  hipLaunchKernelGGL(rpt_vertices_fold, grid_for(n_paths), dim3(256), 0, st, fr, ps, n_paths, out);
}

// blocks of 64 x 4 pixels: a wave is 64 consecutive x of one row (kernels/denoise.inc)
static inline dim3 grid_rows(uint32_t w, uint32_t h) { return dim3((w + 63u) / 64u, (h + 3u) / 4u); }
void launch_denoise_prepare(hipStream_t st, const double* total, const uint32_t* counts, const double* m2, const AovOut& feat,
                            uint32_t w, uint32_t h, uint64_t stride, double* c_out, double* v_out, double* g_normal,
                            double* g_position, double* g_albedo, double* g_depth, uint8_t* g_hit) {
  hipLaunchKernelGGL(rpt_denoise_prepare, grid_rows(w, h), dim3(64, 4), 0, st, total, counts, m2, feat, w, h, stride, c_out, v_out,
                     g_normal, g_position, g_albedo, g_depth, g_hit);
}
void launch_denoise_level(hipStream_t st, const DenoiseGuide& g, const double* c_in, const double* v_in, double* c_out,
                          double* v_out, uint32_t step, const DenoiseSigmas& sg) {
  hipLaunchKernelGGL(rpt_denoise_level, grid_rows(g.width, g.height), dim3(64, 4), 0, st, g, c_in, v_in, c_out, v_out, step, sg);
}
void launch_denoise_finish(hipStream_t st, const double* c_in, uint64_t stride, uint64_t npix, const double* thr,
                           double* out_linear, uint8_t* out_rgb8) {
  hipLaunchKernelGGL(rpt_denoise_finish, grid_for(npix), dim3(256), 0, st, c_in, stride, npix, thr, out_linear, out_rgb8);
}
// the same over a batch of views: the view in blockIdx.z, at most 65535 views per launch
constexpr uint64_t DN_VIEWS_PER_LAUNCH = 65535u;
void launch_denoise_views_prepare(hipStream_t st, const double* total, const uint32_t* counts, const double* m2, const AovOut& feat,
                                  uint32_t w, uint32_t h, uint64_t n_views, uint64_t stride, double* c_out, double* v_out,
                                  double* g_normal, double* g_position, double* g_albedo, double* g_depth, uint8_t* g_hit) {
  for (uint64_t v0 = 0; v0 < n_views; v0 += DN_VIEWS_PER_LAUNCH) {
    dim3 grid = grid_rows(w, h);
    grid.z = (unsigned)std::min(DN_VIEWS_PER_LAUNCH, n_views - v0);
    hipLaunchKernelGGL(rpt_denoise_views_prepare, grid, dim3(64, 4), 0, st, total, counts, m2, feat, w, h, stride, c_out, v_out,
                       g_normal, g_position, g_albedo, g_depth, g_hit, (uint32_t)v0);
  }
}
void launch_denoise_views_level(hipStream_t st, const DenoiseGuide& g, uint64_t n_views, const double* c_in, const double* v_in,
                                double* c_out, double* v_out, uint32_t step, const DenoiseSigmas& sg) {
  for (uint64_t v0 = 0; v0 < n_views; v0 += DN_VIEWS_PER_LAUNCH) {
    dim3 grid = grid_rows(g.width, g.height);
    grid.z = (unsigned)std::min(DN_VIEWS_PER_LAUNCH, n_views - v0);
    hipLaunchKernelGGL(rpt_denoise_views_level, grid, dim3(64, 4), 0, st, g, c_in, v_in, c_out, v_out, step, sg, (uint32_t)v0);
  }
}
void launch_denoise_views_finish(hipStream_t st, const double* c_in, uint64_t stride, uint64_t n, const double* thr,
                                 double* out_linear, uint8_t* out_rgb8, const double* total, const uint32_t* counts,
                                 const double* m2, double* out_mean, double* out_variance) {
  hipLaunchKernelGGL(rpt_denoise_views_finish, grid_for(n), dim3(256), 0, st, c_in, stride, n, thr, out_linear, out_rgb8, total,
                     counts, m2, out_mean, out_variance);
}

// debug builds with -DRPT_PROF: the per-phase table of kernels/prof.inc accumulated so far (and reset):
// out[0] wave cycles, [1] lane cycles, [2] wave iterations, [3] lane iterations, PROF_SLOTS slots each
bool read_prof(unsigned long long out[4][30]) {
  static_assert(PROF_SLOTS == 30, "kernels.h declares the table with 30 slots");
#ifdef RPT_PROF
  static unsigned long long zero[4][PROF_SLOTS];
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof zero) != hipSuccess) return false;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prof), zero, sizeof zero);
  return true;
#else
  (void)out;
  return false;
#endif
}

// the persistent kernel's forms, in the order of RPT_PATHS_FORM_* (kernels.h): this translation unit's rpt_paths, then the
// forms' own translation units
static const PathsForm PATHS_FORMS[] = {{paths_max_blocks_per_cu, launch_paths},
                                        {RPT_NS_VIEWS::paths_max_blocks_per_cu, RPT_NS_VIEWS::launch_paths},
                                        {RPT_NS_RAYS::paths_max_blocks_per_cu, RPT_NS_RAYS::launch_paths},
                                        {RPT_NS_VERTICES::paths_max_blocks_per_cu, RPT_NS_VERTICES::launch_paths}};
static_assert(sizeof PATHS_FORMS / sizeof PATHS_FORMS[0] == RPT_PATHS_FORM_COUNT, "one element per form of the persistent kernel");
static_assert(RPT_PATHS_FORM_CAMERA == 0 && RPT_PATHS_FORM_VIEWS == 1 && RPT_PATHS_FORM_RAYS == 2 && RPT_PATHS_FORM_VERTICES == 3,
              "PATHS_FORMS is indexed by the form");

const KernelTable TABLE = {launch_raygen, launch_raygen_rays, launch_extend, launch_extend_rays, launch_shade,
                           launch_shadow_rays, launch_resolve, launch_finish, launch_scatter_f32, launch_eval_math,
                           PATHS_FORMS, launch_sum_samples, launch_query, sort_temp_bytes, launch_shadow_sum,
                           launch_buffer_accumulate, launch_buffer_retire, launch_buffer_image, launch_buffer_variance,
                           read_prof, launch_path_reorder, launch_aov, launch_aov_fold,
                           launch_denoise_prepare, launch_denoise_level, launch_denoise_finish,
                           launch_raygen_probes, launch_resolve_probes, launch_finish_probes, launch_raygen_views,
                           launch_occ_load, launch_raygen_ao, launch_occ_store, launch_ao_fold,
                           launch_first_hits, launch_hits_store, launch_views_aov_fold,
                           launch_raygen_views_seeded, launch_shade_seeded,
                           launch_denoise_views_prepare, launch_denoise_views_level, launch_denoise_views_finish,
                           launch_vertices_store, launch_vertices_fold,
                           RPT_NS_VIEWS::launch_views_ids, RPT_NS_RAYS::launch_rays_ids, RPT_NS_RAYS::launch_project_probes,
                           launch_raygen_direct, launch_direct_fold};
#endif // !__HIP_DEVICE_COMPILE__
