// kernels/launch_paths.inc — the choice of the persistent path kernel's instantiation, its occupancy query and its launch: ONE
// text, included once per form of the kernel (RPT_PATHS_FORM, kernels.h) in the form's translation unit — rpt_paths
// (launch.inc), rpt_paths_views (paths_views.inc), rpt_paths_rays (paths_rays.inc), rpt_paths_vertices (paths_vertices.inc).
// Every instance has the signatures of kernels.h's PathsForm and reads its own member of PathsRays.  Host pass only.
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VIEWS
#define RPT_PATHS_FN rpt_paths_views
#define RPT_PATHS_RAYS views
#elif RPT_PATHS_FORM == RPT_PATHS_FORM_RAYS
#define RPT_PATHS_FN rpt_paths_rays
#define RPT_PATHS_RAYS rays
#elif RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
#define RPT_PATHS_FN rpt_paths_vertices
#define RPT_PATHS_RAYS rays
#else
#define RPT_PATHS_FN rpt_paths
#define RPT_PATHS_RAYS cam
#endif
static uint32_t paths_park_off(uint32_t lds_bytes) { return (lds_bytes + 15u) & ~15u; }
// THE choice of rpt_paths' instantiation (occupancy is asked of, and the launch goes to, what this returns).  flat = null:
// RPT_PATHS_FN<KdLds>, which never parks (its stack fills the wave's LDS) — callers clear `park` for it.
static const void* paths_kernel(const FlatLayout* flat, bool park) {
#define RPT_PK(L) (park ? (const void*)RPT_PATHS_FN<L, true> : (const void*)RPT_PATHS_FN<L, false>)
  if (!flat) return (const void*)RPT_PATHS_FN<KdLds, false>;
  if (flat->obj_filter) return RPT_PK(KdFlatF);
#if RPT_FUSE_QUERY && RPT_RAY_STASH >= 2
  // one light that casts shadow rays (the host doubled the quotient table for it): the two-ray form (kernels/paths.inc
  // FUSE), with a hit's scene constants in the wave's tables where the host found room for them
  if (flat->n_tris && flat->fuse_query && !park) {
#if RPT_SCENE_CONSTS
    if (flat->scene_consts) return (const void*)RPT_PATHS_FN<KdFlat, false, true, true>;
#endif
    return (const void*)RPT_PATHS_FN<KdFlat, false, true>;
  }
#endif
  return flat->n_tris ? RPT_PK(KdFlat) : RPT_PK(KdFlatG);
#undef RPT_PK
}
int paths_max_blocks_per_cu(const FlatLayout* flat, uint32_t lds_bytes, bool park) {
  if (!flat) park = false;
  if (park) lds_bytes = paths_park_off(lds_bytes) + RPT_PATHS_PARK_LDS;
  int nb = 0; // per instantiation: their static LDS differs (RPT_PATHS_FN<KdFlat> stashes camera rays)
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, paths_kernel(flat, park), 64, lds_bytes);
  if (e != hipSuccess || nb <= 0) nb = 8;
  return nb;
}
// (l.n_items: npix * ceil(spp / chunk), checked against the 32-bit work counter by the caller)
void launch_paths(hipStream_t st, const Scene& sc, const Frame& fr, const PathsRays& from, const PathsLaunch& l) {
  const bool park = l.flat && l.park; // (RPT_PATHS_FN<KdLds> has no room for the queues)
  // items a wave claims with one atomic on the work counter: 1/32 of its share of the launch, within [16, 256]
  // (RptSceneOptions::paths_batch = 0)
  uint32_t batch = l.batch;
  if (batch == 0u) batch = std::min(256u, std::max(l.n_items / (std::max(1u, l.nblocks) * 32u), 16u));
  batch = std::min(batch, (uint32_t)RPT_PATHS_BATCH_MAX); // a caller's own value: what the host's bound on n_items leaves room for
  PersistArgs pa{l.work_counter, l.rec, l.ray_counters, l.lbuf, l.spp, l.chunk, l.n_items, l.nblocks * 64u,
                 rpt_fold_ring_slots(fr.max_bounces), batch, park ? paths_park_off(l.lds_bytes) : 0xffffffffu, *l.lay};
  const uint32_t lds_bytes = park ? paths_park_off(l.lds_bytes) + RPT_PATHS_PARK_LDS : l.lds_bytes;
#if RPT_PATHS_FORM == RPT_PATHS_FORM_VERTICES
  void* args[] = {(void*)&sc, (void*)&fr, (void*)from.rays, (void*)from.vertices, (void*)&pa}; // the kernel's (Scene, Frame, CallerRays, VertexOut, PersistArgs)
#else
  void* args[] = {(void*)&sc, (void*)&fr, (void*)from.RPT_PATHS_RAYS, (void*)&pa}; // the kernel's (Scene, Frame, Camera | ViewRays | CallerRays, PersistArgs)
#endif
  (void)hipLaunchKernel(paths_kernel(l.flat ? l.lay : nullptr, park), dim3(l.nblocks), dim3(64), args, lds_bytes, st);
}
#undef RPT_PATHS_FN
#undef RPT_PATHS_RAYS
