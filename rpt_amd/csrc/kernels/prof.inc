// kernels/prof.inc — per-phase WAVE time, LANE time and iteration counts (debug builds: -DRPT_PROF).
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).
//
// The SQ counters give one "lanes active per VALU instruction" figure per kernel; they cannot say WHICH phase of a
// kernel runs with idle lanes.  A -DRPT_PROF build (scripts/build_variant.sh prof "-DRPT_PROF") keeps, per wave and
// in LDS, a timeline of the phases the wave passes through:
//   PROF_PHASE(i)  the time since the wave's previous mark is added to phase i — once as wave time and once
//                  multiplied by the number of lanes that are active at the mark (the lanes that ran the phase);
//   PROF_COUNT(i)  one iteration of a loop body: one wave iteration, popcount(exec) lane iterations.
// lane / (64 x wave) is the lane occupancy of the phase: the fraction of VALU lane slots that did useful work there.
// The first active lane does the bookkeeping (a handful of DS operations), so a mark may sit in divergent code.
// Regular builds compile all of this to nothing.
#ifdef RPT_PROF
constexpr int PROF_SLOTS = 30;
struct ProfLds {
  long long mark[4];
  unsigned long long wt[4][PROF_SLOTS], lt[4][PROF_SLOTS]; // wave cycles, lane cycles
  unsigned long long wi[4][PROF_SLOTS], li[4][PROF_SLOTS]; // wave iterations, lane iterations
};
__device__ unsigned long long g_prof[4][PROF_SLOTS];
__device__ __forceinline__ ProfLds* prof_lds() {
  __shared__ ProfLds p;
  return &p;
}
__device__ __forceinline__ void prof_init() { // every wave of the block, before its first mark (blocks of <= 256 threads)
  ProfLds* p = prof_lds();
  const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
  if (l < (uint32_t)PROF_SLOTS) { p->wt[w][l] = 0; p->lt[w][l] = 0; p->wi[w][l] = 0; p->li[w][l] = 0; }
  if (l == 0) p->mark[w] = clock64();
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void prof_phase(int i) {
  const uint64_t ex = __ballot(true);
  if ((threadIdx.x & 63u) == (uint32_t)__ffsll((long long)ex) - 1u) {
    ProfLds* p = prof_lds();
    const uint32_t w = threadIdx.x >> 6;
    const long long t = clock64(), dt = t - p->mark[w];
    p->mark[w] = t;
    p->wt[w][i] += (unsigned long long)dt;
    p->lt[w][i] += (unsigned long long)dt * (unsigned long long)__popcll(ex);
  }
}
__device__ __forceinline__ void prof_count(int i) {
  const uint64_t ex = __ballot(true);
  if ((threadIdx.x & 63u) == (uint32_t)__ffsll((long long)ex) - 1u) {
    ProfLds* p = prof_lds();
    const uint32_t w = threadIdx.x >> 6;
    p->wi[w][i] += 1ull;
    p->li[w][i] += (unsigned long long)__popcll(ex);
  }
}
__device__ __forceinline__ void prof_flush() { // at the end of the kernel, all lanes of the wave
  ProfLds* p = prof_lds();
  const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
  __builtin_amdgcn_wave_barrier();
  if (l < (uint32_t)PROF_SLOTS) {
    if (p->wt[w][l]) atomicAdd(&g_prof[0][l], p->wt[w][l]);
    if (p->lt[w][l]) atomicAdd(&g_prof[1][l], p->lt[w][l]);
    if (p->wi[w][l]) atomicAdd(&g_prof[2][l], p->wi[w][l]);
    if (p->li[w][l]) atomicAdd(&g_prof[3][l], p->li[w][l]);
  }
}
#define PROF_INIT() prof_init()
#define PROF_PHASE(i) prof_phase(i)
#define PROF_COUNT(i) prof_count(i)
#define PROF_FLUSH() prof_flush()
#else
constexpr int PROF_SLOTS = 30;
#define PROF_INIT() do { } while (0)
#define PROF_PHASE(i) do { } while (0)
#define PROF_COUNT(i) do { } while (0)
#define PROF_FLUSH() do { } while (0)
#endif
// slot numbers (names: api_render.cpp, PROF_NAMES)
enum {
  // rpt_tree_trace
  PF_TT_REFILL = 0, PF_TT_NODE = 1, PF_TT_BOX = 2, PF_TT_POP = 3, PF_TT_WRITE = 4, PF_TT_EXACT = 5,
  // traversals inside rpt_extend / rpt_shadow / rpt_rays_objects / rpt_paths<KdLds> (iteration counts only)
  PF_IK_NODE = 6, PF_IK_BOX = 7, PF_IK_CHILD = 8, PF_IK_TRI = 9, PF_IK_OBJECT = 10,
  // rpt_paths
  PF_P_FETCH = 11, PF_P_RAYGEN = 12, PF_P_HIT = 13, PF_P_ILLUM = 14, PF_P_VIS = 15, PF_P_NEE = 16, PF_P_SAMPLE = 17,
  PF_P_BSDF = 18, PF_P_RECORD = 19, PF_P_FOLD = 20,
  // loops inside rpt_paths<KdFlat> (iteration counts only)
  PF_P_CAND = 21, PF_P_FOLDIT = 22, PF_P_REJECT = 23,
  // rpt_paths<KdFlat, false, true>: the two-ray query of a hit's shadow ray and bounce ray (flat_query2)
  PF_P_FUSED = 24,
  // its fast shading form (RPT_SHADE_SPLIT): a hit's draws, the straight-line shading block
  PF_P_DRAWS = 25, PF_P_SHADE = 26,
  // its pre-trace pass (RPT_PRETRACE_CULL; iteration counts only): passes run, passes that skipped the two-cube block
  PF_P_PRETRACE = 27, PF_P_PRECULL = 28,
  // the shadow ray's leaf tests in the table runs of flat_query2 (iteration counts only; RPT_SHADOW_WINDOW drops the ones beyond the light)
  PF_P_SHLEAF = 29
};
