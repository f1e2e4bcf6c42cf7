// kernels/wf_sort_key.inc — the key by which queued rays are sorted before a tree's traversal, and the paths of a depth
// before rpt_extend: RPT_SORT_PATTERN, ray_sort_key, SceneBox.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// Sort key of a ray about to enter a tree: where it enters the tree's box (7-bit Morton code per axis)
// and its direction octant, coarse cell first.  Only the ORDER in which queued rays are traversed
// depends on it — every ray's result is its own — so nothing here needs to be exact.
// The key is built from 3-bit groups, most significant first, as RPT_SORT_PATTERN spells them: 'p' = the next bit (one
// per axis) of the entry cell, 'O' = the direction's octant, 'd' = the next bit per axis of the direction inside its
// octant (|component| / |d|_1).  Keys are 32-bit words and rocPRIM sorts 8 bits per pass: up to ten groups = four passes.
// Rounds 2-5 sorted 24 bits, "pppppOpp" (a 32^3 cell, the octant, a 4^3 cell inside): three passes.  Round 6 measured
// what the order is worth to the traversal (profiles/r06_sort_key_ab.txt) — 16 / 18 / 24 bits of that layout:
// rpt_tree_trace 493 / 484 / 467 ms on the 100k-triangle mesh — and that the DIRECTION is worth more than more cell
// bits: "pppOdddppp" (30 bits, four passes) 434 ms, +4.7 % on the frame after the fourth pass's cost; the 16k-triangle
// glass gains 4.5 % in the traversal and pays it back in the sort (+0.9 % on the frame).
// (Only the rays that ENTER the tree get a key: rpt_tree_enter compacts the pairs, launch_query sorts as many as there are.)
#ifndef RPT_SORT_PATTERN
#if !defined(RPT_SORT_PATTERN_ID)
#define RPT_SORT_PATTERN "pppOdddppp"
#elif RPT_SORT_PATTERN_ID == 0 // (A/B builds: a quoted string does not survive the build scripts' word splitting)
#define RPT_SORT_PATTERN "pppppOpp"
#elif RPT_SORT_PATTERN_ID == 1
#define RPT_SORT_PATTERN "pOpdpdpdpp"
#elif RPT_SORT_PATTERN_ID == 2
#define RPT_SORT_PATTERN "ppOdpdpdpp"
#elif RPT_SORT_PATTERN_ID == 3
#define RPT_SORT_PATTERN "pppOddddpp"
#elif RPT_SORT_PATTERN_ID == 4
#define RPT_SORT_PATTERN "ppOdddpppp"
#elif RPT_SORT_PATTERN_ID == 5
#define RPT_SORT_PATTERN "ppppOdddpp"
#elif RPT_SORT_PATTERN_ID == 6
#define RPT_SORT_PATTERN "pppOddpp"
#elif RPT_SORT_PATTERN_ID == 7
#define RPT_SORT_PATTERN "ppOddppp"
#elif RPT_SORT_PATTERN_ID == 8
#define RPT_SORT_PATTERN "ppppppOddd"
#elif RPT_SORT_PATTERN_ID == 9
#define RPT_SORT_PATTERN "pppppOdddp"
#elif RPT_SORT_PATTERN_ID == 10
#define RPT_SORT_PATTERN "pppppppOdd"
#endif
#endif
constexpr uint32_t sort_pattern_count(char c) {
  uint32_t n = 0;
  for (const char* q = RPT_SORT_PATTERN; *q; q++) n += *q == c ? 1u : 0u;
  return n;
}
constexpr uint32_t SORT_POS_BITS = sort_pattern_count('p'), SORT_DIR_BITS = sort_pattern_count('d');
constexpr uint32_t SORT_KEY_BITS = 3u * (SORT_POS_BITS + SORT_DIR_BITS + sort_pattern_count('O'));
static_assert(SORT_KEY_BITS <= 32u && sort_pattern_count('O') <= 1u && SORT_POS_BITS <= 10u && SORT_DIR_BITS <= 10u, "RPT_SORT_PATTERN");
static_assert(SORT_KEY_BITS == 3u * (sizeof(RPT_SORT_PATTERN) - 1u), "RPT_SORT_PATTERN: only 'p', 'd' and one 'O'");
template <class TreeT> RPT_DEV uint32_t ray_sort_key(const TreeT& tr, D3 o, D3 d, double t_enter) {
  constexpr float CELLS = (float)(1u << SORT_POS_BITS), DC = (float)(1u << SORT_DIR_BITS);
  const float px = (float)((o.x + t_enter * d.x - tr.bounds[0]) / (tr.bounds[3] - tr.bounds[0]));
  const float py = (float)((o.y + t_enter * d.y - tr.bounds[1]) / (tr.bounds[4] - tr.bounds[1]));
  const float pz = (float)((o.z + t_enter * d.z - tr.bounds[2]) / (tr.bounds[5] - tr.bounds[2]));
  const uint32_t ix = (uint32_t)fminf(fmaxf(px * CELLS, 0.0f), CELLS - 1.0f);
  const uint32_t iy = (uint32_t)fminf(fmaxf(py * CELLS, 0.0f), CELLS - 1.0f);
  const uint32_t iz = (uint32_t)fminf(fmaxf(pz * CELLS, 0.0f), CELLS - 1.0f);
  const uint32_t oct = (d.x < 0.0 ? 1u : 0u) | (d.y < 0.0 ? 2u : 0u) | (d.z < 0.0 ? 4u : 0u);
  uint32_t jx = 0u, jy = 0u, jz = 0u;
  if constexpr (SORT_DIR_BITS != 0u) { // (scheduling only: nothing here needs to be exact)
    const float ax = fabsf((float)d.x), ay = fabsf((float)d.y), az = fabsf((float)d.z);
    const float inv = 1.0f / fmaxf(ax + ay + az, 1e-30f);
    jx = (uint32_t)fminf(ax * inv * DC, DC - 1.0f); jy = (uint32_t)fminf(ay * inv * DC, DC - 1.0f); jz = (uint32_t)fminf(az * inv * DC, DC - 1.0f);
  }
  uint32_t key = 0u, pb = SORT_POS_BITS, db = SORT_DIR_BITS;
#pragma unroll
  for (uint32_t g = 0; g < sizeof(RPT_SORT_PATTERN) - 1u; g++) {
    const char c = RPT_SORT_PATTERN[g];
    uint32_t grp;
    if (c == 'O') grp = oct;
    else if (c == 'p') { pb--; grp = ((ix >> pb) & 1u) | (((iy >> pb) & 1u) << 1) | (((iz >> pb) & 1u) << 2); }
    else { db--; grp = ((jx >> db) & 1u) | (((jy >> db) & 1u) << 1) | (((jz >> db) & 1u) << 2); }
    key = (key << 3) | grp;
  }
  return key;
}

struct SceneBox { double bounds[6]; }; // the grid of a key that is not a tree's: the scene's bounded objects (path re-order)
