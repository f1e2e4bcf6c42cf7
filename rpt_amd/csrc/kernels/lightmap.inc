// kernels/lightmap.inc — rptgpu_bake_lightmap's own kernels (include/rpt_gpu_lightmap.h states the contract, DESIGN.md §22
// the argument): rpt_lightmap_owners[_large] rasterise the triangles' uv charts into the owner map, rpt_lightmap_texels
// interpolates a piece's texels and compacts the owned ones for the gathers, rpt_lightmap_scatter carries the gathers'
// results back, rpt_lightmap_dilate fills the gutters.  Included by kernels_lightmap.hip alone, inside namespace
// rptlightmap; it touches no shape code, so it has no strict / ext pair.  Plain f64, -ffp-contract=off: every expression
// below is the header's, in its order.

constexpr uint32_t LM_BLOCK = 256;
constexpr uint32_t LM_WAVE = 64;
constexpr uint32_t LM_WAVES = LM_BLOCK / LM_WAVE;
// a box of at most this many texels is strided by the wave that found it (64 steps); a larger one goes to the list the
// second launch strides with its whole grid
constexpr uint64_t LM_SMALL_BOX = 4096;
constexpr uint32_t LM_GRID_MAX = 2048; // blocks of a grid-stride launch (256 CUs x 8)

// e(P, Q, c)
__device__ inline double lm_edge(double px, double py, double qx, double qy, double cx, double cy) {
  return (qx - px) * (cy - py) - (qy - py) * (cx - px);
}

// a triangle in texel space; ok: it may cover something (finite vertices, a finite area that is not zero)
struct LmChart {
  double x1, y1, x2, y2, x3, y3, area;
  bool ok;
};
__device__ inline LmChart lm_chart(const double* uv, uint32_t width, uint32_t height) {
  const double w = (double)width, h = (double)height;
  LmChart c;
  c.x1 = uv[0] * w; c.y1 = uv[1] * h;
  c.x2 = uv[2] * w; c.y2 = uv[3] * h;
  c.x3 = uv[4] * w; c.y3 = uv[5] * h;
  c.area = lm_edge(c.x1, c.y1, c.x2, c.y2, c.x3, c.y3);
  c.ok = __builtin_isfinite(c.x1) && __builtin_isfinite(c.y1) && __builtin_isfinite(c.x2) && __builtin_isfinite(c.y2) &&
         __builtin_isfinite(c.x3) && __builtin_isfinite(c.y3) && __builtin_isfinite(c.area) && c.area != 0.0;
  return c;
}
// does chart c (ok) cover the texel centre (cx, cy)?  e: e1, e2, e3 there
__device__ inline bool lm_covers(const LmChart& c, double cx, double cy, double e[3]) {
  e[0] = lm_edge(c.x2, c.y2, c.x3, c.y3, cx, cy);
  e[1] = lm_edge(c.x3, c.y3, c.x1, c.y1, cx, cy);
  e[2] = lm_edge(c.x1, c.y1, c.x2, c.y2, cx, cy);
  return c.area > 0.0 ? (e[0] >= 0.0 && e[1] >= 0.0 && e[2] >= 0.0) : (e[0] <= 0.0 && e[1] <= 0.0 && e[2] <= 0.0);
}

// the texels a chart (ok: finite vertices) may cover, a superset of the covered ones: lightmap_plan.h's clamp per axis — or
// the whole map for a sliver, whose rounded edge tests also pass along its line beyond the vertices (lightmap_plan.h sliver)
struct LmBox {
  TexelRange x, y;
  uint32_t bw;
  uint64_t count; // <= width * height <= 2^32
};
__device__ inline LmBox lm_box(const LmChart& c, uint32_t width, uint32_t height) {
  LmBox b;
  const double min_x = fmin(fmin(c.x1, c.x2), c.x3), max_x = fmax(fmax(c.x1, c.x2), c.x3);
  const double min_y = fmin(fmin(c.y1, c.y2), c.y3), max_y = fmax(fmax(c.y1, c.y2), c.y3);
  if (sliver(c.area, min_x, max_x, min_y, max_y, width, height)) {
    b.x = TexelRange{0u, width};
    b.y = TexelRange{0u, height};
  } else {
    b.x = clamp_range(min_x, max_x, width);
    b.y = clamp_range(min_y, max_y, height);
  }
  b.bw = b.x.hi - b.x.lo;
  b.count = (uint64_t)b.bw * (b.y.hi - b.y.lo);
  return b;
}
// texel k of box b tested against chart c of triangle j: the lowest index that covers it stays (an integer atomicMin — a
// vector global atomic, and order-independent).  The plain look first only spares atomics: owners never grow
__device__ inline void lm_claim(const LmChart& c, const LmBox& b, uint32_t k, uint32_t j, uint32_t width, uint32_t* owner) {
  const uint32_t x = b.x.lo + k % b.bw, y = b.y.lo + k / b.bw;
  double e[3];
  if (!lm_covers(c, (double)x + 0.5, (double)y + 0.5, e)) return;
  uint32_t* at = owner + ((uint64_t)y * width + x);
  if (__atomic_load_n(at, __ATOMIC_RELAXED) > j) atomicMin(at, j);
}

// One wavefront per triangle (grid-stride), its lanes striding the triangle's box — every branch but the coverage test is
// wave-uniform.  A box above LM_SMALL_BOX texels is appended to large[1 + large[0]++] instead (large[0] zeroed beforehand)
__global__ __launch_bounds__(LM_BLOCK) void rpt_lightmap_owners(Triangles t, uint32_t width, uint32_t height, uint32_t* owner,
                                                                uint32_t* large) {
  const uint32_t lane = threadIdx.x % LM_WAVE;
  const uint64_t waves = (uint64_t)gridDim.x * LM_WAVES;
  for (uint64_t j = (uint64_t)blockIdx.x * LM_WAVES + threadIdx.x / LM_WAVE; j < t.n; j += waves) {
    const LmChart c = lm_chart(t.uvs + 6 * j, width, height);
    if (!c.ok) continue;
    const LmBox b = lm_box(c, width, height);
    if (!b.count) continue;
    if (b.count > LM_SMALL_BOX) {
      if (lane == 0) large[1 + atomicAdd(&large[0], 1u)] = (uint32_t)j;
      continue;
    }
    for (uint32_t k = lane; k < (uint32_t)b.count; k += LM_WAVE) lm_claim(c, b, k, (uint32_t)j, width, owner);
  }
}
// ... and the listed triangles one after the other, each box strided by the whole grid
__global__ __launch_bounds__(LM_BLOCK) void rpt_lightmap_owners_large(Triangles t, uint32_t width, uint32_t height, uint32_t* owner,
                                                                      const uint32_t* large) {
  const uint32_t n_large = large[0];
  const uint64_t threads = (uint64_t)gridDim.x * LM_BLOCK, tid = (uint64_t)blockIdx.x * LM_BLOCK + threadIdx.x;
  for (uint32_t i = 0; i < n_large; i++) {
    const uint32_t j = large[1 + i];
    const LmChart c = lm_chart(t.uvs + 6 * (uint64_t)j, width, height);
    const LmBox b = lm_box(c, width, height);
    for (uint64_t k = tid; k < b.count; k += threads) lm_claim(c, b, (uint32_t)k, j, width, owner);
  }
}

// One lane per texel of the piece [base, base + m)
__global__ __launch_bounds__(LM_BLOCK) void rpt_lightmap_texels(Triangles t, uint32_t width, uint32_t height, double offset,
                                                                uint32_t stream_base, const uint32_t* owner, uint64_t base, uint32_t m,
                                                                RawOut raw, const uint32_t* incl, double* points, double* normals,
                                                                uint32_t* ids) {
  const uint32_t threads = gridDim.x * LM_BLOCK;
  for (uint32_t i = blockIdx.x * LM_BLOCK + threadIdx.x; i < m; i += threads) {
    const uint64_t texel = base + i;
    const uint32_t o = owner[texel];
    double b[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
    if (o != NOBODY) {
      const LmChart c = lm_chart(t.uvs + 6 * (uint64_t)o, width, height);
      const uint32_t x = (uint32_t)texel % width, y = (uint32_t)texel / width; // (a texel index has 32 bits)
      double e[3];
      (void)lm_covers(c, (double)x + 0.5, (double)y + 0.5, e);
      b[0] = e[0] / c.area; b[1] = e[1] / c.area; b[2] = e[2] / c.area;
      const double* p = t.positions + 9 * (uint64_t)o;
      double pos[3], mm[3];
      for (int k = 0; k < 3; k++) pos[k] = (b[0] * p[k] + b[1] * p[3 + k]) + b[2] * p[6 + k];
      if (t.normals) {
        const double* q = t.normals + 9 * (uint64_t)o;
        for (int k = 0; k < 3; k++) mm[k] = (b[0] * q[k] + b[1] * q[3 + k]) + b[2] * q[6 + k];
      } else { // Triangle::from_vertices (mesh.rs:27): (v2 - v1).cross(&(v3 - v1))
        const double ax = p[3] - p[0], ay = p[4] - p[1], az = p[5] - p[2];
        const double bx = p[6] - p[0], by = p[7] - p[1], bz = p[8] - p[2];
        mm[0] = ay * bz - az * by; mm[1] = az * bx - ax * bz; mm[2] = ax * by - ay * bx;
      }
      const double len = sqrt((mm[0] * mm[0] + mm[1] * mm[1]) + mm[2] * mm[2]);
      for (int k = 0; k < 3; k++) {
        n[k] = mm[k] / len;
        g[k] = pos[k] + offset * n[k];
      }
      if (incl) {
        const uint64_t slot = incl[i] - 1u;
        for (int k = 0; k < 3; k++) {
          points[3 * slot + k] = g[k];
          normals[3 * slot + k] = n[k];
        }
        ids[slot] = stream_base + (uint32_t)texel;
      }
    }
    if (raw.owner) raw.owner[texel] = (int32_t)o; // NOBODY is -1
    for (int k = 0; k < 3; k++) {
      if (raw.barycentric) raw.barycentric[3 * texel + k] = b[k];
      if (raw.position) raw.position[3 * texel + k] = g[k];
      if (raw.normal) raw.normal[3 * texel + k] = n[k];
    }
  }
}

__global__ __launch_bounds__(LM_BLOCK) void rpt_lightmap_scatter(const uint32_t* owner, uint64_t base, uint32_t m, const uint32_t* incl,
                                                                 const double* res, uint32_t words, double* out) {
  const uint32_t threads = gridDim.x * LM_BLOCK;
  for (uint32_t i = blockIdx.x * LM_BLOCK + threadIdx.x; i < m; i += threads) {
    const uint64_t texel = base + i;
    const bool owned = owner[texel] != NOBODY;
    const uint64_t slot = owned ? incl[i] - 1u : 0u;
    for (uint32_t k = 0; k < words; k++) out[words * texel + k] = owned ? res[words * slot + k] : 0.0;
  }
}

__global__ __launch_bounds__(LM_BLOCK) void rpt_lightmap_filled(const uint32_t* owner, uint64_t n, uint8_t* filled) {
  const uint64_t threads = (uint64_t)gridDim.x * LM_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * LM_BLOCK + threadIdx.x; i < n; i += threads) filled[i] = owner[i] != NOBODY ? 1 : 0;
}

// One round: every texel of dst from src alone (the ping-pong).  A filled texel keeps its value; an unfilled one with
// filled neighbours takes acc / (double)count over them in the order dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner)
template <uint32_t WORDS>
__global__ __launch_bounds__(LM_BLOCK) void rpt_lightmap_dilate(uint32_t width, uint32_t height, const double* src, const uint8_t* fsrc,
                                                                double* dst, uint8_t* fdst) {
  const uint64_t n = (uint64_t)width * height, threads = (uint64_t)gridDim.x * LM_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * LM_BLOCK + threadIdx.x; i < n; i += threads) {
    double v[WORDS];
    for (uint32_t k = 0; k < WORDS; k++) v[k] = src[WORDS * i + k];
    uint8_t f = fsrc[i];
    if (!f) {
      const int64_t x = (int64_t)(i % width), y = (int64_t)(i / width);
      double acc[WORDS];
      for (uint32_t k = 0; k < WORDS; k++) acc[k] = 0.0;
      uint32_t count = 0;
      for (int64_t dy = -1; dy <= 1; dy++)
        for (int64_t dx = -1; dx <= 1; dx++) {
          const int64_t xx = x + dx, yy = y + dy;
          if (xx < 0 || yy < 0 || xx >= (int64_t)width || yy >= (int64_t)height) continue;
          const uint64_t j = (uint64_t)yy * width + (uint64_t)xx;
          if (!fsrc[j]) continue; // (the texel itself is not filled)
          for (uint32_t k = 0; k < WORDS; k++) acc[k] = acc[k] + src[WORDS * j + k];
          count++;
        }
      if (count) {
        for (uint32_t k = 0; k < WORDS; k++) v[k] = acc[k] / (double)count;
        f = 1;
      }
    }
    for (uint32_t k = 0; k < WORDS; k++) dst[WORDS * i + k] = v[k];
    if (fdst) fdst[i] = f;
  }
}

// ---- the launchers (lightmap.h)
static inline uint32_t lm_blocks(uint64_t items) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (items + LM_BLOCK - 1) / LM_BLOCK), LM_GRID_MAX);
}

hipError_t owners(hipStream_t st, const Triangles& t, uint32_t width, uint32_t height, uint32_t* owner, uint32_t* large) {
  const uint64_t n = (uint64_t)width * height;
  hipError_t e = hipMemsetAsync(owner, 0xFF, n * sizeof(uint32_t), st);
  if (e != hipSuccess || !t.n) return e;
  e = hipMemsetAsync(large, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  const uint32_t by_wave = (uint32_t)std::min<uint64_t>(((uint64_t)t.n + LM_WAVES - 1) / LM_WAVES, 16 * LM_GRID_MAX);
  rpt_lightmap_owners<<<by_wave, LM_BLOCK, 0, st>>>(t, width, height, owner, large);
  rpt_lightmap_owners_large<<<lm_blocks(n), LM_BLOCK, 0, st>>>(t, width, height, owner, large);
  return hipGetLastError();
}

struct LmOwned {
  __host__ __device__ uint32_t operator()(uint32_t o) const { return o != NOBODY ? 1u : 0u; }
};
hipError_t scan_bytes(uint64_t piece, size_t* bytes) {
  *bytes = 0;
  auto in = rocprim::make_transform_iterator((const uint32_t*)nullptr, LmOwned{});
  return rocprim::inclusive_scan(nullptr, *bytes, in, (uint32_t*)nullptr, (size_t)piece, rocprim::plus<uint32_t>());
}
hipError_t scan_owned(hipStream_t st, const uint32_t* owner, uint64_t base, uint32_t m, uint32_t* incl, void* tmp, size_t tmp_bytes) {
  auto in = rocprim::make_transform_iterator(owner + base, LmOwned{});
  return rocprim::inclusive_scan(tmp, tmp_bytes, in, incl, (size_t)m, rocprim::plus<uint32_t>(), st);
}

hipError_t texels(hipStream_t st, const Triangles& t, uint32_t width, uint32_t height, double offset, uint32_t stream_base,
                  const uint32_t* owner, uint64_t base, uint32_t m, const RawOut& raw, const uint32_t* incl, double* points,
                  double* normals, uint32_t* ids) {
  rpt_lightmap_texels<<<lm_blocks(m), LM_BLOCK, 0, st>>>(t, width, height, offset, stream_base, owner, base, m, raw, incl, points,
                                                         normals, ids);
  return hipGetLastError();
}

hipError_t scatter(hipStream_t st, const uint32_t* owner, uint64_t base, uint32_t m, const uint32_t* incl, const double* res,
                   uint32_t words, double* out) {
  rpt_lightmap_scatter<<<lm_blocks(m), LM_BLOCK, 0, st>>>(owner, base, m, incl, res, words, out);
  return hipGetLastError();
}

hipError_t filled_from_owner(hipStream_t st, const uint32_t* owner, uint64_t n, uint8_t* filled) {
  rpt_lightmap_filled<<<lm_blocks(n), LM_BLOCK, 0, st>>>(owner, n, filled);
  return hipGetLastError();
}

hipError_t dilate(hipStream_t st, uint32_t width, uint32_t height, uint32_t words, const double* src, const uint8_t* filled_src,
                  double* dst, uint8_t* filled_dst) {
  const uint32_t blocks = lm_blocks((uint64_t)width * height);
  if (words == 3) rpt_lightmap_dilate<3><<<blocks, LM_BLOCK, 0, st>>>(width, height, src, filled_src, dst, filled_dst);
  else rpt_lightmap_dilate<1><<<blocks, LM_BLOCK, 0, st>>>(width, height, src, filled_src, dst, filled_dst);
  return hipGetLastError();
}
