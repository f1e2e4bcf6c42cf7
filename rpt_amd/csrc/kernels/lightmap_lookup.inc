// kernels/lightmap_lookup.inc — rptgpu_lookup_lightmap's kernel (include/rpt_gpu_lightmap_lookup.h states every expression;
// DESIGN.md §25): rpt_hit_surface has left each ray's object, triangle and barycentrics; one lane per ray finds the object's
// binding in a table, interpolates the triangle's uvs, fetches one texel (NEAREST) or two rows of two (BILINEAR) and writes the
// named channels.  No shape code, no scene record: a translation unit of its own (kernels_lightmap_lookup.hip, inside
// namespace rptlookup), compiled with -ffp-contract=off — the header's order of operations is the code's.
// A lane's values are named scalars throughout: nothing here is an array indexed at run time.

struct Texel {
  double a, b, c;
};
// the two neighbouring texels of one row that a bilinear fetch can need, from ONE contiguous read of 16 or 48 bytes (a map one
// texel wide has no neighbour: the one texel stands for both), and their valid bytes
struct RowTaps {
  Texel lo, hi;
  bool vlo, vhi;
};

LK_DEV Texel texel_at(const Binding& B, uint64_t i) {
  if (B.components == 3u) {
    const double* __restrict__ p = B.map + 3ull * i;
    return Texel{p[0], p[1], p[2]};
  }
  const double s = B.map[i];
  return Texel{s, s, s};
}
LK_DEV bool valid_at(const Binding& B, uint64_t i) { return !B.valid || B.valid[i] != 0; }

// texels (xl, y) and (xl + 1, y); `two`: the map is at least two texels wide, and xl <= width - 2
LK_DEV RowTaps row_taps(const Binding& B, uint32_t y, uint32_t xl, bool two) {
  const uint64_t i = (uint64_t)y * B.width + xl;
  RowTaps r;
  if (B.components == 3u) {
    const double* __restrict__ p = B.map + 3ull * i;
    r.lo = Texel{p[0], p[1], p[2]};
    r.hi = two ? Texel{p[3], p[4], p[5]} : r.lo;
  } else {
    const double* __restrict__ p = B.map + i;
    const double s0 = p[0];
    const double s1 = two ? p[1] : s0;
    r.lo = Texel{s0, s0, s0};
    r.hi = Texel{s1, s1, s1};
  }
  r.vlo = valid_at(B, i);
  r.vhi = two ? valid_at(B, i + 1) : r.vlo;
  return r;
}
LK_DEV Texel pick(bool hi, const RowTaps& r) { return hi ? r.hi : r.lo; }

// floor(s) of an s inside [-1, size] as a texel index clamped to the map's edge
LK_DEV uint32_t clamp_index(int64_t x, uint32_t size) {
  return (uint32_t)(x < 0 ? 0 : (x > (int64_t)size - 1 ? (int64_t)size - 1 : x));
}

__global__ void __launch_bounds__(256) rpt_lightmap_lookup(uint32_t n, Rays r) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t ch = r.channels;
  const int32_t obj = r.object[i];
  const int32_t prim = r.primitive[i];
  int32_t bi = -1;
  if (obj >= 0 && (uint32_t)obj < r.num_objects && prim >= 0) bi = r.binding_of[obj];
  double U = 0.0, V = 0.0;
  double v0 = r.fallback[0], v1 = r.fallback[1], v2 = r.fallback[2];
  bool covered = false;
  if (bi >= 0) {
    const Binding B = r.bindings[bi];
    if ((uint32_t)prim >= B.n_tris) { // (the host holds n_tris to the mesh: cannot happen; never read beyond uvs)
      bi = -1;
    } else {
      const double* __restrict__ bc = r.barycentric + 3ull * i;
      const double u = bc[0], v = bc[1], w = bc[2];
      const double* __restrict__ t = B.uvs + 6ull * (uint32_t)prim;
      U = (u * t[0] + v * t[2]) + w * t[4];
      V = (u * t[1] + v * t[3]) + w * t[5];
      const bool finite = fabs(U) < LK_INF && fabs(V) < LK_INF;
      const double Wd = (double)B.width, Hd = (double)B.height;
      if (r.filter == RPT_LOOKUP_NEAREST) {
        const uint32_t x = (uint32_t)(int64_t)fmin(fmax(floor(U * Wd), 0.0), (double)(B.width - 1u));
        const uint32_t y = (uint32_t)(int64_t)fmin(fmax(floor(V * Hd), 0.0), (double)(B.height - 1u));
        const uint64_t at = (uint64_t)y * B.width + x;
        covered = finite && valid_at(B, at);
        if (covered) {
          const Texel m = texel_at(B, at);
          v0 = m.a; v1 = m.b; v2 = m.c;
        }
      } else {
        const double s = fmin(fmax(U * Wd - 0.5, -1.0), Wd);
        const double tt = fmin(fmax(V * Hd - 0.5, -1.0), Hd);
        const double x0f = floor(s), y0f = floor(tt);
        const double fx = s - x0f, fy = tt - y0f;
        const int64_t x0 = (int64_t)x0f, y0 = (int64_t)y0f;
        const uint32_t xa = clamp_index(x0, B.width), xb = clamp_index(x0 + 1, B.width);
        const uint32_t ya = clamp_index(y0, B.height), yb = clamp_index(y0 + 1, B.height);
        const bool two = B.width >= 2u;
        const uint32_t xl = two ? (xa < B.width - 2u ? xa : B.width - 2u) : 0u;
        const bool a_hi = xa != xl, b_hi = xb != xl;
        const RowTaps ra = row_taps(B, ya, xl, two), rb = row_taps(B, yb, xl, two);
        const Texel m00 = pick(a_hi, ra), m10 = pick(b_hi, ra), m01 = pick(a_hi, rb), m11 = pick(b_hi, rb);
        const bool k00 = a_hi ? ra.vhi : ra.vlo, k10 = b_hi ? ra.vhi : ra.vlo;
        const bool k01 = a_hi ? rb.vhi : rb.vlo, k11 = b_hi ? rb.vhi : rb.vlo;
        const double gx = 1.0 - fx, gy = 1.0 - fy;
        const double w00 = k00 ? gx * gy : 0.0, w10 = k10 ? fx * gy : 0.0;
        const double w01 = k01 ? gx * fy : 0.0, w11 = k11 ? fx * fy : 0.0;
        const double ws = ((w00 + w10) + w01) + w11;
        covered = finite && ws > 0.0;
        if (covered) {
          v0 = (((w00 * m00.a + w10 * m10.a) + w01 * m01.a) + w11 * m11.a) / ws;
          v1 = (((w00 * m00.b + w10 * m10.b) + w01 * m01.b) + w11 * m11.b) / ws;
          v2 = (((w00 * m00.c + w10 * m10.c) + w01 * m01.c) + w11 * m11.c) / ws;
        }
      }
    }
  }
  if (bi < 0) { U = 0.0; V = 0.0; }
  if (ch & RPT_LOOKUP_BINDING) r.binding[i] = bi;
  if (ch & RPT_LOOKUP_COVERED) r.covered[i] = covered ? 1 : 0;
  if (ch & RPT_LOOKUP_UV) {
    double* __restrict__ o = r.uv + 2ull * i;
    o[0] = U; o[1] = V;
  }
  if (ch & RPT_LOOKUP_VALUE) {
    double* __restrict__ o = r.value + 3ull * i;
    o[0] = v0; o[1] = v1; o[2] = v2;
  }
}

#ifndef __HIP_DEVICE_COMPILE__
hipError_t lookup(hipStream_t st, uint32_t n, const Rays& r) {
  hipLaunchKernelGGL(rpt_lightmap_lookup, dim3(launch_blocks(n)), dim3(BLOCK), 0, st, n, r);
  return hipGetLastError();
}
#endif
