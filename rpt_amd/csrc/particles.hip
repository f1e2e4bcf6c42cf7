// particles.hip — the reference's `rpt::ode` (src/ode/particle_system.rs, src/shape/monomial_surface.rs:126-152) on gfx950:
// ParticleSystem::time_derivative of SolidGravitySystem / MarblesSystem / SimpleCircleSystem and the fixed-step RK4
// driver rk4_integrate, bit-identical to the reference's f64 arithmetic.  Compiled with -ffp-contract=off like every
// other object (no a*b+c is fused).  DESIGN.md §8 has the design; the exactness points are cited where they are kept:
//
//  * Accumulation order.  The reference runs `for i { for j < i { acc[j] += f(i,j); acc[i] -= f(i,j) } }`
//    (particle_system.rs:48-56, :74-86), so body k receives its terms as i (partners j = 0..k-1) and then its terms
//    as j (partners i = k+1..n-1): its partners in increasing index.  One thread per body walks them in that order and
//    gets the reference's bits with no atomics; every pair is evaluated twice, once by each of its bodies, identically.
//  * powi as the reference's compiler-rt __powidf2 evaluates it, the reciprocal last: powi(-2) = 1 / (x*x),
//    powi(-5) = 1 / (x * ((x*x) * (x*x))), powi(3) = x * (x*x), powi(1) = x (kernels/vec.inc pow2 / pow3 / pow5).
//  * MonomialSurface::closest_point keeps the FIRST strict minimum of 201 grid distances (NaN never taken, best_x = -1
//    if nothing beats 1e18); spread over lanes it is the lexicographic minimum of (dist2, index).  x.hypot(z) is the
//    platform libm's, glibc 2.35's dbl-64 hypot, which is not correctly rounded: it is restated below.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rpt_gpu.h"
#include "particles.h"

namespace rpt_particles_dev {
#define RPT_DEV __device__ __forceinline__
#include "kernels/vec.inc"

constexpr int BLOCK = 256;         // grid schedule: bodies per workgroup = partner positions per LDS tile
constexpr int SINGLE_BIG = 1024;   // single-workgroup schedule above 256 bodies: threads of the one workgroup
constexpr int SINGLE_COOP = 256;   // ... up to 256 bodies: 256 threads, the closest-point grid spread over lanes
constexpr int SURF_STEPS = 100;    // MarblesSystem's surface: closest_point (not _precise), height 2, exp 4
constexpr double SURF_HEIGHT = 2.;
constexpr int TAB = 2 * SURF_STEPS + 1;
constexpr int NONE = 0x7fffffff;   // "no grid point beat 1e18" (best_x stays -1)
constexpr int PAIR_MAX = 48;       // single-workgroup schedule: pair terms through LDS up to this many bodies
constexpr int PAIR_SLOTS = PAIR_MAX * (PAIR_MAX - 1) / 2;

// ------------------------------------------------------------------ glibc 2.35 hypot (sysdeps/ieee754/dbl-64/e_hypot.c)
// x86-64 builds take the kernel without __FP_FAST_FMA: one Newton-style correction of sqrt(ax*ax + ay*ay).  Scaling by
// 2^-600 / 2^600 outside [2^-511, 2^511], and ax + ay when ay <= ax * 2^-54.  tests/test_ode_host.py proves the host
// restatement (tests/cpp/ode_check.cpp) equal to std::hypot; tests/test_gpu_ode.py evaluates this one directly
// (rptgpu_particles_eval_hypot) and compares it with both.
RPT_DEV double hypot_kernel(double ax, double ay) {
  double t1, t2;
  double h = sqrt(ax * ax + ay * ay);
  if (h <= 2.0 * ay) {
    double delta = h - ay;
    t1 = ax * (2.0 * delta - ax);
    t2 = (delta - 2.0 * (ax - ay)) * delta;
  } else {
    double delta = h - ax;
    t1 = 2.0 * delta * (ax - 2.0 * ay);
    t2 = (4.0 * delta - ay) * ay + delta * delta;
  }
  h -= (t1 + t2) / (2.0 * h);
  return h;
}
RPT_DEV bool is_signaling(double x) {
  uint64_t b = (uint64_t)__double_as_longlong(x) & 0x7fffffffffffffffull;
  return b > 0x7ff0000000000000ull && !(b & 0x0008000000000000ull);
}
RPT_DEV double glibc_hypot(double x, double y) {
  if (!__builtin_isfinite(x) || !__builtin_isfinite(y)) {
    if ((__builtin_isinf(x) || __builtin_isinf(y)) && !is_signaling(x) && !is_signaling(y)) return __builtin_inf();
    return x + y;
  }
  x = __builtin_fabs(x);
  y = __builtin_fabs(y);
  double ax = x < y ? y : x;
  double ay = x < y ? x : y;
  if (ax > 0x1p+511) {
    if (ay <= ax * 0x1p-54) return ax + ay;
    return hypot_kernel(ax * 0x1p-600, ay * 0x1p-600) / 0x1p-600;
  }
  if (ay < 0x1p-511) {
    if (ax >= ay / 0x1p-54) return ax + ay;
    return hypot_kernel(ax / 0x1p-600, ay / 0x1p-600) * 0x1p-600;
  }
  if (ay <= ax * 0x1p-54) return ax + ay;
  return hypot_kernel(ax, ay);
}

// ------------------------------------------------------------------ MonomialSurface::closest_point (:126-152)
// grid point i of -steps..=steps: xf = i / steps and height * xf.powi(4) (powi(4) = (x*x) * (x*x))
RPT_DEV double grid_x(int i, int steps) { return (double)i / (double)steps; }
RPT_DEV double grid_y(double xf, double height) { return height * ((xf * xf) * (xf * xf)); }
// glm::distance2(&pt, &vec2(xf, y)): the squared components summed x then y
RPT_DEV double grid_dist2(double px, double py, double gx, double gy) {
  double dx = px - gx, dy = py - gy;
  return dx * dx + dy * dy;
}
// (dist2, index) pairs: the first strict minimum of a sequential scan is the lexicographic minimum
RPT_DEV void best_merge(double& d, int& i, double d2, int i2) {
  if (d2 < d || (d2 == d && i2 < i)) { d = d2; i = i2; }
}
// the closest point once the grid's best index is known (NONE: best_x stays -1)
RPT_DEV D3 closest_from(D3 p, int best, int steps, double height) {
  double best_x = best == NONE ? -1. : grid_x(best - steps, steps);
  // res.1 * glm::normalize(&vec2(x, z)): the 2-vector's length, then one IEEE division per component (a point on the
  // y axis gives 0 / 0 = NaN, as in the reference)
  double nrm = sqrt(p.x * p.x + p.z * p.z);
  double qx = best_x * (p.x / nrm), qz = best_x * (p.z / nrm);
  double r2 = qx * qx + qz * qz;                 // xz.x.powi(2) + xz.y.powi(2)
  return mk(qx, height * (r2 * r2), qz);         // (...).powi(2)
}
RPT_DEV bool closest_is_point(D3 p) { return length(p) < 1e-12; } // "Can't normalize in this case"
// one lane's share of the scan: grid indices first, first + stride, ... (steps of the marbles' surface, from LDS)
RPT_DEV void scan_tab(double px, double py, const double* tx, const double* ty, int first, int stride, double& d, int& bi) {
  for (int i = first; i < TAB; i += stride) {
    double d2 = grid_dist2(px, py, tx[i], ty[i]);
    if (d2 < d) { d = d2; bi = i; }
  }
}
RPT_DEV D3 surface_closest_serial(D3 p, const double* tx, const double* ty) {
  if (closest_is_point(p)) return p;
  double d = 1e18;
  int bi = NONE;
  scan_tab(glibc_hypot(p.x, p.z), p.y, tx, ty, 0, 1, d, bi);
  return closest_from(p, bi, SURF_STEPS, SURF_HEIGHT);
}
RPT_DEV void fill_tab(double* tx, double* ty) {
  for (int i = threadIdx.x; i < TAB; i += blockDim.x) {
    tx[i] = grid_x(i - SURF_STEPS, SURF_STEPS);
    ty[i] = grid_y(tx[i], SURF_HEIGHT);
  }
}

// ------------------------------------------------------------------ the pair terms and the per-body terms
// SolidGravitySystem (:50-53): dir * (len.powi(-2) - 0.0001 * len.powi(-5)) with d = pos_i - pos_j
RPT_DEV D3 gravity_force(D3 d) {
  D3 dir = normalize(d);
  double len = length(d);
  return dir * (1.0 / pow2(len) - 0.0001 * (1.0 / pow5(len)));
}
// MarblesSystem (:76-84): contact when len < 2R; force = -dir * 5. * ((2R - len) / R).powi(1), evaluated
// ((-dir) * 5.) * ratio
RPT_DEV bool marbles_force(D3 d, double R, D3& f) {
  D3 dir = normalize(d);
  double len = length(d);
  if (!(len < 2. * R)) return false;
  f = ((-dir) * 5.) * ((2. * R - len) / R);
  return true;
}
// surface (:93-106), table (:108-120) and "air resistance" (:121-124) of one marble whose pair terms are in acc
RPT_DEV D3 marbles_body(D3 p, D3 v, D3 closest, double R, D3 acc) {
  D3 vec = p - closest;
  D3 normal = normalize(vec);
  double ratio = (R - length(vec)) / R;
  double nv = dot(v, normal);
  if (-0.1 < ratio && ratio < 0.) acc = acc - (30. * normal) * pow3(nv);
  else if (ratio >= 0.) acc = acc + (100. * normal) * ratio;
  // the table's normal is the full vector (0, 1, 0): its x and z products keep the reference's zeros and NaNs
  D3 tn = mk(0., 1., 0.);
  double tr = ((R - 0.06) - p.y) / R;
  double tv = dot(v, tn);
  if (length(p) > 0.1) {
    if (-0.1 < tr && tr < 0.) acc = acc - (20. * tn) * tv;
    else if (tr >= 0.) acc = acc + (300000. * tn) * tr;
  }
  return acc - v / 5.; // a division, not * 0.2
}

// the pair sum of body k over partners pp(0..n-1), in increasing partner index (the reference's order, see above);
// for partner p < k the body is `i` (d = pk - pp, acc -= f), for p > k it is `j` (d = pp - pk, acc += f)
template <int KIND> RPT_DEV void pair_term(D3 pk, D3 vk, int k, int p, D3 pp, double R, D3& acc) {
  if (p == k) return;
  bool as_i = p < k;
  D3 d = as_i ? pk - pp : pp - pk;
  if (KIND == RPT_PARTICLES_SOLID_GRAVITY) {
    D3 f = gravity_force(d);
    acc = as_i ? acc - f : acc + f;
  } else {
    D3 f;
    if (marbles_force(d, R, f)) {
      acc = as_i ? acc - f : acc + f;
      acc = acc - vk * 0.5; // acc[i] -= vel[i] * 0.5 / acc[j] -= vel[j] * 0.5, in the pair loop
    }
  }
}
RPT_DEV D3 acc_init(int kind) { return kind == RPT_PARTICLES_MARBLES ? mk(0., -1., 0.) : mk(0., 0., 0.); }

// SimpleCircleSystem (:29-39): pos' = (-p.y, p.x, 0), vel' = 0; the others: pos' = vel
template <int KIND> RPT_DEV D3 dpos_of(D3 p, D3 v) { return KIND == RPT_PARTICLES_CIRCLE ? mk(-p.y, p.x, 0.0) : v; }

RPT_DEV D3 ld(const double* a, int k) { return mk(a[3 * k], a[3 * k + 1], a[3 * k + 2]); }
RPT_DEV void st(double* a, int k, D3 v) { a[3 * k] = v.x; a[3 * k + 1] = v.y; a[3 * k + 2] = v.z; }

// ------------------------------------------------------------------ the grid schedule
// One thread per body; the partners' positions pass through LDS one 256-body tile at a time, every lane of a wave
// reading the same partner (an LDS broadcast).  stage < 0: the derivative of src into out.  stage 0..3: the RK4
// stage (particle_system.rs:12-17) fused behind the derivative k of the stage state src:
//   0: ks = k1;          dst = s + k1 * (h / 2)
//   1: ks = ks + k2 * 2; dst = s + k2 * (h / 2)
//   2: ks = ks + k3 * 2; dst = s + k3 * h
//   3: ks = ks + k4;     s = s + ks * (h / 6)        (((k1 + k2*2) + k3*2) + k4) * (step / 6)
// src is never written in the same launch (the stage states alternate between two buffers).
template <int KIND>
__global__ __launch_bounds__(BLOCK) void rpt_particles_stage(uint32_t n, double R, const double* __restrict__ src,
                                                             double* __restrict__ out, double* s, double* ks,
                                                             double* __restrict__ dst, int stage, double h) {
  __shared__ double tp[3 * BLOCK];
  __shared__ double tx[TAB], ty[TAB];
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = k < (int)n;
  if (KIND == RPT_PARTICLES_MARBLES) fill_tab(tx, ty);
  D3 pk = live ? ld(src, k) : mk(0, 0, 0);
  D3 vk = live ? ld(src + 3 * n, k) : mk(0, 0, 0);
  D3 acc = acc_init(KIND);
  if (KIND != RPT_PARTICLES_CIRCLE) {
    for (uint32_t t0 = 0; t0 < n; t0 += BLOCK) {
      __syncthreads();
      for (int c = threadIdx.x; c < 3 * BLOCK && t0 * 3 + c < 3 * n; c += BLOCK) tp[c] = src[3 * t0 + c];
      __syncthreads();
      const int m = min((uint32_t)BLOCK, n - t0);
      if (live)
        for (int q = 0; q < m; q++) pair_term<KIND>(pk, vk, k, (int)t0 + q, mk(tp[3 * q], tp[3 * q + 1], tp[3 * q + 2]), R, acc);
    }
  }
  if (!live) return;
  if (KIND == RPT_PARTICLES_MARBLES) acc = marbles_body(pk, vk, surface_closest_serial(pk, tx, ty), R, acc);
  D3 dp = dpos_of<KIND>(pk, vk);
  D3 dv = KIND == RPT_PARTICLES_CIRCLE ? mk(0.0, 0.0, 0.0) : acc;
  if (stage < 0) {
    st(out, k, dp);
    st(out + 3 * n, k, dv);
    return;
  }
  D3 sp = ld(s, k), sv = ld(s + 3 * n, k);
  if (stage == 0) {
    st(ks, k, dp);
    st(ks + 3 * n, k, dv);
  } else {
    double w = stage == 3 ? 1.0 : 2.0;
    D3 ap = ld(ks, k), av = ld(ks + 3 * n, k);
    ap = stage == 3 ? ap + dp : ap + dp * w;
    av = stage == 3 ? av + dv : av + dv * w;
    if (stage == 3) {
      double h6 = h / 6.0;
      st(s, k, sp + ap * h6);
      st(s + 3 * n, k, sv + av * h6);
      return;
    }
    st(ks, k, ap);
    st(ks + 3 * n, k, av);
  }
  double hs = stage == 2 ? h : h / 2.0;
  st(dst, k, sp + dp * hs);
  st(dst + 3 * n, k, sv + dv * hs);
}

// ------------------------------------------------------------------ the single-workgroup schedule
// rk4_integrate in one workgroup per dispatch: the host splits the step schedule `while time > step { step(step);
// time -= step; } step(time)` (:19-23) into dispatches of a bounded number of steps (the state goes through global
// memory between them, bit for bit); within a dispatch each thread keeps its bodies' state and RK4 sum in registers,
// the stage state's positions live in LDS, and a barrier separates the stages.  Up to 256 bodies
// (256 threads) the marbles' closest-point scan is spread over L = 256 / pow2ceil(n) lanes per body (L <= 64, one
// wave) and reduced lexicographically by (dist2, index); above that each thread scans for its own bodies.  Up to
// PAIR_MAX bodies the n (n - 1) / 2 pair terms are computed once each by all the threads (the same f(i, j) both of its
// bodies would compute) and each body only accumulates them, in its order: the divisions leave the serial chain.
// BPT bodies per thread: 1 on 256 threads (n <= 256), 2 on 1024 threads (n <= RPT_PARTICLES_SINGLE_MAX)
template <int KIND, int BPT>
__global__ __launch_bounds__(BPT == 1 ? SINGLE_COOP : SINGLE_BIG) void rpt_particles_single(uint32_t n, double R, double* state, double* out,
                                                                  int derivative_only, uint32_t nfull, double step,
                                                                  int do_last, double last, int lanes) {
  static_assert(2 * SINGLE_BIG == RPT_PARTICLES_SINGLE_MAX, "two bodies per thread on the big workgroup");
  __shared__ double cp[3 * BPT * (BPT == 1 ? SINGLE_COOP : SINGLE_BIG)]; // the stage state's positions
  __shared__ double cl[3 * SINGLE_COOP];               // the closest points (cooperative scan)
  __shared__ double tx[TAB], ty[TAB];
  __shared__ double pf[3 * (BPT == 1 ? PAIR_SLOTS : 1)]; // the pair terms (pair_tab)
  __shared__ uint8_t pc[BPT == 1 ? PAIR_SLOTS : 1];      // ... and whether the pair touches (marbles)
  const int nt = blockDim.x, tid = threadIdx.x;
  if (KIND == RPT_PARTICLES_MARBLES) fill_tab(tx, ty);
  D3 sp[BPT], sv[BPT], kp[BPT], kv[BPT], cv[BPT];
#pragma unroll
  for (int q = 0; q < BPT; q++) {
    int k = tid + q * nt;
    if (k < (int)n) {
      sp[q] = ld(state, k);
      sv[q] = ld(state + 3 * n, k);
      st(cp, k, sp[q]);
      cv[q] = sv[q];
    }
  }
  __syncthreads();
  // the derivative of the stage state (positions in cp, velocities in cv) for this thread's bodies
  // up to PAIR_MAX bodies the pair terms f(i, j), i > j, are evaluated once each, spread over all the threads, into
  // LDS (pair t = i (i - 1) / 2 + j); each body then only ADDS its terms in the reference's order
  const bool pair_tab = BPT == 1 && KIND != RPT_PARTICLES_CIRCLE && n <= PAIR_MAX;
  auto derivative = [&](D3* dp, D3* dv) {
    if (pair_tab) {
      const int np = (int)(n * (n - 1) / 2);
      for (int t = tid; t < np; t += nt) {
        int i = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
        while (i * (i - 1) / 2 > t) i--;
        while ((i + 1) * i / 2 <= t) i++;
        int j = t - i * (i - 1) / 2;
        D3 d = ld(cp, i) - ld(cp, j); // pos_i - pos_j
        D3 f = mk(0, 0, 0);
        bool c = true;
        if (KIND == RPT_PARTICLES_SOLID_GRAVITY) f = gravity_force(d);
        else c = marbles_force(d, R, f);
        st(pf, t, f);
        pc[t] = c;
      }
    }
    if (KIND == RPT_PARTICLES_MARBLES && lanes > 0) {
      int b = tid / lanes, sub = tid % lanes;
      double d = 1e18;
      int bi = NONE;
      D3 pb = b < (int)n ? ld(cp, b) : mk(0, 0, 0);
      if (b < (int)n && !closest_is_point(pb)) scan_tab(glibc_hypot(pb.x, pb.z), pb.y, tx, ty, sub, lanes, d, bi);
      for (int o = lanes >> 1; o > 0; o >>= 1) {
        double d2 = __shfl_xor(d, o, lanes);
        int i2 = __shfl_xor(bi, o, lanes);
        best_merge(d, bi, d2, i2);
      }
      if (b < (int)n && sub == 0) st(cl, b, closest_is_point(pb) ? pb : closest_from(pb, bi, SURF_STEPS, SURF_HEIGHT));
    }
    if (pair_tab || (KIND == RPT_PARTICLES_MARBLES && lanes > 0)) __syncthreads();
#pragma unroll
    for (int q = 0; q < BPT; q++) {
      int k = tid + q * nt;
      if (k >= (int)n) continue;
      D3 pk = ld(cp, k), vk = cv[q];
      D3 acc = acc_init(KIND);
      if (pair_tab) {
        for (int p = 0; p < (int)n; p++) {
          if (p == k) continue;
          const bool as_i = p < k;
          const int t = as_i ? k * (k - 1) / 2 + p : p * (p - 1) / 2 + k;
          if (!pc[t]) continue; // no contact: nothing added (most marble pairs)
          D3 f = ld(pf, t);
          acc = as_i ? acc - f : acc + f;
          if (KIND == RPT_PARTICLES_MARBLES) acc = acc - vk * 0.5;
        }
      } else if (KIND != RPT_PARTICLES_CIRCLE) {
        for (int p = 0; p < (int)n; p++) pair_term<KIND>(pk, vk, k, p, ld(cp, p), R, acc);
      }
      if (KIND == RPT_PARTICLES_MARBLES)
        acc = marbles_body(pk, vk, lanes > 0 ? ld(cl, k) : surface_closest_serial(pk, tx, ty), R, acc);
      dp[q] = dpos_of<KIND>(pk, vk);
      dv[q] = KIND == RPT_PARTICLES_CIRCLE ? mk(0.0, 0.0, 0.0) : acc;
    }
    __syncthreads(); // every read of cp / cl is done before the stage state is replaced
  };
  D3 dp[BPT], dv[BPT];
  if (derivative_only) {
    derivative(dp, dv);
#pragma unroll
    for (int q = 0; q < BPT; q++) {
      int k = tid + q * nt;
      if (k < (int)n) {
        st(out, k, dp[q]);
        st(out + 3 * n, k, dv[q]);
      }
    }
    return;
  }
  // one RK4 step of size h (particle_system.rs:12-17)
  auto rk4_step = [&](double h) {
    const double h2 = h / 2.0;
    for (int stage = 0; stage < 4; stage++) {
      derivative(dp, dv);
#pragma unroll
      for (int q = 0; q < BPT; q++) {
        int k = tid + q * nt;
        if (k >= (int)n) continue;
        if (stage == 0) { kp[q] = dp[q]; kv[q] = dv[q]; }
        else if (stage == 3) { kp[q] = kp[q] + dp[q]; kv[q] = kv[q] + dv[q]; }
        else { kp[q] = kp[q] + dp[q] * 2.0; kv[q] = kv[q] + dv[q] * 2.0; }
        D3 np, nv;
        if (stage == 3) {
          double h6 = h / 6.0;
          sp[q] = sp[q] + kp[q] * h6;
          sv[q] = sv[q] + kv[q] * h6;
          np = sp[q];
          nv = sv[q];
        } else {
          double hs = stage == 2 ? h : h2;
          np = sp[q] + dp[q] * hs;
          nv = sv[q] + dv[q] * hs;
        }
        st(cp, k, np);
        cv[q] = nv;
      }
      __syncthreads();
    }
  };
  // this dispatch's share of the schedule the host computed with the reference's decrements (api_particles.cpp
  // schedule_of): nfull steps of `step`, then, in the last dispatch, the final step of `last`
  const uint32_t count = nfull + (do_last ? 1u : 0u);
  for (uint32_t i = 0; i < count; i++) rk4_step(i < nfull ? step : last);
#pragma unroll
  for (int q = 0; q < BPT; q++) {
    int k = tid + q * nt;
    if (k < (int)n) {
      st(state, k, sp[q]);
      st(state + 3 * n, k, sv[q]);
    }
  }
}

// ------------------------------------------------------------------ closest_point alone (any height and steps)
__global__ __launch_bounds__(BLOCK) void rpt_monomial_closest(double height, int steps, uint64_t n,
                                                              const double* __restrict__ pts, double* __restrict__ out) {
  uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= n) return;
  D3 p = mk(pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]);
  D3 r = p;
  if (!closest_is_point(p)) {
    double px = glibc_hypot(p.x, p.z), py = p.y, d = 1e18;
    int bi = NONE;
    for (int i = 0; i <= 2 * steps; i++) {
      double gx = grid_x(i - steps, steps);
      double d2 = grid_dist2(px, py, gx, grid_y(gx, height));
      if (d2 < d) { d = d2; bi = i; }
    }
    r = closest_from(p, bi, steps, height);
  }
  out[3 * k] = r.x;
  out[3 * k + 1] = r.y;
  out[3 * k + 2] = r.z;
}

__global__ __launch_bounds__(BLOCK) void rpt_particles_hypot(uint64_t n, const double* __restrict__ x,
                                                             const double* __restrict__ y, double* __restrict__ out) {
  uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k < n) out[k] = glibc_hypot(x[k], y[k]);
}

} // namespace rpt_particles_dev

namespace rptparticles {
using namespace rpt_particles_dev;

static int pow2ceil(uint32_t n) {
  int p = 1;
  while ((uint32_t)p < n) p <<= 1;
  return p;
}

hipError_t launch_single(const Sys& sys, uint32_t n, double* pos_vel, double* out, bool derivative_only, uint32_t nfull,
                         double step, bool do_last, double last, hipStream_t st) {
  int threads = n <= SINGLE_COOP ? SINGLE_COOP : SINGLE_BIG;
  int lanes = 0;
  if (sys.kind == RPT_PARTICLES_MARBLES && n <= SINGLE_COOP) lanes = std::min(64, SINGLE_COOP / pow2ceil(n));
  int d = derivative_only ? 1 : 0;
#define RPT_SINGLE(K, B) hipLaunchKernelGGL((rpt_particles_single<K, B>), dim3(1), dim3(threads), 0, st, n, sys.radius, pos_vel, out, d, nfull, step, do_last ? 1 : 0, last, lanes)
  switch (sys.kind) {
    case RPT_PARTICLES_SOLID_GRAVITY:
      if (threads == SINGLE_COOP) RPT_SINGLE(RPT_PARTICLES_SOLID_GRAVITY, 1); else RPT_SINGLE(RPT_PARTICLES_SOLID_GRAVITY, 2);
      break;
    case RPT_PARTICLES_MARBLES:
      if (threads == SINGLE_COOP) RPT_SINGLE(RPT_PARTICLES_MARBLES, 1); else RPT_SINGLE(RPT_PARTICLES_MARBLES, 2);
      break;
    default:
      if (threads == SINGLE_COOP) RPT_SINGLE(RPT_PARTICLES_CIRCLE, 1); else RPT_SINGLE(RPT_PARTICLES_CIRCLE, 2);
  }
#undef RPT_SINGLE
  return hipGetLastError();
}

static hipError_t stage(const Sys& sys, uint32_t n, const double* src, double* out, double* s, double* ks, double* dst,
                        int stg, double h, hipStream_t st) {
  dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
  switch (sys.kind) {
    case RPT_PARTICLES_SOLID_GRAVITY:
      hipLaunchKernelGGL(rpt_particles_stage<RPT_PARTICLES_SOLID_GRAVITY>, grid, block, 0, st, n, sys.radius, src, out, s, ks, dst, stg, h);
      break;
    case RPT_PARTICLES_MARBLES:
      hipLaunchKernelGGL(rpt_particles_stage<RPT_PARTICLES_MARBLES>, grid, block, 0, st, n, sys.radius, src, out, s, ks, dst, stg, h);
      break;
    default:
      hipLaunchKernelGGL(rpt_particles_stage<RPT_PARTICLES_CIRCLE>, grid, block, 0, st, n, sys.radius, src, out, s, ks, dst, stg, h);
  }
  return hipGetLastError();
}

hipError_t launch_derivative(const Sys& sys, uint32_t n, const double* src, double* out, hipStream_t st) {
  return stage(sys, n, src, out, nullptr, nullptr, nullptr, -1, 0.0, st);
}

hipError_t launch_rk4_step(const Sys& sys, uint32_t n, const GridState& g, double h, hipStream_t st) {
  hipError_t e;
  if ((e = stage(sys, n, g.s, nullptr, g.s, g.ks, g.b, 0, h, st)) != hipSuccess) return e;
  if ((e = stage(sys, n, g.b, nullptr, g.s, g.ks, g.a, 1, h, st)) != hipSuccess) return e;
  if ((e = stage(sys, n, g.a, nullptr, g.s, g.ks, g.b, 2, h, st)) != hipSuccess) return e;
  return stage(sys, n, g.b, nullptr, g.s, g.ks, nullptr, 3, h, st);
}

hipError_t launch_closest_point(double height, uint32_t steps, uint64_t n, const double* pts, double* out, hipStream_t st) {
  hipLaunchKernelGGL(rpt_monomial_closest, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, height, (int)steps, n, pts, out);
  return hipGetLastError();
}

hipError_t launch_hypot(uint64_t n, const double* x, const double* y, double* out, hipStream_t st) {
  hipLaunchKernelGGL(rpt_particles_hypot, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, n, x, y, out);
  return hipGetLastError();
}

} // namespace rptparticles
