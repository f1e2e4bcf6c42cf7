// kernels/vec.inc — 3-vectors, shared-reciprocal division helpers, matrix products (nalgebra's operation order).
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ small vector algebra
struct D3 {
  double x, y, z;
};
RPT_DEV D3 mk(double x, double y, double z) { return D3{x, y, z}; }
RPT_DEV D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
RPT_DEV D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
RPT_DEV D3 operator-(D3 a) { return {-a.x, -a.y, -a.z}; }
RPT_DEV D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
RPT_DEV D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }

// ---- divisions ---------------------------------------------------------------------------------
// Every division the kernels perform yields the IEEE f64 quotient; almost all of them ARE the plain division (div_r).
// RcpD also carries the refined reciprocal of the denominator: hipcc expands a division into div_scale x2, rcp, two
// Newton steps on the reciprocal, q = n*r, e = fma(-d,q,n), div_fmas(e,r,q), div_fixup, and when numerator and
// denominator are in [2^-400, 2^400] nothing is scaled or fixed up, so q = n*r; e = fma(-d,q,n); fma(e,r,q) IS the
// quotient, bit for bit (div_fast; tests/test_gpu_parity.py::test_shared_reciprocal_division_is_ieee, 10^8 operand
// pairs).  ONE place uses that form: the node step of rpt_tree_trace (kernels/tree_trace.inc node_step), per wave, when every ray of
// the wave and the tree qualify (Tree::split_range_ok, safe_coord).  One caveat there: a ZERO numerator gives a zero of
// the sign of num * r, which for num = -0.0 (a split of -0.0 seen from an origin coordinate of +0.0) is not the sign
// IEEE division gives (+0 where it gives -0 for d > 0).  The node step only COMPARES t_split (<= 0, <, >, min / max
// against non-zero bounds), for which the two zeros are the same number; its sign must never be consumed.  Everywhere
// else the shared reciprocal was measured several ways and never paid (DESIGN_HISTORY.md §4.5).
struct RcpD {
  double d, r;
  bool ok;
};
RPT_DEV bool safe_exp(double x) { // 2^-400 <= |x| < 2^400
  uint32_t e = ((uint32_t)(__double_as_longlong(x) >> 52)) & 0x7ffu;
  return e - 623u < 800u;
}
RPT_DEV RcpD rcp_make(double d) {
  RcpD o;
  o.d = d;
  o.ok = safe_exp(d);
  double x = __builtin_amdgcn_rcp(d);
  double e0 = __builtin_fma(-d, x, 1.0);
  double r1 = __builtin_fma(x, e0, x);
  double e1 = __builtin_fma(-d, r1, 1.0);
  o.r = __builtin_fma(r1, e1, r1);
  return o;
}
// the three instructions that ARE the IEEE quotient when n and rc.d are in the safe range (rpt_tree_trace inlines them;
// elsewhere the range check exactness needs costs more than the ~11 instructions it saves: DESIGN_HISTORY.md §4.5,
// variants/node_loop_knobs_and_division_modes.patch); this function serves tests/test_gpu_parity.py::test_shared_reciprocal_division_is_ieee
RPT_DEV double div_fast(double n, const RcpD& rc) {
  double q = n * rc.r;
  double e = __builtin_fma(-rc.d, q, n);
  return __builtin_fma(e, rc.r, q);
}
RPT_DEV bool safe_range(double mn, double mx) { return mn >= 0x1p-400 && mx < 0x1p400; }
// 0, or 2^-340 <= |x| < 2^399: an origin coordinate / split value whose difference with another such value is 0 or
// has a magnitude in [2^-393, 2^400), i.e. is a numerator div_fast is exact for
RPT_DEV bool safe_coord(double x) {
  uint32_t e = ((uint32_t)(__double_as_longlong(x) >> 52)) & 0x7ffu;
  return x == 0.0 || e - 683u < 739u;
}
// v_min_f64 / v_max_f64 themselves: IEEE minNum / maxNum (a quiet NaN operand is ignored, like Rust's f64::min / max).
// fmin / fmax compile to the same instruction PLUS a canonicalisation (v_max_f64 x, x) of every operand that is not
// the result of an arithmetic instruction — loaded values, selected values — which only matters for signalling NaNs;
// no arithmetic produces one.  Used in the hottest loop only (the node step of rpt_tree_trace: five instructions of ~60).
RPT_DEV double fmin_raw(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RPT_DEV double fmax_raw(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RPT_DEV double div_r(double n, const RcpD& rc) { return n / rc.d; }
// N independent IEEE quotients q[k] = n[k] / d[k], issued as one batch (RPT_DIV_BATCH, kernels.h).  The compiler expands
// every f64 `/` into ONE dependent chain of eleven instructions, ten deep, and in the path kernels (256 VGPRs, two waves
// per SIMD) it leaves neighbouring chains one after the other, each paying the wait for VCC in front of v_div_fmas.
// Here every slot performs that expansion op for op, on the same operands — div_scale(d, d, n), rcp, two Newton steps
// on the reciprocal, div_scale(n, d, n) with its flag, the product, its residual, div_fmas under that flag,
// div_fixup(., d, n) — so a slot's result is the bits of n / d for EVERY operand pair, zeros, infinities, NaNs and
// denormals included (they take the route they take in `/`; no range predicate, unlike div_fast above); but the batch
// is written stage by stage, all slots' scales, then all reciprocals, and so on, so that the N chains interleave.
// (tests/test_gpu_div_batch.py: N = 2, 3, 4, 6 against numpy, bit for bit.)  With RPT_DIV_BATCH=0, or in a file that
// takes vec.inc without kernels.h (particles.hip), the slots are the plain `/` in slot order.
template <int N> RPT_DEV void div_ieee(const double (&n)[N], const double (&d)[N], double (&q)[N]) {
#if RPT_DIV_BATCH
  double ds[N], ns[N], r[N], e[N], m[N];
  bool f[N], f0;
#pragma unroll
  for (int k = 0; k < N; k++) ds[k] = __builtin_amdgcn_div_scale(n[k], d[k], false, &f0);
#pragma unroll
  for (int k = 0; k < N; k++) r[k] = __builtin_amdgcn_rcp(ds[k]);
#pragma unroll
  for (int k = 0; k < N; k++) e[k] = __builtin_fma(-ds[k], r[k], 1.0);
#pragma unroll
  for (int k = 0; k < N; k++) r[k] = __builtin_fma(r[k], e[k], r[k]);
#pragma unroll
  for (int k = 0; k < N; k++) e[k] = __builtin_fma(-ds[k], r[k], 1.0);
#pragma unroll
  for (int k = 0; k < N; k++) ns[k] = __builtin_amdgcn_div_scale(n[k], d[k], true, &f[k]);
#pragma unroll
  for (int k = 0; k < N; k++) r[k] = __builtin_fma(r[k], e[k], r[k]);
#pragma unroll
  for (int k = 0; k < N; k++) m[k] = ns[k] * r[k];
#pragma unroll
  for (int k = 0; k < N; k++) e[k] = __builtin_fma(-ds[k], m[k], ns[k]);
#pragma unroll
  for (int k = 0; k < N; k++) m[k] = __builtin_amdgcn_div_fmas(e[k], r[k], m[k], f[k]);
#pragma unroll
  for (int k = 0; k < N; k++) q[k] = __builtin_amdgcn_div_fixup(m[k], d[k], n[k]);
#else
#pragma unroll
  for (int k = 0; k < N; k++) q[k] = n[k] / d[k];
#endif
}
// The batch form costs registers where it stands, and the instantiations of rpt_paths other than the fused ones gain
// VGPR spills and scratch from it (profiles/div_batch_ab.txt), so the shared helpers take it as a template flag, DIVB,
// that only the fused kernels' call chain sets: div6<true>, div3 / normalize_b, normalize_t<DIVB>.  Without the flag a
// helper is the code it always was.
// six slab quotients, two per axis (BoundingBox::intersect kdtree.rs:54-68, Cube::intersect cube.rs:20-37); DIVB: one batch
template <bool DIVB = false>
RPT_DEV void div6(double n0, double n1, const RcpD& rx, double n2, double n3, const RcpD& ry, double n4, double n5,
                  const RcpD& rz, double& q0, double& q1, double& q2, double& q3, double& q4, double& q5) {
  if constexpr (DIVB) {
    const double n[6] = {n0, n1, n2, n3, n4, n5}, d[6] = {rx.d, rx.d, ry.d, ry.d, rz.d, rz.d};
    double q[6];
    div_ieee<6>(n, d, q);
    q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3]; q4 = q[4]; q5 = q[5];
  } else {
    q0 = div_r(n0, rx); q1 = div_r(n1, rx);
    q2 = div_r(n2, ry); q3 = div_r(n3, ry);
    q4 = div_r(n4, rz); q5 = div_r(n5, rz);
  }
}
RPT_DEV D3 operator/(D3 a, double s) {
  RcpD rc = rcp_make(s);
  return {div_r(a.x, rc), div_r(a.y, rc), div_r(a.z, rc)};
}
// a / s with its three quotients as one batch
RPT_DEV D3 div3(D3 a, double s) {
  const double n[3] = {a.x, a.y, a.z}, d[3] = {s, s, s};
  double q[3];
  div_ieee<3>(n, d, q);
  return {q[0], q[1], q[2]};
}
RPT_DEV D3 cmul(D3 a, D3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
// nalgebra's 3-vector dot: the three products summed left to right
RPT_DEV double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RPT_DEV double length2(D3 a) { return dot(a, a); }
RPT_DEV double length(D3 a) { return sqrt(dot(a, a)); }
RPT_DEV D3 normalize(D3 a) { return a / length(a); }
RPT_DEV D3 normalize_b(D3 a) { return div3(a, length(a)); }
template <bool DIVB> RPT_DEV D3 normalize_t(D3 a) {
  if constexpr (DIVB) return normalize_b(a);
  else return normalize(a);
}
RPT_DEV D3 cross(D3 a, D3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <class P> RPT_DEV D3 ld3(P p) { return {p[0], p[1], p[2]}; }
RPT_DEV double sel(int axis, D3 v) { return axis == 0 ? v.x : (axis == 1 ? v.y : v.z); }
RPT_DEV double signum(double x) { return x != x ? x : (__builtin_signbit(x) ? -1.0 : 1.0); }
RPT_DEV bool is_normal(double x) { return __builtin_isnormal(x); }
RPT_DEV double pow2(double x) { return x * x; }
RPT_DEV double pow3(double x) { return x * (x * x); }
RPT_DEV double pow5(double x) { double x2 = x * x; return x * (x2 * x2); }
RPT_DEV D3 lerp(D3 a, D3 b, double t) { return a * (1.0 - t) + b * t; }

// column-major 4x4 * (v, w) and 3x3 * v, accumulated column by column (nalgebra gemv)
template <class P> RPT_DEV D3 mat4_mul(P m, D3 v, double w) {
  D3 r;
  r.x = ((m[0] * v.x + m[4] * v.y) + m[8] * v.z) + m[12] * w;
  r.y = ((m[1] * v.x + m[5] * v.y) + m[9] * v.z) + m[13] * w;
  r.z = ((m[2] * v.x + m[6] * v.y) + m[10] * v.z) + m[14] * w;
  return r;
}
template <class P> RPT_DEV D3 mat3_mul(P m, D3 v) {
  D3 r;
  r.x = (m[0] * v.x + m[3] * v.y) + m[6] * v.z;
  r.y = (m[1] * v.x + m[4] * v.y) + m[7] * v.z;
  r.z = (m[2] * v.x + m[5] * v.y) + m[8] * v.z;
  return r;
}
