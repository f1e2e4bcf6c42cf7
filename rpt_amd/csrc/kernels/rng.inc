// kernels/rng.inc — Philox4x32-10 stream and the rand 0.8 / rand_distr 0.4 distributions restated on it.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ Philox4x32-10 stream
// A block yields two u64 draws; the second one is kept in `hi` (valid while draw is odd), so
// the ten rounds run once per two draws.
struct Rng {
  uint32_t k0, k1, pixel, slo, shi, draw;
  uint64_t hi;
};
#ifndef RPT_PHILOX_NOINLINE
#define RPT_PHILOX_NOINLINE 0
#endif
#if RPT_PHILOX_NOINLINE
__device__ __noinline__ void philox_block(
#else
RPT_DEV void philox_block(
#endif
    uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                          uint32_t c3, uint64_t& lo, uint64_t& hi) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  lo = ((uint64_t)c1 << 32) | c0;
  hi = ((uint64_t)c3 << 32) | c2;
}
RPT_DEV Rng rng_make(uint64_t seed, uint32_t pixel, uint64_t sample, uint32_t draw) {
  Rng r{(uint32_t)seed, (uint32_t)(seed >> 32), pixel, (uint32_t)sample, (uint32_t)(sample >> 32), draw, 0};
  if (draw & 1u) { // resuming in the middle of a block (wavefront pipeline): refill the cache
    uint64_t lo;
    philox_block(r.k0, r.k1, pixel, r.slo, r.shi, draw >> 1, lo, r.hi);
  }
  return r;
}
RPT_DEV uint64_t next_u64(Rng& r) {
  uint64_t v;
  if (r.draw & 1u) {
    v = r.hi;
  } else {
    philox_block(r.k0, r.k1, r.pixel, r.slo, r.shi, r.draw >> 1, v, r.hi);
  }
  r.draw++;
  return v;
}
// Two consecutive draws with ONE block computation that every lane runs together.  Lanes of a wave disagree about the
// parity of `draw` (a specular bounce takes one draw more than a diffuse one), and two next_u64 calls in a row then
// run the ten rounds twice, once for the even lanes and once for the odd ones.  Here the block both kinds of lane need
// is block (draw + 1) >> 1: an even lane takes its two halves, an odd lane its cached half and the block's first
// half, the second one becoming the new cache — the same values in the same order as two next_u64 calls.
#ifndef RPT_RNG_PAIR
#define RPT_RNG_PAIR 1 // 0: two next_u64 calls (A/B builds)
#endif
RPT_DEV void next2_u64(Rng& r, uint64_t& a, uint64_t& b) {
#if !RPT_RNG_PAIR
  a = next_u64(r);
  b = next_u64(r);
  return;
#endif
  uint64_t lo, hi;
  philox_block(r.k0, r.k1, r.pixel, r.slo, r.shi, (r.draw + 1u) >> 1, lo, hi);
  if (r.draw & 1u) {
    a = r.hi; b = lo; r.hi = hi;
  } else {
    a = lo; b = hi;
  }
  r.draw += 2u;
}
// Blocks j and j + 1 of a stream in one straight-line run: the two chains' rounds side by side under one key schedule, as
// div_ieee's slots (vec.inc).  Each chain is philox_block's, operation for operation.
RPT_DEV void philox_block2(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t j, uint64_t& lo0,
                           uint64_t& hi0, uint64_t& lo1, uint64_t& hi1) {
  uint32_t a0 = c0, a1 = c1, a2 = c2, a3 = j, b0 = c0, b1 = c1, b2 = c2, b3 = j + 1u;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * a0, q0 = (uint64_t)0xD2511F53u * b0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * a2, q1 = (uint64_t)0xCD9E8D57u * b2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ a1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ a3 ^ k1;
    uint32_t m0 = (uint32_t)(q1 >> 32) ^ b1 ^ k0, m2 = (uint32_t)(q0 >> 32) ^ b3 ^ k1;
    a0 = n0; a1 = (uint32_t)p1; a2 = n2; a3 = (uint32_t)p0;
    b0 = m0; b1 = (uint32_t)q1; b2 = m2; b3 = (uint32_t)q0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  lo0 = ((uint64_t)a1 << 32) | a0;
  hi0 = ((uint64_t)a3 << 32) | a2;
  lo1 = ((uint64_t)b1 << 32) | b0;
  hi1 = ((uint64_t)b3 << 32) | b2;
}
// The stream is random-access: draw k is half k & 1 of block k >> 1, and a lane whose counter d is odd holds draw d in
// `hi`.  A window is the draws d .. d + 3 of every lane of the wave out of ONE issue of blocks (d + 1) >> 1 and the
// next one: an even lane's are the four halves, an odd lane's its cached half and the first three.  `tail`, the second
// block's second half, is draw d + 3 of an even lane and draw d + 4 of an odd one — so it is the half to cache
// whenever the counter behind what the caller consumes, d + 3 or d + 4, is odd (draw_take).  The stream itself is
// left where it was: a caller consumes with draw_take.
struct DrawWindow {
  uint64_t w0, w1, w2, w3, tail;
};
RPT_DEV DrawWindow draw_window(const Rng& r) {
  uint64_t l0, h0, l1, h1;
  philox_block2(r.k0, r.k1, r.pixel, r.slo, r.shi, (r.draw + 1u) >> 1, l0, h0, l1, h1);
  const bool odd = r.draw & 1u;
  return DrawWindow{odd ? r.hi : l0, odd ? l0 : h0, odd ? h0 : l1, odd ? l1 : h1, h1};
}
// the window's first `count` draws are consumed, count = 3 or 4: the stream as that many next_u64 calls leave it
RPT_DEV void draw_take(Rng& r, const DrawWindow& w, uint32_t count) {
  r.draw += count;
  r.hi = w.tail;
}
// rand 0.8 Standard f64: 53 bits in [0,1)
RPT_DEV double gen_f64(Rng& r) { return (double)(next_u64(r) >> 11) * (1.0 / 9007199254740992.0); }
// 52-bit mantissa trick: [1,2) - 1
RPT_DEV double gen_u52(Rng& r) {
  return __longlong_as_double((long long)((next_u64(r) >> 12) | 0x3FF0000000000000ull)) - 1.0;
}
// rand 0.8 UniformFloat::sample_single
RPT_DEV double gen_range(Rng& r, double low, double high) {
  double scale = high - low;
  for (;;) {
    double res = gen_u52(r) * scale + low;
    if (res < high) return res;
  }
}
// rand 0.8 Bernoulli
RPT_DEV bool gen_bool(Rng& r, double p) {
  if (p == 1.0) return true;
  uint64_t p_int = (uint64_t)(p * 18446744073709551616.0);
  return next_u64(r) < p_int;
}
// rand 0.8 UniformInt for Uniform::from(0..n)
RPT_DEV uint64_t gen_index_zone(Rng& r, uint64_t n, uint64_t zone) {
  for (;;) {
    uint64_t v = next_u64(r);
    uint64_t hi = __umul64hi(v, n), lo = v * n;
    if (lo <= zone) return hi;
  }
}
RPT_DEV uint64_t gen_index(Rng& r, uint64_t n) {
  uint64_t ints_to_reject = (0xFFFFFFFFFFFFFFFFull - n + 1) % n;
  uint64_t zone = 0xFFFFFFFFFFFFFFFFull - ints_to_reject;
  for (;;) {
    uint64_t v = next_u64(r);
    uint64_t hi = __umul64hi(v, n), lo = v * n;
    if (lo <= zone) return hi;
  }
}
RPT_DEV double gen_pm1(Rng& r) { return gen_u52(r) * 2.0 + -1.0; }
RPT_DEV double u52_of(uint64_t v) { return __longlong_as_double((long long)((v >> 12) | 0x3FF0000000000000ull)) - 1.0; }
RPT_DEV void gen_pm1_pair(Rng& r, double& x, double& y) { // x = gen_pm1(r); y = gen_pm1(r);
  uint64_t a, b;
  next2_u64(r, a, b);
  x = u52_of(a) * 2.0 + -1.0;
  y = u52_of(b) * 2.0 + -1.0;
}
RPT_DEV void gen_f64_pair(Rng& r, double& x, double& y) { // x = gen_f64(r); y = gen_f64(r);
  uint64_t a, b;
  next2_u64(r, a, b);
  x = (double)(a >> 11) * (1.0 / 9007199254740992.0);
  y = (double)(b >> 11) * (1.0 / 9007199254740992.0);
}
// rand_distr 0.4 UnitDisc / UnitCircle
RPT_DEV void unit_disc(Rng& r, double& x, double& y) {
  for (;;) {
    PROF_COUNT(PF_P_REJECT);
    gen_pm1_pair(r, x, y);
    if (x * x + y * y <= 1.0) return;
  }
}
RPT_DEV void unit_circle(Rng& r, double& ox, double& oy) {
  double x1, x2, sum;
  for (;;) {
    PROF_COUNT(PF_P_REJECT);
    gen_pm1_pair(r, x1, x2);
    sum = x1 * x1 + x2 * x2;
    if (sum < 1.0) break;
  }
  double diff = x1 * x1 - x2 * x2;
  ox = diff / sum;
  oy = 2.0 * x1 * x2 / sum;
}
