// kernels/paths_shade.inc — the fused rpt_paths' draw-first shading: hit_draws, bsdf_opaque, sample_f_opaque, illuminate_mesh.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).
// These functions serve the fused kernels only, so their divisions go in batches (vec.inc div_ieee: div3, normalize_b).

#if RPT_SHADE_SPLIT
// ------------------------------------------------------------------ a hit's draws first, its shading in one block
// The fast form of the fused kernel's shading (rpt_paths<KdFlat, false, true>, RPT_SHADE_SPLIT): a wave whose light is
// an untransformed mesh and whose shading lanes all hit opaque materials (C2).  Every draw of a hit is taken first, in
// the reference's order and by its own loops: illuminate's triangle index and (u, v) pairs until u + v <= 1, then, if
// the path goes on, gen_bool(f), u_theta for the specular lobe and +-1 pairs until one is accepted (sample_f).  What
// the draws decide is kept as their integers, and the shading that follows is one straight-line block.
// (One loop for the whole sequence, a Philox block per lane and round with each lane stepping through its own state
// machine, was measured too: the per-round selects of that state cost far more than the blocks it saved, 25 % slower.)
struct HitDraws {
  uint64_t tri;   // the light triangle's index
  uint64_t a, b;  // the (u, v) pair that was kept
  uint64_t th;    // u_theta's draw (the specular lobe; a dummy 0.5 otherwise)
  uint64_t qa, qb; // the +-1 pair that was kept
  bool spec;      // gen_bool(f)
};
RPT_DEV bool uv_rejected(uint64_t a, uint64_t b) { return (a >> 11) + (b >> 11) >= (1ull << 53) + 2ull; } // u + v > 1
// sf: sample_f runs (depth < max_bounces); f: sample_f's lobe probability; mc (CONSTS): the material's constants, with
// gen_bool(f)'s threshold among them
#if RPT_DRAW_PLAN
// The single draws among them — the index, gen_bool's, u_theta's — are not drawn one by one (next_u64 computes a block
// at the lanes whose counter is even, and the wave pays a whole block issue for it): they come out of blocks that every
// lane computes together with the pair behind them (rng.inc: the stream is random-access).  Which draw feeds which value,
// and where the stream stands afterwards, is what the sequence of calls gives (RPT_DRAW_PLAN 0, below).
template <bool CONSTS = false>
RPT_DEV void hit_draws(Rng& r, bool sf, uint64_t n, uint64_t zone, double f, HitDraws& o, const MatConsts* mc = nullptr) {
  // the index and the first (u, v) pair are draws d, d + 1, d + 2.  Block (d + 1) >> 1 holds all three of an odd lane
  // (with its cached half) and the first two of an even lane, which is then where an odd lane is in front of a pair: the
  // one loop below serves the even lanes' first pair and everybody's redraws, a block per round
  {
    uint64_t lo, hi;
    philox_block(r.k0, r.k1, r.pixel, r.slo, r.shi, (r.draw + 1u) >> 1, lo, hi);
    const bool odd = r.draw & 1u;
    const uint64_t vi = odd ? r.hi : lo;
    bool need, redraw; // need: the lane has no accepted pair yet; redraw: the round it needs follows a rejected pair
    if (__ballot(vi * n > zone) != 0ull) { // some lane's index draw lies outside the zone (below 2^-60 per draw, and
      o.tri = gen_index_zone(r, n, zone);  // never for a power of two): the wave takes the sequence of calls
      next2_u64(r, o.a, o.b);
      need = uv_rejected(o.a, o.b);
      redraw = true;
    } else {
      o.tri = __umul64hi(vi, n);
      o.a = lo; o.b = hi;
      need = odd ? uv_rejected(lo, hi) : true;
      redraw = odd;
      r.hi = hi; // an even lane stands at d + 1 with that draw cached, an odd one at d + 3 with nothing to cache
      r.draw += odd ? 3u : 1u;
    }
    while (need) {
      if (redraw) PROF_COUNT(PF_P_REJECT);
      next2_u64(r, o.a, o.b);
      need = uv_rejected(o.a, o.b);
      redraw = true;
    }
  }
  o.th = 1ull << 63; o.qa = 0; o.qb = 0; o.spec = false;
  if (!sf) return;
  // gen_bool(f) — no draw when f == 1.0 —, u_theta for the specular lobe and the first +-1 pair: three or four draws
  // from the window's front
  const DrawWindow w = draw_window(r);
  const bool gb = f != 1.0;
  uint64_t p_int;
  if constexpr (CONSTS) p_int = mc->p_int;
  else p_int = (uint64_t)(f * 18446744073709551616.0);
  o.spec = gb ? w.w0 < p_int : true;
  const bool four = gb && o.spec; // both single draws in front of the pair; else exactly one of them
  if (o.spec) o.th = gb ? w.w1 : w.w0;
  o.qa = four ? w.w2 : w.w1;
  o.qb = four ? w.w3 : w.w2;
  draw_take(r, w, four ? 4u : 3u);
  for (;;) {
    PROF_COUNT(PF_P_REJECT);
    const double x = u52_of(o.qa) * 2.0 + -1.0, y = u52_of(o.qb) * 2.0 + -1.0;
    const double sum = x * x + y * y;
    if (o.spec ? sum < 1.0 : sum <= 1.0) break;
    next2_u64(r, o.qa, o.qb);
  }
}
#else
template <bool CONSTS = false>
RPT_DEV void hit_draws(Rng& r, bool sf, uint64_t n, uint64_t zone, double f, HitDraws& o, const MatConsts* mc = nullptr) {
  o.tri = gen_index_zone(r, n, zone);
  next2_u64(r, o.a, o.b);
  while ((o.a >> 11) + (o.b >> 11) >= (1ull << 53) + 2ull) {
    PROF_COUNT(PF_P_REJECT);
    next2_u64(r, o.a, o.b);
  }
  o.th = 1ull << 63; o.qa = 0; o.qb = 0; o.spec = false;
  if (!sf) return;
  if constexpr (CONSTS) o.spec = f == 1.0 ? true : next_u64(r) < mc->p_int; // gen_bool: no draw when f == 1.0
  else o.spec = gen_bool(r, f);
  if (o.spec) o.th = next_u64(r);
  for (;;) {
    PROF_COUNT(PF_P_REJECT);
    next2_u64(r, o.qa, o.qb);
    const double x = u52_of(o.qa) * 2.0 + -1.0, y = u52_of(o.qb) * 2.0 + -1.0;
    const double sum = x * x + y * y;
    if (o.spec ? sum < 1.0 : sum <= 1.0) break;
  }
}
#endif

// bsdf() for an opaque material: both directions outside (the reflection case) or zero, its early return a select
// (CONSTS: m2, m2 * PI, f0 and one - f0 from the material's constants)
template <bool CONSTS = false>
RPT_DEV D3 bsdf_opaque(const Material& m, D3 n, D3 wo, D3 wi, const MatConsts* mc = nullptr) { // material.rs:125-170
  D3 color = ld3(m.color);
  double n_dot_wi = dot(n, wi);
  double n_dot_wo = dot(n, wo);
  const bool lit = !__builtin_signbit(n_dot_wi) && !__builtin_signbit(n_dot_wo);
  const D3 one = mk(1, 1, 1);
  double m2, m2pi;
  D3 f0, omf0;
  if constexpr (CONSTS) {
    m2 = mc->m2; m2pi = mc->m2pi;
    f0 = ld3(mc->f0); omf0 = ld3(mc->omf0);
  } else {
    m2 = m.roughness * m.roughness;
    m2pi = m2 * PI;
    double f0s = pow2((m.index - 1.0) / (m.index + 1.0));
    f0 = lerp(mk(f0s, f0s, f0s), color, m.metallic);
    omf0 = one - f0;
  }
  D3 h = normalize_b(wi + wo); // (wi * 1.0 + wo in bsdf)
  double wo_dot_h = dot(wo, h);
  double n_dot_h = dot(n, h);
  double nh2 = pow2(n_dot_h);
#if RPT_DIV_BATCH
  // the exponent of dd and g's quotient wait for nothing of each other: one batch of two
  double ga = n_dot_wi * n_dot_h, gb = n_dot_wo * n_dot_h;
  double g = fmin(ga, gb);
  const double sn[2] = {nh2 - 1.0, 2.0 * g}, sd[2] = {m2 * nh2, wo_dot_h};
  double sq[2];
  div_ieee<2>(sn, sd, sq);
  double dd = rptc_exp(sq[0]) / (m2pi * nh2 * nh2);
  D3 f = f0 + omf0 * pow5(1.0 - wo_dot_h);
  g = sq[1];
#else
  double dd = rptc_exp((nh2 - 1.0) / (m2 * nh2)) / (m2pi * nh2 * nh2);
  D3 f = f0 + omf0 * pow5(1.0 - wo_dot_h);
  double ga = n_dot_wi * n_dot_h, gb = n_dot_wo * n_dot_h;
  double g = fmin(ga, gb);
  g = (2.0 * g) / wo_dot_h;
#endif
  g = fmin(g, 1.0);
  D3 q = div3(dd * f * g, 4.0 * n_dot_wo * n_dot_wi);
  D3 diffuse = div3(cmul(one - f, color), PI);
  return lit ? q + diffuse : mk(0, 0, 0);
}

// sample_f() for an opaque material on the drawn values: both lobes' local vectors, the lane's one behind a select
template <bool CONSTS = false>
RPT_DEV void sample_f_opaque(const Material& m, D3 n, D3 wo, double f, const HitDraws& dr, D3& wi, double& pdf,
                             const MatConsts* mc = nullptr) {
  double m2; // material.rs:224-313
  if constexpr (CONSTS) m2 = mc->m2;
  else m2 = m.roughness * m.roughness;
  const double u_theta = (double)(dr.th >> 11) * (1.0 / 9007199254740992.0);
  const double x = u52_of(dr.qa) * 2.0 + -1.0, y = u52_of(dr.qb) * 2.0 + -1.0;
  const double sum = x * x + y * y;
  double theta = rptc_atan(sqrt(m2 * -rpt_log(u_theta)));
  double sin_t, cos_t;
  rptc_sincos_pio2(theta, &sin_t, &cos_t);
  double diff = x * x - y * y;
  const double cn[2] = {diff, 2.0 * x * y}, cd[2] = {sum, sum}; // cx = diff / sum, cy = 2xy / sum: one batch
  double cq[2];
  div_ieee<2>(cn, cd, cq);
  const double cx = cq[0], cy = cq[1];
  const D3 loc = dr.spec ? mk(cx * sin_t, cy * sin_t, cos_t) : mk(x, y, sqrt(1.0 - x * x - y * y));
  const D3 world = local_to_world_mul(n, loc);
  wi = dr.spec ? -(wo - world * (dot(world, wo) * 2.0)) : world; // -glm::reflect_vec(wo, h)
  double p = 0.0;
  {
    D3 h = normalize_b(wi + wo);
    double p_h;
    if constexpr (CONSTS) { // beckmann_pdf with its PI * m2 from the table (the product m2 * PI: the same number)
      double cos_t = fabs(dot(h, n));
      double sin_t = sqrt(1.0 - cos_t * cos_t);
      p_h = (1.0 / (mc->m2pi * pow3(cos_t))) * rptc_exp(-pow2(sin_t / cos_t) / m2);
    } else {
      p_h = beckmann_pdf(m2, n, h);
    }
    p += f * p_h / (4.0 * fabs(dot(h, wo)));
  }
  p += (1.0 - f) * fmax(dot(wi, n), 0.0) * FRAC_1_PI;
  pdf = p;
}

// illuminate() of an untransformed mesh light on the drawn values (light.rs:23-47, mesh.rs:84-98, kdtree.rs:138-143)
// (CONSTS: Shape::sample's pdf of the drawn triangle, (1 / area) / num_prims, from the wave's table)
template <bool CONSTS = false>
RPT_DEV void illuminate_mesh(CLight& l, CTree& tr, const Tri* __restrict__ tp, D3 pos, const HitDraws& dr, D3& intensity,
                             D3& wi, double& dist, const double* light_pdf = nullptr) {
  const double u = (double)(dr.a >> 11) * (1.0 / 9007199254740992.0), v = (double)(dr.b >> 11) * (1.0 / 9007199254740992.0);
  double w = 1.0 - u - v;
  D3 v1 = ld3(tp->v), v2 = ld3(tp->v + 3), v3 = ld3(tp->v + 6);
  D3 n1 = ld3(tp->v + 9), n2 = ld3(tp->v + 12), n3 = ld3(tp->v + 15);
  SampleOut s{u * v1 + v * v2 + w * v3, normalize_b(u * n1 + v * n2 + w * n3), 0.0};
  if constexpr (CONSTS) {
    s.p = light_pdf[dr.tri];
  } else {
    double area = 0.5 * length(cross(v2 - v1, v3 - v1));
    s.p = 1.0 / area;
    s.p = s.p / (double)tr.num_prims;
  }
  D3 disp = s.v - pos;
  double len = length(disp);
#if RPT_DIV_BATCH
  // cosine and wi = disp / len share the divisor and wait for nothing else: one batch of four
  const double ln[4] = {fmax(-dot(disp, s.n), 0.0), disp.x, disp.y, disp.z}, ld[4] = {len, len, len, len};
  double lq[4];
  div_ieee<4>(ln, ld, lq);
  double cosine = lq[0];
  double surface_area = fmax(cosine, 0.0) / (len * len);
  intensity = div3(ld3(l.mat_color) * l.mat_emittance * surface_area, s.p);
  wi = mk(lq[1], lq[2], lq[3]);
#else
  double cosine = fmax(-dot(disp, s.n), 0.0) / len;
  double surface_area = fmax(cosine, 0.0) / (len * len);
  intensity = ld3(l.mat_color) * l.mat_emittance * surface_area / s.p;
  wi = disp / len;
#endif
  dist = len;
}
#endif
