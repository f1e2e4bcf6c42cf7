// kernels/shapes.inc — Sphere / Plane / Cube / MonomialSurface / Triangle intersection, kd-leaf tests.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ primitive intersections
// All follow Shape::intersect's contract (shape.rs:19-21): mutate (rt, rn) and return true only
// when a hit closer than rt was found at t >= t_min.

RPT_DEV bool isect_sphere(D3 o, D3 d, double t_min, double& rt, D3& rn, const bool want_n = true) { // sphere.rs:13-45
  double a = length2(d);
  double b = dot(d, o);
  double c = length2(o) - 1.0;
  double disc = b * b - a * c;
  if (__builtin_signbit(disc)) return false;
  disc = sqrt(disc);
  RcpD ra = rcp_make(a);
  double t = div_r(-b - disc, ra);
  if (t < t_min) {
    t = div_r(-b + disc, ra);
    if (t < t_min) return false;
  }
  if (t < rt) {
    rt = t;
    if (want_n) rn = normalize(o + t * d);
    return true;
  }
  return false;
}

template <class P> RPT_DEV bool isect_plane(P pl, D3 o, D3 d, double t_min, double& rt, D3& rn, const bool want_n = true) {
  // plane.rs:17-32
  D3 n = ld3(pl);
  double cosine = dot(n, d);
  if (fabs(cosine) < 1e-8) return false;
  double time = (pl[3] - dot(n, o)) / cosine;
  if (time >= t_min && time < rt) {
    rt = time;
    if (want_n) rn = (-normalize(n)) * signum(cosine);
    return true;
  }
  return false;
}

// Cube::intersect (cube.rs:20-72) in two steps: everything up to the candidate (time, normal), which does not
// depend on the record, and the accept against record.time.  Split so that two cubes can be evaluated side by side.
template <bool DIVB = false> // the six slab quotients as one batch (vec.inc div6)
RPT_DEV bool cube_candidate(D3 o, const RcpD& rdx, const RcpD& rdy, const RcpD& rdz, double t_min, double& time,
                            D3& normal) {
  // compute_interval per axis: (t1, t2) sorted, s = sign of the ENTRY face normal along the axis
  double x1, x2, y1, y2, z1, z2, sx = -1.0, sy = -1.0, sz = -1.0;
  div6<DIVB>(-0.5 - o.x, 0.5 - o.x, rdx, -0.5 - o.y, 0.5 - o.y, rdy, -0.5 - o.z, 0.5 - o.z, rdz, x1, x2, y1, y2, z1, z2);
  if (x1 > x2) { double t = x1; x1 = x2; x2 = t; sx = 1.0; }
  if (y1 > y2) { double t = y1; y1 = y2; y2 = t; sy = 1.0; }
  if (z1 > z2) { double t = z1; z1 = z2; z2 = t; sz = 1.0; }
  double start, end;
  D3 sn, en; // exit normal is the opposite face of the same axis: -s
  if (x1 > y1 && x1 > z1) { start = x1; sn = mk(sx, 0, 0); }
  else if (y1 > z1) { start = y1; sn = mk(0, sy, 0); }
  else { start = z1; sn = mk(0, 0, sz); }
  if (x2 < y2 && x2 < z2) { end = x2; en = mk(-sx, 0, 0); }
  else if (y2 < z2) { end = y2; en = mk(0, -sy, 0); }
  else { end = z2; en = mk(0, 0, -sz); }
  if (start > end || end < t_min) return false;
  if (start < t_min) { time = end; normal = en; }
  else { time = start; normal = sn; }
  return true;
}
RPT_DEV bool isect_cube(D3 o, const RcpD& rdx, const RcpD& rdy, const RcpD& rdz, double t_min, double& rt,
                        D3& rn) {
  double time = 0.0;
  D3 normal = mk(0, 0, 0);
  if (cube_candidate(o, rdx, rdy, rdz, t_min, time, normal) && time < rt) {
    rt = time;
    rn = normal;
    return true;
  }
  return false;
}

// ---- shapes of the extended set (RPT_EXT_SHAPES builds only).  Inlined into the path kernels this code costs
// scenes that never use it 2-4 % (registers, code size; measured on C2 and C3), and as a real call 11 %, so
// the kernels exist in two builds and a scene gets the extended one only if it contains such a shape.
#ifdef RPT_EXT_SHAPES
// MonomialSurface::intersect (monomial_surface.rs:21-106; exp = 4 only, as the reference :10):
// bounding-box slab test, ten Newton steps on the derivative when the ray starts below the surface,
// then sixty bisection steps.  Everything is +,-,*,/ in the reference's order (powi(2) = s*s,
// powi(3) = t*(t*t)), so the root is reproducible bit for bit on any IEEE machine.
RPT_DEV bool isect_monomial(double height, D3 o, D3 d, const RcpD& rdx, const RcpD& rdy, const RcpD& rdz,
                            double t_min, double& rt, D3& rn, const bool want_n) {
  // BoundingBox::intersect (kdtree.rs:54-68) of [(-1,0,-1), (1,height,1)] (monomial_surface.rs:183-190)
  double x1, x2, y1, y2, z1, z2;
  div6(-1.0 - o.x, 1.0 - o.x, rdx, 0.0 - o.y, height - o.y, rdy, -1.0 - o.z, 1.0 - o.z, rdz, x1, x2, y1, y2, z1, z2);
  double b_min = fmax(fmax(fmin(x1, x2), fmin(y1, y2)), fmin(z1, z2));
  double b_max = fmin(fmin(fmax(x1, x2), fmax(y1, y2)), fmax(z1, z2));
  if (fmax(b_min, t_min) > fmin(b_max, rt)) return false;
  auto dist = [&](double t) {
    double x = o.x + t * d.x, y = o.y + t * d.y, z = o.z + t * d.z;
    double s = x * x + z * z;
    return y - height * (s * s);
  };
  double t_max;
  const bool maximize = dist(t_min) < 0.0;
  if (maximize) {
    double coef0 = o.x * o.x + o.z * o.z;
    double coef1 = 2. * (o.x * d.x + o.z * d.z);
    double coef2 = d.x * d.x + d.z * d.z;
    double cur_x = (b_min + b_max) / 2.;
    for (int i = 0; i < 10; i++) {
      double f = dist(cur_x);
      if (f > 0.) break;
      double t = cur_x;
      double dy1 = 2. * coef0 * coef1 + 2. * t * (coef1 * coef1 + 2. * coef0 * coef2)
                   + 3. * (t * t) * 2. * coef1 * coef2 + 4. * (t * (t * t)) * coef2 * coef2;
      double der = d.y - height * dy1;
      double dy2 = 2. * (coef1 * coef1 + 2. * coef0 * coef2) + 3. * 2. * t * 2. * coef1 * coef2
                   + 4. * 3. * (t * t) * coef2 * coef2;
      double der2 = -height * dy2;
      cur_x -= der / der2;
    }
    t_max = cur_x;
    if (t_max < t_min) return false;
  } else {
    t_max = 10000.;
  }
  if ((dist(t_min) < 0.0) == (dist(t_max) < 0.0)) return false;
  double l = t_min, r = t_max;
#pragma unroll 1
  for (int i = 0; i < 60; i++) {
    double m = (l + r) / 2.0;
    if ((dist(m) >= 0.0) == maximize) r = m;
    else l = m;
  }
  if (r > rt) return false;
  D3 pos = o + r * d;
  double s = pos.x * pos.x + pos.z * pos.z;
  if (s > 1.0) return false;
  rt = r;
  if (want_n) {
    D3 n = normalize(mk(height * 4.0 * pos.x * s, -1.0, height * 4.0 * pos.z * s));
    if (dot(n, d) > 0.0) n = -n; // two-sided
    rn = n;
  }
  return true;
}

#endif // RPT_EXT_SHAPES

// Triangle::intersect (mesh.rs:49-82: plane hit + barycentrics; NOT Moeller-Trumbore, whose
// rounding differs), split in two so that a leaf can issue the loads and the division of several
// triangles before the order-dependent accept step.  plane_normal, d0, d1, d00, d01, d11, denom
// come precomputed (TriX): same operations on the host, same bits.
struct TriPlane {
  double cosine, time;
};
RPT_DEV TriPlane tri_plane(const TriX* __restrict__ tx, D3 o, D3 d) { // mesh.rs:50-58, rt-independent part
  D3 pn = ld3(tx->pn), v1 = ld3(tx->v1);
  TriPlane r;
  r.cosine = dot(pn, d);
  r.time = dot(pn, v1 - o) / r.cosine;
  return r;
}
struct TriBary {
  double u, v, w;
};
RPT_DEV TriBary tri_bary(const TriX* __restrict__ tx, TriPlane pl, D3 o, D3 d) { // mesh.rs:60-72 for a given plane hit
  D3 v1 = ld3(tx->v1), d0 = ld3(tx->d0), d1 = ld3(tx->d1);
  D3 d2 = (o + pl.time * d) - v1;
  double d00 = tx->d00, d01 = tx->d01, d11 = tx->d11, denom = tx->denom;
  double d20 = dot(d2, d0);
  double d21 = dot(d2, d1);
  TriBary b;
  b.v = (d11 * d20 - d01 * d21) / denom;
  b.w = (d00 * d21 - d01 * d20) / denom;
  b.u = 1.0 - b.v - b.w;
  return b;
}
// tri_plane of two records, their two `time` divisions as one batch, and tri_bary of two plane hits, the four
// barycentric quotients as one batch (vec.inc div_ieee): each value is the one the single form computes
RPT_DEV void tri_plane2(const TriX* __restrict__ ta, const TriX* __restrict__ tb, D3 o, D3 d, TriPlane& pa, TriPlane& pb) {
  D3 pna = ld3(ta->pn), v1a = ld3(ta->v1), pnb = ld3(tb->pn), v1b = ld3(tb->v1);
  pa.cosine = dot(pna, d);
  pb.cosine = dot(pnb, d);
  const double n[2] = {dot(pna, v1a - o), dot(pnb, v1b - o)}, c[2] = {pa.cosine, pb.cosine};
  double t[2];
  div_ieee<2>(n, c, t);
  pa.time = t[0];
  pb.time = t[1];
}
RPT_DEV void tri_bary2(const TriX* __restrict__ ta, TriPlane pa, const TriX* __restrict__ tb, TriPlane pb, D3 o, D3 d,
                       TriBary& ba, TriBary& bb) {
  double n[4], c[4], q[4];
  const TriX* __restrict__ tx[2] = {ta, tb};
  const double time[2] = {pa.time, pb.time};
#pragma unroll
  for (int k = 0; k < 2; k++) {
    D3 v1 = ld3(tx[k]->v1), d0 = ld3(tx[k]->d0), d1 = ld3(tx[k]->d1);
    D3 d2 = (o + time[k] * d) - v1;
    double d00 = tx[k]->d00, d01 = tx[k]->d01, d11 = tx[k]->d11;
    double d20 = dot(d2, d0);
    double d21 = dot(d2, d1);
    n[2 * k] = d11 * d20 - d01 * d21;
    n[2 * k + 1] = d00 * d21 - d01 * d20;
    c[2 * k] = c[2 * k + 1] = tx[k]->denom;
  }
  div_ieee<4>(n, c, q);
  ba.v = q[0]; ba.w = q[1]; ba.u = 1.0 - ba.v - ba.w;
  bb.v = q[2]; bb.w = q[3]; bb.u = 1.0 - bb.v - bb.w;
}
template <bool DIVB = false> // the two barycentric quotients and the normal's three as batches
RPT_DEV bool tri_accept(const TriX* __restrict__ tx, const Tri* __restrict__ tris, const uint32_t* __restrict__ refp,
                        TriPlane pl, D3 o, D3 d, double t_min, double& rt, D3& rn, const bool want_n) { // mesh.rs:53-82
  const double time = pl.time;
  if ((fabs(pl.cosine) < 1e-8) | (time < t_min) | (time >= rt)) return false; // (one branch for the three guards)
  D3 v1 = ld3(tx->v1), d0 = ld3(tx->d0), d1 = ld3(tx->d1);
  D3 d2 = (o + time * d) - v1;
  double d00 = tx->d00, d01 = tx->d01, d11 = tx->d11, denom = tx->denom;
  double d20 = dot(d2, d0);
  double d21 = dot(d2, d1);
  double v, w;
  if constexpr (DIVB) {
    const double bn[2] = {d11 * d20 - d01 * d21, d00 * d21 - d01 * d20}, bd[2] = {denom, denom};
    double bq[2];
    div_ieee<2>(bn, bd, bq);
    v = bq[0];
    w = bq[1];
  } else {
    v = (d11 * d20 - d01 * d21) / denom;
    w = (d00 * d21 - d01 * d20) / denom;
  }
  double u = 1.0 - v - w;
  if ((u >= 0.0) & (v >= 0.0) & (w >= 0.0)) {
    rt = time;
    if (want_n) { // the triangle's index is only needed for its vertex normals
      const Tri* tp = tris + *refp;
      D3 n1 = ld3(tp->v + 9), n2 = ld3(tp->v + 12), n3 = ld3(tp->v + 15);
      rn = normalize_t<DIVB>(u * n1 + v * n2 + w * n3);
    }
    return true;
  }
  return false;
}

// Transformed<Sphere|Cube> as a kd-leaf primitive (children of KdTree<Box<dyn Bounded>>).  What a test
// needs of a child — its kind and the 12 used entries of inverse_transform — is fetched as a ChildM one
// entry AHEAD of the test (kd_leaf), so the gather of child i+1 is in flight while child i is tested.
struct ChildM {
  double m[16]; // column-major; rows 3 are never read (Ray::apply_transform, shape.rs:64-71)
  int32_t kind, has_xf;
};
RPT_DEV ChildM ld_child(const Inst* __restrict__ in) {
  ChildM c;
  c.kind = in->kind;
  c.has_xf = in->has_xf;
#pragma unroll
  for (int col = 0; col < 4; col++)
#pragma unroll
    for (int r = 0; r < 3; r++) c.m[4 * col + r] = in->inv[4 * col + r];
  return c;
}
RPT_DEV bool isect_child(const ChildM& c, const Inst* __restrict__ in, D3 o, D3 d, double t_min, double& rt, D3& rn,
                         const bool want_n) {
  D3 lo = o, ld = d;
  if (c.has_xf) { // Ray::apply_transform shape.rs:64-71
    lo = mat4_mul(c.m, o, 1.0);
    ld = mat4_mul(c.m, d, 0.0);
  }
  bool hit;
  if (c.kind == RPT_SHAPE_SPHERE) {
    hit = isect_sphere(lo, ld, t_min, rt, rn, want_n);
  } else {
    RcpD rx = rcp_make(ld.x), ry = rcp_make(ld.y), rz = rcp_make(ld.z);
#ifdef RPT_EXT_SHAPES
    if (c.kind == RPT_SHAPE_MONOMIAL) hit = isect_monomial(in->plane[0], lo, ld, rx, ry, rz, t_min, rt, rn, want_n);
    else
#endif
      hit = isect_cube(lo, rx, ry, rz, t_min, rt, rn);
  }
  if (want_n && hit && c.has_xf) rn = normalize(mat3_mul(in->nrm, rn)); // shape.rs:131-132
  return hit;
}

// up to four consecutive leaf entries: loads and `time` divisions of all of them are issued
// before the order-dependent accept step (m = entries left in the leaf, >= 1)
// DIVB (the fused path kernels): the `time` divisions two by two, a quad's four barycentric quotients and the normal's
// three as batches (tri_plane2, tri_bary2, normalize_b)
template <bool SHADOW, bool DIVB_ = false>
RPT_DEV bool tri_batch(const TriX* __restrict__ recs, const Tri* __restrict__ tris, const uint32_t* __restrict__ refp,
                       uint32_t m, bool pair_only, D3 o, D3 d, double t_min, double& rt, D3& rn) {
  constexpr bool DIVB = DIVB_ && RPT_DIV_BATCH != 0;
  bool found = false, h;
  TriPlane p0, p1;
  if constexpr (DIVB) {
    tri_plane2(recs, recs + (m > 1 ? 1u : 0u), o, d, p0, p1);
  } else {
    p0 = tri_plane(recs, o, d);
    p1 = tri_plane(recs + (m > 1 ? 1u : 0u), o, d);
  }
  if (pair_only) { // a quad's two triangles (polygon(), shape.rs:307-313): no second pair to overlap
    if (m > 1) {
      // Both barycentric evaluations (mesh.rs:60-72) in one straight-line block — they depend on the record only
      // through the `time < record.time` guard — then the two accepts in the reference's order.  A value computed
      // for a triangle whose guard fails is simply not used.
      TriBary b0, b1;
      if constexpr (DIVB) {
        tri_bary2(recs, p0, recs + 1, p1, o, d, b0, b1);
      } else {
        b0 = tri_bary(recs, p0, o, d);
        b1 = tri_bary(recs + 1, p1, o, d);
      }
      int win = -1;
      if (!(fabs(p0.cosine) < 1e-8) && !(p0.time < t_min || p0.time >= rt) && b0.u >= 0.0 && b0.v >= 0.0 && b0.w >= 0.0) {
        rt = p0.time;
        win = 0;
      }
      if (!(fabs(p1.cosine) < 1e-8) && !(p1.time < t_min || p1.time >= rt) && b1.u >= 0.0 && b1.v >= 0.0 && b1.w >= 0.0) {
        rt = p1.time;
        win = 1;
      }
      if (win >= 0 && !SHADOW) { // the normal of the hit that stands (an overwritten first hit never needed one)
        const Tri* tp = tris + refp[win];
        TriBary b = win ? b1 : b0;
        D3 n1 = ld3(tp->v + 9), n2 = ld3(tp->v + 12), n3 = ld3(tp->v + 15);
        rn = normalize_t<DIVB>(b.u * n1 + b.v * n2 + b.w * n3);
      }
      return win >= 0;
    }
    return tri_accept<DIVB>(recs, tris, refp, p0, o, d, t_min, rt, rn, !SHADOW);
  }
  TriPlane p2, p3;
  if constexpr (DIVB) {
    tri_plane2(recs + (m > 2 ? 2u : 0u), recs + (m > 3 ? 3u : 0u), o, d, p2, p3);
  } else {
    p2 = tri_plane(recs + (m > 2 ? 2u : 0u), o, d);
    p3 = tri_plane(recs + (m > 3 ? 3u : 0u), o, d);
  }
  h = tri_accept<DIVB>(recs, tris, refp, p0, o, d, t_min, rt, rn, !SHADOW);
  found = found || h;
  if (m > 1) { h = tri_accept<DIVB>(recs + 1, tris, refp + 1, p1, o, d, t_min, rt, rn, !SHADOW); found = found || h; }
  if (m > 2) { h = tri_accept<DIVB>(recs + 2, tris, refp + 2, p2, o, d, t_min, rt, rn, !SHADOW); found = found || h; }
  if (m > 3) { h = tri_accept<DIVB>(recs + 3, tris, refp + 3, p3, o, d, t_min, rt, rn, !SHADOW); found = found || h; }
  return found;
}

// ---- conservative box filter in front of Triangle::intersect -------------------------------------------------------
// Measured on the reference-rule trees (100k-triangle mesh, 16k-triangle glass): a ray visits ~17 leaves and is tested
// against ~225 / 120 triangles, of which 98 % / 92 % it does not even pass near — the leaves hold up to 15 triangles
// and 44 % of the tests are repeats of a triangle that straddles several leaves.  Each of those tests costs the exact
// f64 arithmetic of mesh.rs:49-82 and 3-8 per-lane 16-byte gathers, and the gathers are what bounds the traversal
// kernel (profiles/r02_*).  So every leaf entry carries a 16-byte conservative box (LeafBox); the ray is first tested
// against the box with cheap arithmetic, and only entries whose box it crosses inside [t_min, record.time] get the
// exact test, in leaf order.
//
// Why this cannot change a result: Triangle::intersect returns true only if t_min <= time < record.time and the
// computed barycentrics are >= 0, i.e. the point o + time*d lies in the triangle up to the rounding of mesh.rs:60-73
// (relative 1e-16 / sin^2 of the triangle's angle; triangles with sin < 1e-5 are never filtered, host_scene.cpp).
// That point is then inside the triangle's box, which the stored box contains with a margin of one grid step
// (1.5e-5 of the mesh extent) on every side, while the f32 slab arithmetic below is off by less than a fifth of a
// step (BoxRay::on guards the operand ranges) and the window is rounded outwards.  Hence an entry the filter rejects is an entry the exact test
// rejects; rejected tests have no side effects; accepted ones run unchanged and in the same order.
struct BoxRay {
  // slab parameter of grid coordinate q on axis k, counted from t0:  t - t0 = q * a_k + b_k.  In f32: the stored boxes
  // have a margin of one grid step = |a_k|, and with t0 at the point where the ray enters the tree's bounds
  // |b_k| <= ~65535 |a_k|, so the f32 evaluation is off by < 0.2 |a_k| (boxray_make guards |b_k| <= 1e6 |a_k|).
  // f32 runs at twice the f64 rate and has min3 / max3; the box tests were 46 % of rpt_tree_trace's instructions.
  float ax, ay, az, bx, by, bz;
  double t0;
  bool on;
};
// An axis the ray does not move along (d_k == 0: every shadow ray towards an axis-aligned directional light has one) has
// no slab parameter; its test is "is the origin's coordinate inside the box on that axis".  The same fma's give
// exactly that with a_k = BOX_PAR and b_k = -BOX_PAR * (the origin's grid coordinate): both faces on the same side of
// the origin -> an interval of +-1e30 * (distance in grid steps), empty against any window and any other axis; faces
// on either side -> (-huge, +huge).  The boxes' margin of one grid step dwarfs the rounding of the grid coordinate.
constexpr double BOX_PAR = 1e30;
// t0: where the box parameters are counted from — max(root slab entry, 0), i.e. a point of the ray inside the bounds
// QUADRIC: the filtered entries may be spheres.  Triangle::intersect and Cube::intersect are linear in the origin: what
// they accept is a point within ~1e-16 |o| of the primitive, so an origin within 1e12 grid steps will do.
// Sphere::intersect (sphere.rs:13-45) forms b^2 - 4ac with b^2 ~ 4ac ~ |o|^2 (object units): it accepts lines that pass
// the unit sphere at up to 1 + ~1e-16 |o|^2, i.e. a far-away origin makes it accept points that are NOT near the
// sphere (a camera 1e10 radii away: by hundreds of radii) — and the reference's result, garbage or not, is the
// contract.  With the origin within 1e7 steps and no filtered sphere smaller than 64 steps (host_scene.cpp,
// quadric_too_small) the excess is below 1e-16 * 1e14 / 64 = 2e-4 steps.
template <bool QUADRIC, class TreeT> RPT_DEV BoxRay boxray_make(const TreeT& tr, D3 o, D3 d, double t0) {
  constexpr double FAR = QUADRIC ? 1e7 : 1e12;
  BoxRay r;
  const bool zx = d.x == 0.0, zy = d.y == 0.0, zz = d.z == 0.0;
  double rx = 1.0 / d.x, ry = 1.0 / d.y, rz = 1.0 / d.z;
  double gx = 0.0, gy = 0.0, gz = 0.0; // the origin's grid coordinates: needed on zero axes only (three divisions)
  if (zx || zy || zz) {
    gx = (o.x - tr.qlo[0]) / tr.qscale[0]; gy = (o.y - tr.qlo[1]) / tr.qscale[1]; gz = (o.z - tr.qlo[2]) / tr.qscale[2];
  }
  double ax = zx ? BOX_PAR : tr.qscale[0] * rx, ay = zy ? BOX_PAR : tr.qscale[1] * ry, az = zz ? BOX_PAR : tr.qscale[2] * rz;
  const double ux = (tr.qlo[0] - o.x) * rx, uy = (tr.qlo[1] - o.y) * ry, uz = (tr.qlo[2] - o.z) * rz; // counted from the origin
  double bx = zx ? -gx * BOX_PAR : ux - t0, by = zy ? -gy * BOX_PAR : uy - t0, bz = zz ? -gz * BOX_PAR : uz - t0;
  // per axis: finite f32 operands; the point o + t0 d within ~1e6 grid steps of the grid (it is inside the bounds
  // unless the caller's t0 is not what it should be); and an origin within 1e12 steps, so that what the f64
  // subtraction u - t0 cancels leaves an error far below a step.  Comparisons with NaN are false: NaN switches it off.
  const bool okx = zx ? fabs(gx) < 1e6 : (fabs(ax) > 1e-30 && fabs(ax) < 1e30 && fabs(bx) < 1e6 * fabs(ax) && fabs(ux) < FAR * fabs(ax));
  const bool oky = zy ? fabs(gy) < 1e6 : (fabs(ay) > 1e-30 && fabs(ay) < 1e30 && fabs(by) < 1e6 * fabs(ay) && fabs(uy) < FAR * fabs(ay));
  const bool okz = zz ? fabs(gz) < 1e6 : (fabs(az) > 1e-30 && fabs(az) < 1e30 && fabs(bz) < 1e6 * fabs(az) && fabs(uz) < FAR * fabs(az));
  r.on = !(zx && zy && zz) && okx && oky && okz && fabs(t0) < 1e300;
  r.ax = (float)ax; r.ay = (float)ay; r.az = (float)az;
  r.bx = (float)bx; r.by = (float)by; r.bz = (float)bz;
  r.t0 = t0;
  return r;
}
// the window [t_lo, t_hi] in the filter's terms: f32, counted from t0, rounded OUTWARDS (one ulp and a bit more).
// A NaN bound stays NaN (t_min is NaN below a 0/0 split, and `time < NaN` rejects nothing in Triangle::intersect:
// the comparisons of leaf_box_pass are written so that it rejects nothing there either); inf - inf = NaN likewise.
RPT_DEV void box_window(const BoxRay& r, double t_lo, double t_hi, float& wl, float& wh) {
  float l = (float)(t_lo - r.t0), h = (float)(t_hi - r.t0);
  wl = l - (fabsf(l) * 1.2e-7f + 1e-30f);
  wh = h + (fabsf(h) * 1.2e-7f + 1e-30f);
}
// does the ray cross the entry's box somewhere in the window?  (false = the exact test would reject)
// Per axis: the centre's slab parameter, then both ends at once (v_pk_fma_f32: half * (-|a|, +|a|) + centre) — the
// near end is the minus one whatever the direction's sign, so no min / max per axis; 17 VALU instructions per box
// where the (min, max) encoding took 26.  Three roundings of <= 0.06 |a| each (|t| <= 1e6 |a|, boxray_make) against
// the boxes' margin of one step = |a|.
typedef float F2 __attribute__((ext_vector_type(2)));
RPT_DEV bool leaf_box_pass(const LeafBox& lb, const BoxRay& r, float wl, float wh) {
  const float cx = (float)(lb.w[0] & 0xffffu), cy = (float)(lb.w[1] & 0xffffu), cz = (float)(lb.w[2] & 0xffffu);
  const float ex = (float)(lb.w[0] >> 16), ey = (float)(lb.w[1] >> 16), ez = (float)(lb.w[2] >> 16);
  const float tx = __builtin_fmaf(cx, r.ax, r.bx), ty = __builtin_fmaf(cy, r.ay, r.by), tz = __builtin_fmaf(cz, r.az, r.bz);
  const float hx = fabsf(r.ax), hy = fabsf(r.ay), hz = fabsf(r.az); // once per batch of boxes: not ray state
  const F2 X = __builtin_elementwise_fma(F2{ex, ex}, F2{-hx, hx}, F2{tx, tx});
  const F2 Y = __builtin_elementwise_fma(F2{ey, ey}, F2{-hy, hy}, F2{ty, ty});
  const F2 Z = __builtin_elementwise_fma(F2{ez, ez}, F2{-hz, hz}, F2{tz, tz});
  const float lo = fmaxf(fmaxf(X.x, Y.x), Z.x), hi = fminf(fminf(X.y, Y.y), Z.y);
  return lo <= hi && !(hi < wl) && !(lo > wh);
}

// a MESH leaf with the filter: boxes of up to 32 entries at a time (four loads in flight), then the exact tests of the
// entries that passed, in leaf order (kdtree.rs:162-171)
template <bool SHADOW, class TreeT>
RPT_DEV bool kd_leaf_boxed(const Scene& sc, const TreeT& tr, const uint32_t* __restrict__ refs, KdNode n, D3 o, D3 d,
                           double t_min, double t_stop, double& rt, D3& rn, const BoxRay& br) {
  bool found = false;
  const uint32_t first = n.a, cnt = n.ib >> 2;
  const TriX* __restrict__ recs = sc.lrec + tr.ref_base + first;
  const LeafBox* __restrict__ boxes = sc.lbox + tr.ref_base + first;
  const Tri* __restrict__ tris = sc.tris + tr.prim_base;
  for (uint32_t base = 0; base < cnt; base += 32u) {
    const uint32_t lim = min(cnt - base, 32u);
    uint32_t m = lim >= 32u ? 0xffffffffu : ((1u << lim) - 1u);
    if (br.on) {
      // a hit beyond the light cannot matter to a visibility query, and record.time only shrinks
      float wl, wh;
      box_window(br, t_min, SHADOW ? fmin(rt, t_stop) : rt, wl, wh);
      m = 0u;
#ifndef RPT_BOX_BATCH
#define RPT_BOX_BATCH 8 // 2 / 4 / 8 / 16 measured: 66.0 / 69.5 / 71.1 / 69.7 Msamples/s on the 100k-triangle mesh
#endif
      for (uint32_t b = 0; b < lim; b += RPT_BOX_BATCH) { // RPT_BOX_BATCH gathers in flight per lane
        PROF_COUNT(PF_TT_BOX);
        LeafBox w[RPT_BOX_BATCH];
#pragma unroll
        for (uint32_t k = 0; k < RPT_BOX_BATCH; k++) w[k] = boxes[base + min(b + k, lim - 1u)]; // (clamped: read unclamped like the group leaves below, C3 loses 0.6 % — a mesh leaf's second batch is mostly past its end)
        uint32_t p = 0u;
#pragma unroll
        for (uint32_t k = 0; k < RPT_BOX_BATCH; k++) p |= (leaf_box_pass(w[k], br, wl, wh) ? 1u : 0u) << k;
        m |= p << b;
      }
      m &= lim >= 32u ? 0xffffffffu : ((1u << lim) - 1u);
    }
    PROF_PHASE(PF_TT_BOX);
    while (m) { // Triangle::intersect of the survivors, first to last
      PROF_COUNT(PF_TT_EXACT);
      const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1u;
      const uint32_t j = base + i;
      TriPlane p = tri_plane(recs + j, o, d);
      bool h = tri_accept(recs + j, tris, refs + first + j, p, o, d, t_min, rt, rn, !SHADOW);
      found = found || h;
      if (SHADOW && rt <= t_stop) break;
    }
    PROF_PHASE(PF_TT_EXACT);
    if (SHADOW && rt <= t_stop) return found;
  }
  return found;
}

struct KdNoLds;

// leaf: test every referenced primitive in order (kdtree.rs:162-171).  SHADOW: the caller only
// needs to know whether some hit has t <= t_stop (renderer.rs:197), so normals are skipped and
// the leaf stops at the first such hit — every accept decision up to that point is the reference's.
// A GROUP leaf here holds placed spheres, cubes and monomial surfaces only: an object whose group has TREE children (a
// mesh or another group, to any depth) never reaches these kernels — the per-tree pipeline walks it with rpt_nest_trace
// or rpt_tree_generic (kernels/tree_trace.inc, tree_generic.inc; scene_plan.h route_object routes by FlatScene::tree_kids).
template <bool TRIS, bool SHADOW, bool DIVB = false /* tri_batch's */, class TreeT>
RPT_DEV bool kd_leaf(const Scene& sc, const TreeT& tr, const uint32_t* __restrict__ refs, KdNode n, D3 o, D3 d,
                     double t_min, double t_stop, double& rt, D3& rn, const BoxRay* br = nullptr) {
  bool found = false;
  uint32_t first = n.a, cnt = n.ib >> 2;
  if (br && br->on && cnt > 2u) { // leaves worth filtering; a quad's two triangles keep the paired path below
    if constexpr (TRIS) {
      return kd_leaf_boxed<SHADOW>(sc, tr, refs, n, o, d, t_min, t_stop, rt, rn, *br);
    } else {
      const LeafBox* __restrict__ boxes = sc.lbox + tr.ref_base + first;
      const Inst* __restrict__ kids = sc.insts + tr.prim_base;
      for (uint32_t base = 0; base < cnt; base += 32u) {
        const uint32_t lim = min(cnt - base, 32u);
        float wl, wh;
        box_window(*br, t_min, SHADOW ? fmin(rt, t_stop) : rt, wl, wh);
        uint32_t m = 0u;
#ifndef RPT_GBOX_BATCH
#define RPT_GBOX_BATCH 4
#endif
        for (uint32_t b = 0; b < lim; b += RPT_GBOX_BATCH) { // RPT_GBOX_BATCH gathers in flight per lane
          PROF_COUNT(PF_IK_BOX);
          LeafBox w[RPT_GBOX_BATCH];
#pragma unroll
          for (uint32_t k = 0; k < RPT_GBOX_BATCH; k++) w[k] = boxes[base + b + k]; // unclamped: one address + immediates; bits past lim are masked below, the array is padded (RPT_LBOX_PAD)
          uint32_t p = 0u;
#pragma unroll
          for (uint32_t k = 0; k < RPT_GBOX_BATCH; k++) p |= (leaf_box_pass(w[k], *br, wl, wh) ? 1u : 0u) << k;
          m |= p << b;
        }
        m &= lim >= 32u ? 0xffffffffu : ((1u << lim) - 1u);
        while (m) { // the children whose box the ray crosses, in leaf order (kdtree.rs:166)
          PROF_COUNT(PF_IK_CHILD);
          const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
          m &= m - 1u;
          const Inst* __restrict__ c = kids + refs[first + base + i];
          ChildM cur = ld_child(c);
          bool h = isect_child(cur, c, o, d, t_min, rt, rn, !SHADOW);
          found = found || h;
          if (SHADOW && rt <= t_stop) return found;
        }
      }
      return found;
    }
  }
  if (TRIS) {
    // intersection records are stored in LEAF order (lrec[j] <-> refs[j]): a leaf is one
    // contiguous run of 128-byte lines, no index gather; four at a time so loads and divisions
    // overlap, then the accept step runs in the reference's order
    const TriX* __restrict__ recs = sc.lrec + tr.ref_base + first;
    const Tri* __restrict__ tris = sc.tris + tr.prim_base;
    for (uint32_t b = 0; b < cnt; b += 4) {
      PROF_COUNT(PF_IK_TRI);
      bool h = tri_batch<SHADOW, DIVB>(recs + b, tris, refs + first + b, cnt - b, cnt <= 2, o, d, t_min, rt, rn);
      found = found || h;
      if (SHADOW && rt <= t_stop) break;
    }
  } else {
    if (cnt == 0) return false; // an empty leaf (kdtree.rs:236 with no objects)
    const Inst* __restrict__ base = sc.insts + tr.prim_base;
    const Inst* __restrict__ c = base + refs[first];
    ChildM cur = ld_child(c);
    for (uint32_t i = 0; i < cnt; i++) {
      PROF_COUNT(PF_IK_CHILD);
      const Inst* __restrict__ cn = c;
      ChildM nx = cur;
      if (i + 1 < cnt) { // the next entry's record is requested before this one is tested
        cn = base + refs[first + i + 1];
        nx = ld_child(cn);
      }
      bool h = isect_child(cur, c, o, d, t_min, rt, rn, !SHADOW);
      found = found || h;
      if (SHADOW && rt <= t_stop) break;
      c = cn;
      cur = nx;
    }
  }
  return found;
}
