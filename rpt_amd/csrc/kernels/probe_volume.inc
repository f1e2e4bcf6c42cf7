// kernels/probe_volume.inc — the probe volume's rule and the two kernels that apply it to the caller's points and to first hits
// (include/rpt_gpu_probe_volume.h states every expression; DESIGN.md §26).  One lane per point: the three axes' cells, eight
// tap bases and weights, then the loop j outer, channel inner — per (j, c) the eight taps' products summed in tap order and
// B_j times that sum added to M[c] —, which is the header's order and keeps neither the 27 interpolated coefficients nor 27
// quotients: one division per channel ends it.  The SH9 basis is kernels/sh9_basis.inc's sh9_basis, the bake's own text (kernels/probe_dir.inc includes the same file).
// Compiled in translation units of their own (kernels_probe_volume.hip inside namespace rptvolume; kernels_probe_volume_views.hip
// takes the rule alone, PV_RULE_ONLY), over kernels/vec.inc, with -ffp-contract=off.
// Every loop below has constant bounds and is unrolled: a lane's values are named scalars, nothing is indexed at run time.

struct Cell {
  double f;          // the fraction towards i1
  uint32_t i0, i1;
  bool inside;
};
// step 2 of the rule for one axis: n probes from o on, h apart
RPT_DEV Cell cell_of(double q, double o, double h, uint32_t n) {
  const double top = (double)(n - 1u);
  const double g = (q - o) / h;
  const double s = fmin(fmax(g, 0.0), top);
  const double i0f = floor(s);
  Cell c;
  c.f = s - i0f;
  const int64_t i0 = (int64_t)i0f; // in [0, n - 1]: s is
  c.i0 = (uint32_t)i0;
  c.i1 = i0 + 1 > (int64_t)n - 1 ? n - 1u : (uint32_t)(i0 + 1);
  c.inside = g >= 0.0 && g <= top;
  return c;
}

struct Lit {
  double e0, e1, e2; // E, meaningful when covered
  bool covered, inside;
};
RPT_DEV bool finite3(D3 a) { return fabs(a.x) < PV_INF && fabs(a.y) < PV_INF && fabs(a.z) < PV_INF; }

// the rule at (P, N): steps 1 to 8.  Every tap index is inside the grid whatever P and N are (NaN included: fmax takes 0.0)
RPT_DEV Lit volume_rule(const Volume& v, D3 P, D3 N) {
  const D3 Q = mk(P.x + v.normal_bias * N.x, P.y + v.normal_bias * N.y, P.z + v.normal_bias * N.z);
  const Cell cx = cell_of(Q.x, v.origin[0], v.spacing[0], v.nx);
  const Cell cy = cell_of(Q.y, v.origin[1], v.spacing[1], v.ny);
  const Cell cz = cell_of(Q.z, v.origin[2], v.spacing[2], v.nz);
  const double X[2] = {1.0 - cx.f, cx.f}, Y[2] = {1.0 - cy.f, cy.f}, Z[2] = {1.0 - cz.f, cz.f};
  const uint32_t I[2] = {cx.i0, cx.i1}, J[2] = {cy.i0, cy.i1}, K[2] = {cz.i0, cz.i1};
  const double* __restrict__ tap[8];
  double w[8];
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const int a = t & 1, b = (t >> 1) & 1, c = t >> 2;
    const uint64_t p = ((uint64_t)K[c] * v.ny + J[b]) * v.nx + I[a];
    tap[t] = v.coeffs + 27ull * p;
    const double wt = (X[a] * Y[b]) * Z[c];
    w[t] = (!v.valid || v.valid[p] != 0) ? wt : 0.0;
  }
  const double ws = ((((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]) + w[6]) + w[7];
  Lit r;
  r.inside = cx.inside && cy.inside && cz.inside;
  r.covered = finite3(Q) && finite3(N) && ws > 0.0;
  r.e0 = 0.0; r.e1 = 0.0; r.e2 = 0.0;
  if (r.covered) {
    double Yn[9];
    sh9_basis(N, Yn);
    const double A[9] = {3.141592653589793,  2.0943951023931953, 2.0943951023931953, 2.0943951023931953, 0.7853981633974483,
                         0.7853981633974483, 0.7853981633974483, 0.7853981633974483, 0.7853981633974483};
    double M[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 9; j++) {
      const double B = A[j] * Yn[j];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double S = w[0] * tap[0][3 * j + c];
#pragma unroll
        for (int t = 1; t < 8; t++) S = S + w[t] * tap[t][3 * j + c];
        M[c] = j == 0 ? B * S : M[c] + B * S;
      }
    }
    r.e0 = M[0] / ws; r.e1 = M[1] / ws; r.e2 = M[2] / ws;
  }
  return r;
}

#ifndef PV_RULE_ONLY
__global__ void __launch_bounds__(256) rpt_probe_volume_sample(uint32_t n, Volume v, Points p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Lit r = volume_rule(v, ld3(p.positions + 3ull * i), ld3(p.normals + 3ull * i));
  if (p.channels & RPT_VOLUME_VALUE) {
    double* __restrict__ o = p.value + 3ull * i;
    o[0] = r.covered ? r.e0 : p.fallback[0]; o[1] = r.covered ? r.e1 : p.fallback[1]; o[2] = r.covered ? r.e2 : p.fallback[2];
  }
  if (p.channels & RPT_VOLUME_COVERED) p.covered[i] = r.covered ? 1 : 0;
  if (p.channels & RPT_VOLUME_INSIDE) p.inside[i] = r.inside ? 1 : 0;
}

// (no __restrict__ on the hit arrays and the outputs: a host caller's T, OBJECT, POSITION and NORMAL are rewritten in place —
// everything of ray i is read before anything of it is written, and no lane touches another ray's)
__global__ void __launch_bounds__(256) rpt_probe_volume_lookup(uint32_t n, Volume v, Hits h) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double t = h.t[i];
  const int32_t obj = h.object[i];
  Lit r;
  r.covered = false; r.inside = false; r.e0 = 0.0; r.e1 = 0.0; r.e2 = 0.0;
  D3 P = mk(0.0, 0.0, 0.0), N = mk(0.0, 0.0, 0.0);
  if (obj >= 0) {
    const D3 nrm = ld3(h.normal + 3ull * i), dir = ld3(h.dirs + 3ull * i);
    P = ld3(h.position + 3ull * i);
    const double d = (nrm.x * dir.x + nrm.y * dir.y) + nrm.z * dir.z;
    N = d > 0.0 ? mk(-nrm.x, -nrm.y, -nrm.z) : nrm;
    if (h.channels & (RPT_VOLUME_VALUE | RPT_VOLUME_COVERED | RPT_VOLUME_INSIDE)) r = volume_rule(v, P, N);
  }
  if (h.channels & RPT_VOLUME_T) h.o_t[i] = t;
  if (h.channels & RPT_VOLUME_OBJECT) h.o_object[i] = obj;
  if (h.channels & RPT_VOLUME_POSITION) {
    double* o = h.o_position + 3ull * i;
    o[0] = P.x; o[1] = P.y; o[2] = P.z;
  }
  if (h.channels & RPT_VOLUME_NORMAL) {
    double* o = h.o_normal + 3ull * i;
    o[0] = N.x; o[1] = N.y; o[2] = N.z;
  }
  if (h.channels & RPT_VOLUME_VALUE) {
    double* o = h.o_value + 3ull * i;
    o[0] = r.covered ? r.e0 : h.fallback[0]; o[1] = r.covered ? r.e1 : h.fallback[1]; o[2] = r.covered ? r.e2 : h.fallback[2];
  }
  if (h.channels & RPT_VOLUME_COVERED) h.o_covered[i] = r.covered ? 1 : 0;
  if (h.channels & RPT_VOLUME_INSIDE) h.o_inside[i] = r.inside ? 1 : 0;
}

#ifndef __HIP_DEVICE_COMPILE__
hipError_t sample(hipStream_t st, uint32_t n, const Volume& v, const Points& p) {
  hipLaunchKernelGGL(rpt_probe_volume_sample, dim3(launch_blocks(n)), dim3(BLOCK), 0, st, n, v, p);
  return hipGetLastError();
}
hipError_t lookup(hipStream_t st, uint32_t n, const Volume& v, const Hits& r) {
  hipLaunchKernelGGL(rpt_probe_volume_lookup, dim3(launch_blocks(n)), dim3(BLOCK), 0, st, n, v, r);
  return hipGetLastError();
}
#endif
#endif // PV_RULE_ONLY
