// kernels/wavefront.inc — the multi-kernel path pipeline over SoA path state (wf_state.inc): rpt_raygen / _rays / _probes / _views
// [_seeded] (wf_raygen_views.inc), rpt_extend, rpt_shade [_seeded] (wf_shade.inc), rpt_shadow_rays, rpt_shadow_sum, rpt_resolve / _probes, rpt_finish / _probes, rpt_path_permute.
// Its closest-hit and visibility queries over deep trees are the per-tree kernels of tree_query / tree_trace / tree_generic.inc.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// ------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(256) rpt_raygen(Frame fr, Camera cam, PathState ps, uint32_t n_paths) {
  uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_paths) return;
  uint32_t s_local = slot / fr.npix, p_local = slot - s_local * fr.npix;
  uint32_t pixel = fr.pixels[p_local];
  uint32_t y = pixel / fr.width, x = pixel - y * fr.width;
  // renderer.rs:132-134
  double dim = (double)max(fr.width, fr.height);
  double xn = ((double)(2 * x + 1) - (double)fr.width) / dim;
  double yn = ((double)(2 * (fr.height - y) - 1) - (double)fr.height) / dim;
  Rng rng = rng_make(fr.seed, pixel, fr.sample_base + s_local, 0);
  double dx = gen_range(rng, -1.0 / dim, 1.0 / dim); // renderer.rs:137-138
  double dy = gen_range(rng, -1.0 / dim, 1.0 / dim);
  double px = xn + dx, py = yn + dy;
  // Camera::cast_ray camera.rs:64-81 (d and right precomputed on the host, same expressions)
  D3 direction = ld3(cam.direction), up = ld3(cam.up), right = ld3(cam.right);
  D3 origin = ld3(cam.eye);
  D3 new_dir = cam.d * direction + px * right + py * up;
  if (cam.aperture > 0.0) {
    D3 focal_point = origin + normalize(new_dir) * cam.focal_distance;
    double a, b;
    unit_disc(rng, a, b);
    origin = origin + (a * right + b * up) * cam.aperture;
    new_dir = focal_point - origin;
  }
  D3 dir = normalize(new_dir);
  st_soa3(ps.ray, ps.cap, slot, origin);
  st_soa3(ps.ray + 3 * ps.cap, ps.cap, slot, dir);
  ps.draw[slot] = rng.draw;
  ps.pid[slot] = slot; // depth 0: the paths stand in the order of their ids
}

// The same first step for rays the caller made (rptgpu_trace_rays): slot = s_local * npix + p_local starts on ray p_local of
// the piece, read as the caller laid it out ([n][3] f64, origins and dirs already offset to the piece) and used as given
// (no normalisation: rptgpu_closest_hit's rule).  Every sample of a ray starts from the same ray; its stream (fr.pixels[
// p_local], fr.sample_base + s_local) continues at draw first_draw.  ids_out: the caller named no stream ids — ray i of its
// WHOLE array has stream i — so the lanes of the first sample write id_base + p_local where rpt_shade will look for it
// (fr.pixels points at ids_out then).
__global__ void __launch_bounds__(256) rpt_raygen_rays(Frame fr, const double* __restrict__ origins, const double* __restrict__ dirs,
                                                       uint32_t first_draw, uint32_t* __restrict__ ids_out, uint32_t id_base,
                                                       PathState ps, uint32_t n_paths) {
  uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_paths) return;
  uint32_t s_local = slot / fr.npix, p_local = slot - s_local * fr.npix;
  st_soa3(ps.ray, ps.cap, slot, ld3(origins + 3 * (uint64_t)p_local));
  st_soa3(ps.ray + 3 * ps.cap, ps.cap, slot, ld3(dirs + 3 * (uint64_t)p_local));
  ps.draw[slot] = first_draw;
  ps.pid[slot] = slot;
  if (ids_out && s_local == 0) ids_out[p_local] = id_base + p_local;
}

// probe_direction (a light probe's direction from its stream) and sh9_basis: kernels/probe_dir.inc, shared with the rays'
// translation unit (rpt_paths_rays, rpt_project_probes)
#include "probe_dir.inc"

// The first step for light probes: slot = s_local * npix + p_local is direction fr.sample_base + s_local of probe p_local of
// the piece (positions and normals [n][3] f64, already offset to the piece; normals only read for IRRADIANCE).  The path
// leaves the probe's position along the direction and continues the direction's stream where it stopped, as rpt_raygen
// does behind the camera's draws.  ids_out: as rpt_raygen_rays — fr.pixels points there, so the stream id is computed, not
// read (the first sample's lanes are only now writing it).
__global__ void __launch_bounds__(256) rpt_raygen_probes(Frame fr, const double* __restrict__ positions, const double* __restrict__ normals,
                                                         uint32_t kind, uint32_t* __restrict__ ids_out, uint32_t id_base,
                                                         PathState ps, uint32_t n_paths) {
  uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_paths) return;
  uint32_t s_local = slot / fr.npix, p_local = slot - s_local * fr.npix;
  const uint32_t id = ids_out ? id_base + p_local : fr.pixels[p_local];
  const D3 normal = kind == RPT_PROBE_IRRADIANCE ? ld3(normals + 3 * (uint64_t)p_local) : mk(0, 0, 0);
  Rng rng = rng_make(fr.seed, id, fr.sample_base + s_local, 0);
  const D3 dir = probe_direction(kind, normal, rng);
  st_soa3(ps.ray, ps.cap, slot, ld3(positions + 3 * (uint64_t)p_local));
  st_soa3(ps.ray + 3 * ps.cap, ps.cap, slot, dir);
  ps.draw[slot] = rng.draw;
  ps.pid[slot] = slot;
  if (ids_out && s_local == 0) ids_out[p_local] = id;
}

// rpt_raygen_views and rpt_raygen_views_seeded: kernels/wf_raygen_views.inc, once for every seed source (RPT_WF_SEEDED 0: the Frame's seed; 1: a
// seed per view, carried per index of the piece)
#define RPT_WF_SEEDED 0
#include "wf_raygen_views.inc"
#undef RPT_WF_SEEDED
#define RPT_WF_SEEDED 1
#include "wf_raygen_views.inc"
#undef RPT_WF_SEEDED

// closest hit for every queued path.  queue == nullptr means the identity queue (depth 0).
__global__ void __launch_bounds__(256, RPT_WF_WAVES) rpt_extend(Scene sc, PathState ps, const uint32_t* __restrict__ queue,
                                                  uint32_t n) {
  __shared__ KdLdsW kd_lds;
  PROF_INIT();
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t slot = queue ? queue[i] : i;
  D3 o = ld_soa3(ps.ray, ps.cap, slot);
  D3 d = ld_soa3(ps.ray + 3 * ps.cap, ps.cap, slot);
  double t;
  D3 nrm;
  int obj = closest_hit<KdLdsW>(sc, o, d, t, nrm, &kd_lds);
  ps.hit[slot] = t;
  st_soa3(ps.hit + ps.cap, ps.cap, slot, nrm);
  ps.hit_obj[slot] = obj;
  PROF_FLUSH();
}

// stand-alone closest-hit over caller-provided rays (rptgpu_closest_hit)
__global__ void __launch_bounds__(256) rpt_extend_rays(Scene sc, const double* __restrict__ origins,
                                                       const double* __restrict__ dirs, uint64_t n,
                                                       double* __restrict__ out_t, double* __restrict__ out_n,
                                                       int32_t* __restrict__ out_obj) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  D3 o = ld3(origins + 3 * i), d = ld3(dirs + 3 * i);
  double t;
  D3 nrm;
  int obj = closest_hit(sc, o, d, t, nrm);
  out_t[i] = t;
  out_n[3 * i] = nrm.x; out_n[3 * i + 1] = nrm.y; out_n[3 * i + 2] = nrm.z;
  out_obj[i] = obj;
}

// rpt_shade and rpt_shade_seeded: kernels/wf_shade.inc, once for every seed source (RPT_WF_SEEDED 0: the Frame's seed; 1: a
// seed per view, carried per index of the piece)
#define RPT_WF_SEEDED 0
#include "wf_shade.inc"
#undef RPT_WF_SEEDED
#define RPT_WF_SEEDED 1
#include "wf_shade.inc"
#undef RPT_WF_SEEDED

// The visibility test of sample_lights (renderer.rs:191-197) for the paths queued for the depth's lights (rpt_shade's
// per-light queues: hits whose light can add something), scenes without deep trees: one thread per shadow ray, the
// whole scene traversed in the kernel.  ONE launch serves every light of the depth — blockIdx.y is the light, the grid's
// x extent covers the longest queue, a light without rays (ambient ones never have any) costs its blocks one load.  The
// answer goes to srt[light][slot] as a record time — -inf: occluded, +inf: not — which is the form rpt_shadow_sum reads
// for the per-tree queries too.
__global__ void __launch_bounds__(256, RPT_WF_WAVES) rpt_shadow_rays(Scene sc, PathState ps, const uint32_t* __restrict__ sq_all,
                                                                     const uint32_t* __restrict__ sq_counts,
                                                                     double* __restrict__ srt) {
  __shared__ KdLdsW kd_lds;
  PROF_INIT();
  const int light = (int)blockIdx.y;
  const uint32_t* __restrict__ sq = sq_all + (uint64_t)light * ps.cap;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sq_counts[light]) return;
  const uint32_t slot = sq[i];
  const double* sh = ps.shadow + (uint64_t)light * SHADOW_FIELDS * ps.cap;
  D3 pos = ld_soa3(ps.ray, ps.cap, slot);
  D3 wi = ld_soa3(sh, ps.cap, slot);
  double dist = sh[3 * ps.cap + slot];
  srt[(uint64_t)light * ps.cap + slot] = visible<KdLdsW>(sc, pos, wi, dist, &kd_lds) ? INF : -INF;
  PROF_FLUSH();
}

// sample_lights' sum (renderer.rs:186-201) once every shadow ray of the depth has been resolved:
// lights in scene order, starting from zero; A_k = emission + sum (renderer.rs:153-154)
__global__ void __launch_bounds__(256) rpt_shadow_sum(Scene sc, PathState ps, const uint32_t* __restrict__ queue, uint32_t n,
                                                      uint32_t rec_off /* as in rpt_shade */, const double* __restrict__ srt) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t slot = queue ? queue[i] : i;
  if (ps.hit_obj[slot] < 0) return;
  D3 color = mk(0, 0, 0);
  for (int l = 0; l < sc.num_lights; l++) {
    const double* sh = ps.shadow + (uint64_t)l * SHADOW_FIELDS * ps.cap;
    D3 contrib = ld_soa3(sh + 4 * ps.cap, ps.cap, slot);
    if (clight(sc, l).kind == RPT_LIGHT_AMBIENT) {
      color = color + contrib;
    } else if (!null_contribution(contrib)) {
      // (a contribution that is exactly zero was never queued, rpt_shade: its srt entry is stale or was never written,
      // and adding a zero of either sign would change nothing: the sum starts at +0 and is never -0)
      double t_stop = light_stop(sh[3 * ps.cap + slot]);
      if (srt[(uint64_t)l * ps.cap + slot] > t_stop) color = color + contrib; // renderer.rs:197 (false for a NaN hit: visible())
    }
  }
  const uint64_t col = (uint64_t)rec_off + i;
  D3 emit = ld_rec3(ps, 0, col);
  st_rec3(ps, 0, col, emit + color);
}

// trace_ray's value for the path that ended with record c: L = that record's A, then the records above it back to front
// along their links (renderer.rs:162-167)
RPT_DEV D3 fold_path(const PathState& ps, uint32_t c) {
  D3 L = ld_rec3(ps, 0, c);
  for (c = ps.rec_parent[c]; c != REC_NONE; c = ps.rec_parent[c]) {
    D3 A = ld_rec3(ps, 0, c);
    D3 f = ld_rec3(ps, 3, c);
    double inv_pdf = ps.rec[(uint64_t)c * REC_FIELDS + 6], abscos = ps.rec[(uint64_t)c * REC_FIELDS + 7];
    D3 indirect = inv_pdf * cmul(f, L) * abscos;
    L = mk(A.x + fmin(indirect.x, FIREFLY_CLAMP), A.y + fmin(indirect.y, FIREFLY_CLAMP),
           A.z + fmin(indirect.z, FIREFLY_CLAMP));
  }
  return L;
}

// fold the depth records of every sample of a pixel, add to the pixel's running sum
__global__ void __launch_bounds__(256) rpt_resolve(Frame fr, PathState ps, uint32_t n_samples) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= fr.npix) return;
  D3 acc = ld3(fr.accum + 3 * (uint64_t)p);
  for (uint32_t s = 0; s < n_samples; s++) {
    uint64_t slot = (uint64_t)s * fr.npix + p;
    acc = acc + fold_path(ps, ps.last_col[slot]); // the record the path ended with; renderer.rs:139
  }
  fr.accum[3 * (uint64_t)p] = acc.x;
  fr.accum[3 * (uint64_t)p + 1] = acc.y;
  fr.accum[3 * (uint64_t)p + 2] = acc.z;
}

// rpt_resolve for light probes: one thread per probe of the piece, its samples in ascending order.  IRRADIANCE adds every
// path's radiance to the probe's 3 running sums; SH9 weights it by the nine basis functions of the path's FIRST direction —
// made again from the stream (the path state's direction was overwritten at the first bounce) — into 27 sums, [9][3].  The
// sums rest in fr.accum between the passes of a piece, SoA over the piece ([27 or 3][npix]: neighbouring probes, neighbouring
// words), so the order of additions across a pass border is the order within a pass.
__global__ void __launch_bounds__(256) rpt_resolve_probes(Frame fr, PathState ps, uint32_t n_samples, uint32_t kind) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= fr.npix) return;
  if (kind == RPT_PROBE_IRRADIANCE) {
    D3 acc = ld_soa3(fr.accum, fr.npix, p);
    for (uint32_t s = 0; s < n_samples; s++) acc = acc + fold_path(ps, ps.last_col[(uint64_t)s * fr.npix + p]);
    st_soa3(fr.accum, fr.npix, p, acc);
    return;
  }
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] = fr.accum[(uint64_t)k * fr.npix + p];
  const uint32_t id = fr.pixels[p];
  for (uint32_t s = 0; s < n_samples; s++) {
    const D3 L = fold_path(ps, ps.last_col[(uint64_t)s * fr.npix + p]);
    Rng rng = rng_make(fr.seed, id, fr.sample_base + s, 0);
    double Y[9];
    sh9_basis(probe_direction(RPT_PROBE_SH9, mk(0, 0, 0), rng), Y);
#pragma unroll
    for (int j = 0; j < 9; j++) {
      acc[3 * j] = acc[3 * j] + L.x * Y[j];
      acc[3 * j + 1] = acc[3 * j + 1] + L.y * Y[j];
      acc[3 * j + 2] = acc[3 * j + 2] + L.z * Y[j];
    }
  }
#pragma unroll
  for (int k = 0; k < 27; k++) fr.accum[(uint64_t)k * fr.npix + p] = acc[k];
}
// the sums of a piece's probes times `scale` (4 pi / S, pi / S) into the caller's layout, [npix][width]
__global__ void __launch_bounds__(256) rpt_finish_probes(Frame fr, uint32_t width, double scale, double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)fr.npix * width) return;
  const uint64_t p = i / width, k = i - p * width;
  out[i] = fr.accum[k * fr.npix + p] * scale;
}

// ------------------------------------------------------------------ re-ordering the paths of a depth (round 6)
// Scenes whose trees are walked INSIDE rpt_extend / rpt_shadow_rays (no per-tree queue, hence no per-tree sort): the rays
// of a wave are the paths that happen to stand next to each other.  Camera rays do so coherently — node steps at 58 of 64
// lanes on the fractal spheres — but from the first bounce on neighbours point anywhere (31 lanes).  With dense path state
// the order of a depth's paths is free: the survivors' next state (rpt_shade wrote it in the order of their blocks) is
// sorted by the same key the per-tree sort uses — where the ray starts in the scene's bounds, its octant, its direction —
// and gathered into the current arrays in that order.  Scheduling only: every path keeps its id, its stream, its records.
// order == nullptr: in the order rpt_shade wrote them (a depth too small to be worth sorting)
__global__ void __launch_bounds__(256) rpt_path_permute(PathState ps, uint32_t n, const uint32_t* __restrict__ order) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t src = order ? order[j] : j;
  const double2* __restrict__ row = reinterpret_cast<const double2*>(ps.next_rows + (uint64_t)src * 8u);
  const double2 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3]; // one 64-byte sector
  ps.ray[j] = r0.x; ps.ray[ps.cap + j] = r0.y; ps.ray[2 * ps.cap + j] = r1.x;
  ps.ray[3 * ps.cap + j] = r1.y; ps.ray[4 * ps.cap + j] = r2.x; ps.ray[5 * ps.cap + j] = r2.y;
  uint32_t a, b2, c, z;
  unpack_u32(r3.x, a, b2);
  unpack_u32(r3.y, c, z);
  ps.draw[j] = a;
  ps.pid[j] = b2;
  ps.col[j] = c;
}

// color / iterations * 2^EV (renderer.rs:141) into the full frame (zeros elsewhere) — or, `packed`, into a compact
// [npix][3] array in the order of fr.pixels: what a rank sends to the root of the multi-GPU gather
template <typename OutT>
__global__ void __launch_bounds__(256) rpt_finish(Frame fr, double iterations, double ev_scale, OutT* __restrict__ out, int packed) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= fr.npix) return;
  uint64_t pixel = packed ? (uint64_t)p : (uint64_t)fr.pixels[p];
  for (int c = 0; c < 3; c++)
    out[3 * pixel + c] = (OutT)(fr.accum[3 * (uint64_t)p + c] / iterations * ev_scale);
}
// the root of the gather: one rank's packed pixels into their places in the full frame
__global__ void __launch_bounds__(256) rpt_scatter_f32(const float* __restrict__ src, const uint32_t* __restrict__ pixels, uint32_t n,
                                                       float* __restrict__ dst) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint64_t pixel = pixels[p];
  for (int c = 0; c < 3; c++) dst[3 * pixel + c] = src[3 * (uint64_t)p + c];
}
