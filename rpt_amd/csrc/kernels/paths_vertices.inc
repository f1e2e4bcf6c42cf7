// kernels/paths_vertices.inc — rpt_paths_vertices: the persistent path kernel over a piece of the caller's rays, leaving every
// path's vertices in the caller's layout as it goes (rptgpu_trace_vertices under RPT_FLAG_VERTICES_PERSISTENT, include/
// rpt_gpu_vertices_persistent.h, DESIGN.md §19.1).  The loop is paths_loop.inc's, the text rpt_paths is compiled from; here
// are what only this form needs — its ray and the three stores of a vertex —, its instantiations and its launchers.
// Addressing: sample s of a launch whose first sample is vo.s_first, of ray p_local of the piece, is path
// p_local * iterations + (s_first + s) of the piece's arrays, and its vertex of depth d entry path * stride + d (64-bit: a
// piece's vertices may pass 2^32).  The kernel writes d < len only; the filler behind a path's last vertex is the host's
// (api_vertices.cpp).  The channel mask is a kernel argument (wave-uniform): a channel that is not asked for is neither
// computed nor stored, and its pointer is never read.  The values are the wavefront route's (kernels/wf_vertices.inc), bit
// for bit: rpt_vertices_store's behind the query, rpt_vertices_fold's from the record and at the path's end.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// the ray of sample `smp` of the piece's index p_local, whose stream id is `id`: caller_ray's of kernels/paths_rays.inc for
// rays (cr.kind < 0, the only kind this form is launched with), word for word — rpt_raygen_rays' ray
RPT_DEV void caller_ray(const Frame& fr, const CallerRays& cr, uint32_t p_local, uint32_t id, uint32_t smp, D3& ro, D3& rd, Rng& rr) {
  ro = ld3(cr.origins + 3 * (uint64_t)p_local);
  rd = ld3(cr.dirs + 3 * (uint64_t)p_local);
  rr = rng_make(fr.seed, id, fr.sample_base + smp, cr.first_draw);
}

RPT_DEV void st_vertex3(double* __restrict__ a, uint64_t v, D3 x) { a[3 * v] = x.x; a[3 * v + 1] = x.y; a[3 * v + 2] = x.z; }
RPT_DEV uint64_t vertex_path_index(const VertexOut& vo, uint32_t p_local, uint32_t s) {
  return (uint64_t)p_local * vo.iterations + ((uint64_t)vo.s_first + s);
}
RPT_DEV uint64_t vertex_index(const VertexOut& vo, uint32_t p_local, uint32_t s, uint32_t depth) {
  return vertex_path_index(vo, p_local, s) * vo.stride + depth;
}
// behind the closest-hit query of a path's depth: the hit, the ray it was made for and the position the stream had when
// that ray was made (rpt_vertices_store's values; POSITION: hit_store's Ray::at, +0.0 on a miss)
RPT_DEV void vertex_hit(const VertexOut& vo, uint64_t v, D3 o, D3 d, double t, D3 nrm, int obj, uint32_t draw) {
  const uint32_t ch = vo.channels;
  if (ch & RPT_VERTEX_T) vo.t[v] = t;
  if (ch & RPT_VERTEX_NORMAL) st_vertex3(vo.normal, v, nrm);
  if (ch & RPT_VERTEX_OBJECT) vo.object[v] = obj;
  if (ch & RPT_VERTEX_DIRECTION) st_vertex3(vo.direction, v, d);
  if (ch & RPT_VERTEX_POSITION) {
    D3 p = mk(0, 0, 0);
    if (obj >= 0) p = o + t * d;
    st_vertex3(vo.position, v, p);
  }
  if (ch & RPT_VERTEX_DRAW) vo.draw[v] = draw;
}
// where a depth's record goes to the ring: the path goes on from this vertex, so all four of its values exist
RPT_DEV void vertex_record(const VertexOut& vo, uint64_t v, D3 A, D3 f, double inv_pdf, double abscos) {
  const uint32_t ch = vo.channels;
  if (ch & RPT_VERTEX_RADIANCE) st_vertex3(vo.radiance, v, A);
  if (ch & RPT_VERTEX_BSDF) st_vertex3(vo.bsdf, v, f);
  if (ch & RPT_VERTEX_INV_PDF) vo.inv_pdf[v] = inv_pdf;
  if (ch & RPT_VERTEX_ABS_COS) vo.abs_cos[v] = abscos;
}
// where a path ends at `depth` with radiance A (on the spot, or when a drain has looked its parked lookup up): the last
// vertex's radiance — its three factors stay the filler — and the path's length
RPT_DEV void vertex_end(const VertexOut& vo, uint32_t p_local, uint32_t s, uint32_t depth, D3 A) {
  const uint32_t ch = vo.channels;
  const uint64_t pi = vertex_path_index(vo, p_local, s);
  if (ch & RPT_VERTEX_RADIANCE) st_vertex3(vo.radiance, pi * vo.stride + depth, A);
  if (ch & RPT_VERTEX_LENGTH) vo.length[pi] = depth + 1u;
}

#define RPT_PATHS_FORM RPT_PATHS_FORM_VERTICES
#include "paths_loop.inc"
#undef RPT_PATHS_FORM

// the instantiations paths_kernel() can pick in this translation unit (kernels/launch_paths.inc): with the ray stash off
// (kernels_vertices_strict[_ext].hip) the plain hand-out of every scene class, parked lookups or not
static_assert(RPT_RAY_STASH == 0, "rpt_paths_vertices: a stashed hit keeps its position, not its t (DESIGN.md §19.1)");
template __global__ void rpt_paths_vertices<KdLds, false>(Scene, Frame, CallerRays, VertexOut, PersistArgs);
template __global__ void rpt_paths_vertices<KdFlat, false>(Scene, Frame, CallerRays, VertexOut, PersistArgs);
template __global__ void rpt_paths_vertices<KdFlat, true>(Scene, Frame, CallerRays, VertexOut, PersistArgs);
template __global__ void rpt_paths_vertices<KdFlatG, false>(Scene, Frame, CallerRays, VertexOut, PersistArgs);
template __global__ void rpt_paths_vertices<KdFlatG, true>(Scene, Frame, CallerRays, VertexOut, PersistArgs);
template __global__ void rpt_paths_vertices<KdFlatF, false>(Scene, Frame, CallerRays, VertexOut, PersistArgs);
template __global__ void rpt_paths_vertices<KdFlatF, true>(Scene, Frame, CallerRays, VertexOut, PersistArgs);

#if !defined(__HIP_DEVICE_COMPILE__)
// the launchers the kernel tables point to (kernels.h)
#define RPT_PATHS_FORM RPT_PATHS_FORM_VERTICES
#include "launch_paths.inc"
#undef RPT_PATHS_FORM
#endif // !__HIP_DEVICE_COMPILE__
