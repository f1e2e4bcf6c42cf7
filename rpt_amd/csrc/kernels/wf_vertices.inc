// kernels/wf_vertices.inc — rptgpu_trace_vertices (include/rpt_gpu_vertices.h, DESIGN.md §19): the vertices of the paths a
// wavefront pass runs, carried into the caller's layout.  Nothing here computes a value of its own; the kernels read what
// the pass's own kernels left in the path state and the depth records:
//   rpt_vertices_store  per depth, behind the closest-hit query and in front of rpt_shade (which overwrites the slot's ray
//                       origin with the hit position): the geometry and the stream position of the depth's paths
//   rpt_vertices_fold   at the end of a pass that resolved, in front of rpt_resolve: every path's record chain, walked as
//                       fold_path walks it, and its length
// The filler behind a path's last vertex is not these kernels': the host fills a piece's arrays before its first pass
// (api_vertices.cpp), and both kernels only ever write d < len (RPT_VERTICES_FILL_IN_KERNEL=1, kernels.h: the measured-and-
// slower form in which rpt_vertices_fold writes it).
// Addressing: path = s_local * npix + p_local (rpt_raygen_rays' slot, carried in PathState::pid through every re-order) is
// sample vo.s_first + s_local of ray p_local of the piece.  The arrays are path-major — (B + 1) entries per path side by
// side — so the lanes of rpt_vertices_store write one entry each, a path's stride apart (the direct form; a column-ordered
// staging area has not been tried), while a lane of rpt_vertices_fold writes its path's entries one after the other.
// The channel mask is a kernel argument (wave-uniform): a channel that is not asked for is neither computed nor stored, and
// its pointer is never read.  Part of kernels.inc (inside namespace RPT_NS).

RPT_DEV void st_vertex3(double* __restrict__ a, uint64_t v, D3 x) { a[3 * v] = x.x; a[3 * v + 1] = x.y; a[3 * v + 2] = x.z; }

// the path's first entry in the per-path arrays (x stride: in the per-vertex arrays)
RPT_DEV uint64_t vertex_path_index(const Frame& fr, const VertexOut& vo, uint32_t path) {
  const uint32_t s_local = path / fr.npix, p_local = path - s_local * fr.npix;
  return (uint64_t)p_local * vo.iterations + (vo.s_first + s_local);
}

// The depth's n paths stand densely in the state arrays (slot i); the hit is the closest-hit query's, the ray still the one
// it was made for.  The record is rptgpu_first_hits' for that ray: hit_store's expressions (kernels/hits.inc).
__global__ void __launch_bounds__(256) rpt_vertices_store(Frame fr, PathState ps, uint32_t n, uint32_t depth, VertexOut vo) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || depth >= vo.stride) return;
  const uint32_t ch = vo.channels;
  const uint64_t v = vertex_path_index(fr, vo, ps.pid[i]) * vo.stride + depth;
  const int obj = ps.hit_obj[i];
  if (ch & RPT_VERTEX_T) vo.t[v] = ps.hit[i];
  if (ch & RPT_VERTEX_NORMAL) st_vertex3(vo.normal, v, ld_soa3(ps.hit + ps.cap, ps.cap, i));
  if (ch & RPT_VERTEX_OBJECT) vo.object[v] = obj;
  if (ch & (RPT_VERTEX_POSITION | RPT_VERTEX_DIRECTION)) {
    const D3 d = ld_soa3(ps.ray + 3 * ps.cap, ps.cap, i);
    if (ch & RPT_VERTEX_DIRECTION) st_vertex3(vo.direction, v, d);
    if (ch & RPT_VERTEX_POSITION) {
      D3 p = mk(0, 0, 0);
      if (obj >= 0) p = ld_soa3(ps.ray, ps.cap, i) + ps.hit[i] * d; // Ray::at: hit_store's and rpt_shade's expression
      st_vertex3(vo.position, v, p);
    }
  }
  if (ch & RPT_VERTEX_DRAW) vo.draw[v] = ps.draw[i];
}

// One thread per path of the pass.  last_col[path] is the record the path ended with (trustworthy once every depth of the
// pass has run); the chain up its parent links is the path back to front: once to count, once to write at d = len-1-k.
// A record's f, 1/pdf and |cos| were written only when the path went on from it — the last record's are stale pool memory
// and are not read.  Entries at d >= len keep the filler the host laid down.
__global__ void __launch_bounds__(256) rpt_vertices_fold(Frame fr, PathState ps, uint32_t n_paths, VertexOut vo) {
  const uint32_t path = blockIdx.x * blockDim.x + threadIdx.x;
  if (path >= n_paths) return;
  const uint32_t ch = vo.channels;
  const uint64_t pi = vertex_path_index(fr, vo, path), v0 = pi * vo.stride;
  const uint32_t c_last = ps.last_col[path];
  uint32_t len = 0;
  for (uint32_t c = c_last; c != REC_NONE && len < vo.stride; c = ps.rec_parent[c]) len++;
  if (ch & RPT_VERTEX_LENGTH) vo.length[pi] = len;
  if (ch & (RPT_VERTEX_RADIANCE | RPT_VERTEX_BSDF | RPT_VERTEX_INV_PDF | RPT_VERTEX_ABS_COS)) {
    uint32_t c = c_last;
    for (uint32_t k = 0; k < len; k++, c = ps.rec_parent[c]) {
      const uint64_t v = v0 + (len - 1u - k);
      if (ch & RPT_VERTEX_RADIANCE) st_vertex3(vo.radiance, v, ld_rec3(ps, 0, c));
      if (ch & RPT_VERTEX_BSDF) st_vertex3(vo.bsdf, v, k ? ld_rec3(ps, 3, c) : mk(0, 0, 0));
      if (ch & RPT_VERTEX_INV_PDF) vo.inv_pdf[v] = k ? ps.rec[(uint64_t)c * REC_FIELDS + 6] : 0.0;
      if (ch & RPT_VERTEX_ABS_COS) vo.abs_cos[v] = k ? ps.rec[(uint64_t)c * REC_FIELDS + 7] : 0.0;
    }
  }
#if RPT_VERTICES_FILL_IN_KERNEL
  for (uint32_t d = len; d < vo.stride; d++) { // the filler: what no vertex of this path wrote
    const uint64_t v = v0 + d;
    const D3 zero = mk(0, 0, 0);
    if (ch & RPT_VERTEX_T) vo.t[v] = 0.0;
    if (ch & RPT_VERTEX_NORMAL) st_vertex3(vo.normal, v, zero);
    if (ch & RPT_VERTEX_OBJECT) vo.object[v] = -1;
    if (ch & RPT_VERTEX_POSITION) st_vertex3(vo.position, v, zero);
    if (ch & RPT_VERTEX_DIRECTION) st_vertex3(vo.direction, v, zero);
    if (ch & RPT_VERTEX_DRAW) vo.draw[v] = 0u;
    if (ch & RPT_VERTEX_RADIANCE) st_vertex3(vo.radiance, v, zero);
    if (ch & RPT_VERTEX_BSDF) st_vertex3(vo.bsdf, v, zero);
    if (ch & RPT_VERTEX_INV_PDF) vo.inv_pdf[v] = 0.0;
    if (ch & RPT_VERTEX_ABS_COS) vo.abs_cos[v] = 0.0;
  }
#endif
}
