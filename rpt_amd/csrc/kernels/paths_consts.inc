// kernels/paths_consts.inc — what rpt_paths keeps of a flat scene in the wave's LDS (FlatLds), and the tables of a hit's scene
// constants that hang off it: MatConsts, mat_consts_of / light_pdf_of / cube_nrm_of, xf_cube_pair, scene_consts_fill.
// Part of kernels.inc (included inside namespace RPT_NS; see that file for the build variants).

// What a flat scene keeps in LDS instead of a traversal stack: its intersection records, triangles, leaf
// entries and per-object materials (every tree has fewer than 16 primitives), read with ds_read at LDS
// latency instead of through L1/L2, which the clamp records keep flushing — and, in what is left of the
// wave's 20 KB stays free (rounds 2-3 kept clamp records there; the fold walker's records live in global memory).
// (the layout of the wave's dynamic LDS, FlatLayout, is computed on the host: flat_layout.h, scene_plan.h plan_flat)
struct FlatLds {
  const TriX* lrec;
  const Tri* tris;
  const uint32_t* refs;
  const Material* obj_mat;           // the material OF object i (not the scene's material table)
  const uint32_t (*obj_leaf)[4];     // MESH objects: ref_base, prim_base, first entry, entry count of the one leaf
  double* qtab;                      // [slots][64 lanes]: this ray's quotients (value - o) / d of the shared planes, the x
                                     // planes' first, then y, then z (as many slots as there are distinct planes)
  const double* plane_vals;          // [3][4] distinct plane coordinates (device memory, read through s_load)
  uint32_t plane_cnt;                // 4 bits per axis; 0 = no table
  // object filter (rpt_paths<KdFlatF>, flat_query_filtered): there obj_leaf[i][3] also carries kind << 8 | has_xf << 16
  const double* obox;                // [objects][6]: bounds of MESH objects
  const LeafBox* obj_box;            // [objects] conservative boxes (device memory, read through s_load)
  const double* obj_grid;            // qlo[3], qscale[3], bounds[6] (device memory, s_load)
  uint64_t obj_always;
  // rpt_paths<KdFlat, false, true, true>: what a hit derives from the scene alone, once per wave (SceneConsts below)
  // — ONE address for the three tables (each one more that the loop keeps costs the kernel scalar registers it has to
  // spill): [objects] MatConsts from it on, behind them [triangles of the light's mesh] doubles, and in front of it, back
  // to front, [cubes in two-cube blocks, in object order][face][3] doubles (mat_consts_of, light_pdf_of, cube_nrm_of)
  const unsigned char* consts;
};
// ------------------------------------------------------------------ a hit's scene constants, once per wave
// SceneConsts (rpt_paths<KdFlat, false, true, true>, RPT_SCENE_CONSTS): the straight-line code of a hit computes values
// that depend on the material, the light's triangle or the cube alone — fixed for the whole launch.  Every wave computes
// them once, in its prologue (scene_consts_fill), with the loop's own expressions on the same operands in the same order,
// so the bits are the loop's; it reads the scene's records from device memory as they stand at the launch, so a live
// update needs nothing more.  Lane `ob` does object `ob`, lane `k` triangle `k` of the light's mesh, lanes 0-11 the
// faces of a two-cube block.  (FlatLds::consts says where the three tables lie.)
// The three groups can be built one by one (A/B builds): RPT_SCENE_CONSTS is a mask, 1 = the materials' constants,
// 2 = the light's pdfs, 4 = the cubes' normals (kernels.h says which ones the default builds, and why).
constexpr bool SC_MAT = (RPT_SCENE_CONSTS & 1) != 0, SC_LIGHT = (RPT_SCENE_CONSTS & 2) != 0, SC_CUBE = (RPT_SCENE_CONSTS & 4) != 0;
struct MatConsts {   // of the material of an object (bsdf_opaque, sample_f_opaque and the kernel's lobe probability)
  double m2, m2pi;   // roughness^2; m2 * PI (bsdf's Beckmann denominator m2 * PI * nh2 * nh2; beckmann_pdf's PI * m2)
  double f0s;        // pow2((index - 1) / (index + 1))
  double f0[3];      // lerp((f0s, f0s, f0s), color, metallic)
  double omf0[3];    // (1, 1, 1) - f0
  double fs;         // sample_f's lobe probability
  uint64_t p_int;    // gen_bool(fs)'s threshold (unused when fs == 1.0: gen_bool then takes no draw)
};
static_assert(sizeof(MatConsts) == RPT_MAT_CONSTS_BYTES, "kernels.h sizes the wave's LDS budget with it");
// a face of the unit cube as cube_candidate names its normals: 2 * axis + (1 if the normal points down the axis)
RPT_DEV D3 cube_face_normal(uint32_t face) {
  const double s = (face & 1u) ? -1.0 : 1.0;
  const uint32_t axis = face >> 1;
  return mk(axis == 0u ? s : 0.0, axis == 1u ? s : 0.0, axis == 2u ? s : 0.0);
}
RPT_DEV const MatConsts* mat_consts_of(const FlatLds* fl, int obj) { return reinterpret_cast<const MatConsts*>(fl->consts) + obj; }
RPT_DEV const double* light_pdf_of(const Scene& sc, const FlatLds* fl) {
  return reinterpret_cast<const double*>(fl->consts + (SC_MAT ? (uint32_t)sc.num_objects : 0u) * (uint32_t)sizeof(MatConsts));
}
RPT_DEV D3 cube_nrm_of(const FlatLds* fl, uint32_t slot, uint32_t face) { // cube `slot` sits slot + 1 cubes in front of fl->consts
  return ld3(reinterpret_cast<const double*>(fl->consts) - (slot + 1u) * 18u + face * 3u);
}
RPT_DEV bool xf_cube_pair(const Scene& sc, int i) { // flat_query's condition for its two-cube block
  return cinst(sc, i).kind == RPT_SHAPE_CUBE && cinst(sc, i).has_xf && i + 1 < sc.num_objects &&
         cinst(sc, i + 1).kind == RPT_SHAPE_CUBE && cinst(sc, i + 1).has_xf;
}
// the prologue's part (all 64 lanes, before the barrier; `tris` = the scene's triangles in device memory)
RPT_DEV void scene_consts_fill(const Scene& sc, const Tri* __restrict__ tris, uint32_t l, unsigned char* consts) {
  MatConsts* mc = reinterpret_cast<MatConsts*>(consts);
  double* light_pdf = reinterpret_cast<double*>(consts + (SC_MAT ? (uint32_t)sc.num_objects : 0u) * (uint32_t)sizeof(MatConsts));
  for (uint32_t ob = l; SC_MAT && ob < (uint32_t)sc.num_objects; ob += 64) {
    const Material& mat = sc.materials[sc.insts[ob].material];
    MatConsts c;
    const D3 color = ld3(mat.color);
    const D3 one = mk(1, 1, 1);
    c.m2 = mat.roughness * mat.roughness;
    c.m2pi = c.m2 * PI;
    c.f0s = pow2((mat.index - 1.0) / (mat.index + 1.0));
    const D3 f0 = lerp(mk(c.f0s, c.f0s, c.f0s), color, mat.metallic);
    const D3 omf0 = one - f0;
    c.f0[0] = f0.x; c.f0[1] = f0.y; c.f0[2] = f0.z;
    c.omf0[0] = omf0.x; c.omf0[1] = omf0.y; c.omf0[2] = omf0.z;
    const double mean = ((color.x + color.y) + color.z) / 3.0;
    double fs = (1.0 - mat.metallic) * c.f0s + mat.metallic * mean;
    fs = fs * (1.0 - 0.2) + 1.0 * 0.2;
    c.fs = fs;
    c.p_int = (uint64_t)(fs * 18446744073709551616.0);
    mc[ob] = c;
  }
  CLight& lg = clight(sc, 0);
  CInst& li = cinst(sc, lg.inst);
  if (SC_LIGHT && lg.kind == RPT_LIGHT_OBJECT && li.kind == RPT_SHAPE_MESH && !li.has_xf) { // illuminate_mesh's light
    CTree& tr = ctree(sc, li.tree);
    for (uint32_t k = l; k < tr.num_prims; k += 64) {
      const Tri* tp = tris + tr.prim_base + k;
      const D3 v1 = ld3(tp->v), v2 = ld3(tp->v + 3), v3 = ld3(tp->v + 6);
      const double area = 0.5 * length(cross(v2 - v1, v3 - v1));
      double p = 1.0 / area;
      p = p / (double)tr.num_prims;
      light_pdf[k] = p;
    }
  }
  uint32_t slot = 0;
  for (int i = 0; SC_CUBE && i < sc.num_objects;) { // the two-cube blocks in the order flat_query meets them
    if (!xf_cube_pair(sc, i)) { i++; continue; }
    if (l < 12u) {
      const uint32_t c = l / 6u, face = l - 6u * c;
      const D3 w = normalize(mat3_mul(sc.insts[i + (int)c].nrm, cube_face_normal(face))); // Transformed::intersect shape.rs:131-132
      double* q = reinterpret_cast<double*>(consts) - (slot + c + 1u) * 18u + face * 3u;
      q[0] = w.x; q[1] = w.y; q[2] = w.z;
    }
    slot += 2u;
    i += 2;
  }
}
