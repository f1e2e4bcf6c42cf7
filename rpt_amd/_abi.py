"""ctypes mirror of include/rpt_gpu.h and the loader of the product library.

The product library (`rpt_amd/lib/librptgpu.so`, built by `__graft_entry__.build()` with
hipcc for gfx950) is the ONLY compute path: there is no CPU fallback here.  If the library
is missing, loading raises; if it loads but no GPU is present, every compute entry point
returns RPTGPU_E_NO_DEVICE which is raised as `RptGpuError`.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RPTGPU_LIB") or os.path.join(HERE, "lib", "librptgpu.so")  # RPTGPU_LIB: dev A/B builds

ABI_VERSION = 7

RPTGPU_OK = 0
RPTGPU_E_INVALID_ARGUMENT = -1
RPTGPU_E_UNSUPPORTED_SHAPE = -2
RPTGPU_E_NO_DEVICE = -3
RPTGPU_E_HIP = -4
RPTGPU_E_OUT_OF_MEMORY = -5
RPTGPU_E_TREE_TOO_DEEP = -6
RPTGPU_E_UNIMPLEMENTED_SAMPLE = -7
RPTGPU_E_COMM = -8
RPTGPU_UNIQUE_ID_BYTES = 128

RPT_SHAPE_SPHERE, RPT_SHAPE_PLANE, RPT_SHAPE_CUBE, RPT_SHAPE_MESH, RPT_SHAPE_GROUP, RPT_SHAPE_MONOMIAL = range(6)
RPT_LIGHT_POINT, RPT_LIGHT_AMBIENT, RPT_LIGHT_DIRECTIONAL, RPT_LIGHT_OBJECT = range(4)
RPT_ENV_COLOR, RPT_ENV_HDRI = range(2)
RPT_PRECISION_F64_STRICT = 0  # the only arithmetic mode (ABI v4 removed F64_FAST)
RPT_FLAG_PROFILE_KERNELS = 1
RPT_FLAG_WAVEFRONT = 2
RPT_FLAG_GENERAL_TRAVERSAL = 4
RPT_FLAG_PERSISTENT = 8
RPT_FLAG_VIEWS_PERSISTENT = 16  # include/rpt_gpu_views_persistent.h: RptViewQuery.flags of render_views (views_persistent_supported())
RPT_FLAG_RAYS_PERSISTENT = 32  # include/rpt_gpu_rays_persistent.h: RptRayQuery.flags of trace_rays, RptProbeQuery.flags of bake_probes (rays_persistent_supported())
RPT_FLAG_VERTICES_PERSISTENT = 64  # include/rpt_gpu_vertices_persistent.h: RptVertexQuery.flags of trace_vertices (vertices_persistent_supported())
RPT_K_RAYGEN, RPT_K_EXTEND, RPT_K_SHADE, RPT_K_SHADOW, RPT_K_RESOLVE, RPT_K_PATHS, RPT_K_TREE_TRACE, RPT_K_TREE_SORT = range(8)
RPT_K_COUNT = 8
RPT_PARTICLES_SOLID_GRAVITY, RPT_PARTICLES_MARBLES, RPT_PARTICLES_CIRCLE = range(3)
RPT_PARTICLES_FLAG_SINGLE_GROUP = 1
RPT_PARTICLES_FLAG_GRID = 2
RPT_PARTICLES_SINGLE_MAX = 2048
RPT_PARTICLES_MAX_N = 715827882
RPT_PARTICLES_MAX_STEPS = 1 << 26
RPT_AOV_DEPTH, RPT_AOV_NORMAL, RPT_AOV_ALBEDO, RPT_AOV_POSITION, RPT_AOV_OBJECT = 1, 2, 4, 8, 16
RPT_AOV_ALL = 31
RPT_PROBE_SH9, RPT_PROBE_IRRADIANCE = 0, 1
RPT_VIEW_PERSPECTIVE, RPT_VIEW_ORTHOGRAPHIC, RPT_VIEW_PANORAMA = 0, 1, 2
RPT_HIT_T, RPT_HIT_NORMAL, RPT_HIT_OBJECT, RPT_HIT_POSITION, RPT_HIT_ALBEDO = 1, 2, 4, 8, 16
RPT_HIT_ALL = 31
(RPT_VERTEX_LENGTH, RPT_VERTEX_T, RPT_VERTEX_NORMAL, RPT_VERTEX_OBJECT, RPT_VERTEX_POSITION, RPT_VERTEX_DIRECTION, RPT_VERTEX_DRAW,
 RPT_VERTEX_RADIANCE, RPT_VERTEX_BSDF, RPT_VERTEX_INV_PDF, RPT_VERTEX_ABS_COS, RPT_VERTEX_RGB) = (1 << k for k in range(12))
RPT_VERTEX_ALL = 4095
# include/rpt_gpu_hit_surface.h: RptSurfaceQuery.channels of hit_surface (hit_surface_supported())
RPT_SURFACE_T, RPT_SURFACE_OBJECT, RPT_SURFACE_CHILD, RPT_SURFACE_PRIMITIVE, RPT_SURFACE_BARYCENTRIC = 1, 2, 4, 8, 16
RPT_SURFACE_ALL = 31
# include/rpt_gpu_lightmap.h: RptLightmapQuery.channels of bake_lightmap (lightmap_supported())
(RPT_LIGHTMAP_IRRADIANCE, RPT_LIGHTMAP_AO, RPT_LIGHTMAP_OWNER, RPT_LIGHTMAP_BARYCENTRIC, RPT_LIGHTMAP_POSITION,
 RPT_LIGHTMAP_NORMAL) = 1, 2, 4, 8, 16, 32
RPT_LIGHTMAP_ALL = 63
# include/rpt_gpu_lightmap_lookup.h: RptLookupQuery.channels and .filter of lookup_lightmap (lightmap_lookup_supported())
(RPT_LOOKUP_T, RPT_LOOKUP_OBJECT, RPT_LOOKUP_BINDING, RPT_LOOKUP_COVERED, RPT_LOOKUP_UV, RPT_LOOKUP_VALUE) = 1, 2, 4, 8, 16, 32
RPT_LOOKUP_ALL = 63
RPT_LOOKUP_NEAREST, RPT_LOOKUP_BILINEAR = 0, 1
# include/rpt_gpu_probe_volume.h: RptVolumeQuery.channels of sample_ / lookup_probe_volume (probe_volume_supported())
(RPT_VOLUME_T, RPT_VOLUME_OBJECT, RPT_VOLUME_POSITION, RPT_VOLUME_NORMAL, RPT_VOLUME_VALUE, RPT_VOLUME_COVERED,
 RPT_VOLUME_INSIDE) = 1, 2, 4, 8, 16, 32, 64
RPT_VOLUME_ALL = 127
RPT_VOLUME_POINT = RPT_VOLUME_VALUE | RPT_VOLUME_COVERED | RPT_VOLUME_INSIDE  # what a point has: no ray, no hit

f64 = C.c_double
V3 = f64 * 3


class RptMaterial(C.Structure):
    _fields_ = [("color", V3), ("index", f64), ("roughness", f64), ("metallic", f64),
                ("emittance", f64), ("transparent", C.c_int32), ("_pad", C.c_int32)]


class RptTriangle(C.Structure):
    _fields_ = [("v1", V3), ("v2", V3), ("v3", V3), ("n1", V3), ("n2", V3), ("n3", V3)]


class RptTransform(C.Structure):
    _fields_ = [("transform", f64 * 16), ("linear", f64 * 9), ("inverse_transform", f64 * 16),
                ("normal_transform", f64 * 9), ("scale", f64)]


class RptShape(C.Structure):
    pass


RptShape._fields_ = [("kind", C.c_int32), ("transformed", C.c_int32), ("xf", RptTransform),
                     ("plane_normal", V3), ("plane_value", f64),
                     ("monomial_height", f64), ("monomial_exp", f64),
                     ("triangles", C.POINTER(RptTriangle)), ("num_triangles", C.c_uint64),
                     ("children", C.POINTER(RptShape)), ("num_children", C.c_uint64)]


class RptObject(C.Structure):
    _fields_ = [("shape", RptShape), ("material", RptMaterial)]


class RptLight(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("color", V3), ("vec", V3),
                ("object", RptObject)]


class RptEnvironment(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("color", V3), ("width", C.c_uint32),
                ("height", C.c_uint32), ("texels", C.POINTER(f64))]


class RptScene(C.Structure):
    _fields_ = [("objects", C.POINTER(RptObject)), ("num_objects", C.c_uint64),
                ("lights", C.POINTER(RptLight)), ("num_lights", C.c_uint64),
                ("environment", RptEnvironment)]


class RptCamera(C.Structure):
    _fields_ = [("eye", V3), ("direction", V3), ("up", V3), ("fov", f64), ("aperture", f64),
                ("focal_distance", f64)]


class RptRenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_bounces", C.c_uint32),
                ("iterations", C.c_uint32), ("exposure_value", f64), ("seed", C.c_uint64),
                ("sample_index_base", C.c_uint64), ("tile_width", C.c_uint32),
                ("tile_height", C.c_uint32), ("part_index", C.c_uint32),
                ("part_count", C.c_uint32), ("precision_mode", C.c_uint32),
                ("flags", C.c_uint32), ("collective", C.c_uint32), ("_reserved0", C.c_uint32)]


RPT_COLLECTIVE_DEFAULT, RPT_COLLECTIVE_GATHER, RPT_COLLECTIVE_REDUCE = 0, 1, 2


class RptSceneOptions(C.Structure):
    """include/rpt_gpu.h RptSceneOptions (ABI v6, sized access v7): the knobs of a scene handle; rptgpu_scene_options_default fills it."""
    _fields_ = [("struct_size", C.c_uint32), ("_reserved0", C.c_uint32),
                ("deep_depth", C.c_uint32), ("fast_max_depth", C.c_uint32),
                ("sort_rays", C.c_int32), ("rays_in_kernel", C.c_int32),
                ("sort_min_bytes", C.c_uint64), ("sort_shadow_min_bytes", C.c_uint64),
                ("sort_min_rays", C.c_uint32), ("nest_trace", C.c_int32),
                ("leaf_boxes", C.c_int32), ("object_filter_min", C.c_int32),
                ("device_build_min", C.c_uint64),
                ("build_threads", C.c_uint32), ("paths_chunk", C.c_uint32),
                ("workspace_bytes", C.c_uint64), ("lbuf_bytes", C.c_uint64), ("target_paths", C.c_uint64),
                ("comm_timeout_s", f64),
                ("env_park", C.c_int32), ("paths_batch", C.c_uint32)]


class RptStats(C.Structure):
    _fields_ = [("kernel_ms", f64 * RPT_K_COUNT), ("kernel_launches", C.c_uint64 * RPT_K_COUNT),
                ("extend_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("shadow_rays_traced", C.c_uint64),
                ("samples", C.c_uint64), ("total_ms", f64),
                ("reduce_calls", C.c_uint64), ("reduce_render_ms", f64), ("reduce_collective_ms", f64),
                ("reduce_copy_ms", f64)]


class RptKdTree(C.Structure):
    _fields_ = [("num_nodes", C.c_uint64), ("num_refs", C.c_uint64), ("max_depth", C.c_uint32),
                ("regular", C.c_uint32), ("split", C.POINTER(f64)), ("info", C.POINTER(C.c_uint32)),
                ("a", C.POINTER(C.c_uint32)), ("b", C.POINTER(C.c_uint32)),
                ("refs", C.POINTER(C.c_uint32))]


class RptParticleSystem(C.Structure):
    """include/rpt_gpu.h RptParticleSystem (the reference's rpt::ode systems; detected by symbol within ABI 7)."""
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("radius", f64)]


class RptAdaptive(C.Structure):
    """include/rpt_gpu.h RptAdaptive (the adaptive buffer's stopping rule; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("min_batches", C.c_uint32), ("abs_tol", f64), ("rel_tol", f64)]


class RptAovBuffers(C.Structure):
    """include/rpt_gpu.h RptAovBuffers (rptgpu_render_aov's host arrays; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_uint32), ("hits", C.POINTER(C.c_uint32)),
                ("depth", C.POINTER(f64)), ("normal", C.POINTER(f64)), ("albedo", C.POINTER(f64)),
                ("position", C.POINTER(f64)), ("object", C.POINTER(C.c_int32))]


class RptDenoise(C.Structure):
    """include/rpt_gpu.h RptDenoise (rptgpu_buffer_denoise's parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_uint32), ("sigma_color", f64), ("sigma_normal", f64),
                ("sigma_depth", f64), ("sigma_albedo", f64)]


class RptRayQuery(C.Structure):
    """include/rpt_gpu.h RptRayQuery (rptgpu_trace_rays' parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_bounces", C.c_uint32), ("iterations", C.c_uint32),
                ("first_draw", C.c_uint32), ("exposure_value", f64), ("seed", C.c_uint64),
                ("sample_index_base", C.c_uint64), ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptProbeQuery(C.Structure):
    """include/rpt_gpu.h RptProbeQuery (rptgpu_bake_probes' parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("samples", C.c_uint32), ("max_bounces", C.c_uint32),
                ("seed", C.c_uint64), ("sample_index_base", C.c_uint64), ("precision_mode", C.c_uint32),
                ("flags", C.c_uint32)]


class RptVisibilityQuery(C.Structure):
    """include/rpt_gpu.h RptVisibilityQuery (rptgpu_occluded's parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("precision_mode", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class RptAoQuery(C.Structure):
    """include/rpt_gpu.h RptAoQuery (rptgpu_bake_ao's parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("samples", C.c_uint32), ("seed", C.c_uint64), ("sample_index_base", C.c_uint64),
                ("max_distance", f64), ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptDirectQuery(C.Structure):
    """include/rpt_gpu_direct.h RptDirectQuery (rptgpu_bake_direct's parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("samples", C.c_uint32), ("seed", C.c_uint64), ("sample_index_base", C.c_uint64),
                ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptViewDenoise(C.Structure):
    """include/rpt_gpu_views_denoised.h RptViewDenoise (rptgpu_render_views_denoised's batches, features and filter)."""
    _fields_ = [("struct_size", C.c_uint32), ("batches", C.c_uint32), ("feature_iterations", C.c_uint32), ("_pad", C.c_uint32),
                ("feature_sample_index_base", C.c_uint64), ("filter", RptDenoise)]


class RptViewDenoiseOut(C.Structure):
    """include/rpt_gpu_views_denoised.h RptViewDenoiseOut (rptgpu_render_views_denoised's output arrays; any may be NULL)."""
    _fields_ = [("struct_size", C.c_uint32), ("_pad", C.c_uint32), ("denoised", C.POINTER(f64)), ("rgb8", C.POINTER(C.c_uint8)),
                ("mean", C.POINTER(f64)), ("variance", C.POINTER(f64))]


class RptView(C.Structure):
    """include/rpt_gpu.h RptView (one view of rptgpu_render_views; detected by symbol within ABI 7)."""
    _fields_ = [("camera", RptCamera), ("projection", C.c_uint32), ("_pad", C.c_uint32), ("ortho_scale", f64)]


class RptViewQuery(C.Structure):
    """include/rpt_gpu.h RptViewQuery (rptgpu_render_views' parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("max_bounces", C.c_uint32),
                ("iterations", C.c_uint32), ("_pad", C.c_uint32), ("exposure_value", f64), ("seed", C.c_uint64),
                ("seed_stride", C.c_uint64), ("sample_index_base", C.c_uint64), ("precision_mode", C.c_uint32),
                ("flags", C.c_uint32)]


class RptHitQuery(C.Structure):
    """include/rpt_gpu.h RptHitQuery (rptgpu_first_hits' parameters; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_uint32), ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptHitArrays(C.Structure):
    """include/rpt_gpu.h RptHitArrays (rptgpu_first_hits' output arrays, host or device; detected by symbol within ABI 7)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("t", C.POINTER(f64)), ("normal", C.POINTER(f64)),
                ("object", C.POINTER(C.c_int32)), ("position", C.POINTER(f64)), ("albedo", C.POINTER(f64))]


class RptVertexQuery(C.Structure):
    """include/rpt_gpu_vertices.h RptVertexQuery (rptgpu_trace_vertices' parameters: RptRayQuery's and the channels)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_bounces", C.c_uint32), ("iterations", C.c_uint32),
                ("first_draw", C.c_uint32), ("exposure_value", f64), ("seed", C.c_uint64),
                ("sample_index_base", C.c_uint64), ("precision_mode", C.c_uint32), ("flags", C.c_uint32),
                ("channels", C.c_uint32), ("reserved", C.c_uint32)]


class RptVertexArrays(C.Structure):
    """include/rpt_gpu_vertices.h RptVertexArrays (rptgpu_trace_vertices' output arrays, host or device)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("length", C.POINTER(C.c_uint32)), ("t", C.POINTER(f64)),
                ("normal", C.POINTER(f64)), ("object", C.POINTER(C.c_int32)), ("position", C.POINTER(f64)),
                ("direction", C.POINTER(f64)), ("draw", C.POINTER(C.c_uint32)), ("radiance", C.POINTER(f64)),
                ("bsdf", C.POINTER(f64)), ("inv_pdf", C.POINTER(f64)), ("abs_cos", C.POINTER(f64)), ("rgb", C.POINTER(f64))]


class RptSurfaceQuery(C.Structure):
    """include/rpt_gpu_hit_surface.h RptSurfaceQuery (rptgpu_hit_surface's parameters: RptHitQuery's fields)."""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_uint32), ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptSurfaceArrays(C.Structure):
    """include/rpt_gpu_hit_surface.h RptSurfaceArrays (rptgpu_hit_surface's output arrays, host or device)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("t", C.POINTER(f64)), ("object", C.POINTER(C.c_int32)),
                ("child", C.POINTER(C.c_int32)), ("primitive", C.POINTER(C.c_int32)), ("barycentric", C.POINTER(f64))]


class RptLightmapQuery(C.Structure):
    """include/rpt_gpu_lightmap.h RptLightmapQuery (rptgpu_bake_lightmap's parameters)."""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("samples", C.c_uint32), ("max_bounces", C.c_uint32), ("dilate", C.c_uint32), ("stream_base", C.c_uint32),
                ("seed", C.c_uint64), ("sample_index_base", C.c_uint64), ("offset", f64), ("max_distance", f64),
                ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptLightmapArrays(C.Structure):
    """include/rpt_gpu_lightmap.h RptLightmapArrays (rptgpu_bake_lightmap's output arrays, host or device)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("irradiance", C.POINTER(f64)), ("ao", C.POINTER(f64)),
                ("owner", C.POINTER(C.c_int32)), ("barycentric", C.POINTER(f64)), ("position", C.POINTER(f64)),
                ("normal", C.POINTER(f64))]


class RptLightmapFilter(C.Structure):
    """include/rpt_gpu_lightmap_filter.h RptLightmapFilter (rptgpu_filter_lightmap's parameters)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("words", C.c_uint32),
                ("levels", C.c_uint32), ("dilate", C.c_uint32), ("sigma_normal", f64), ("sigma_plane", f64),
                ("sigma_distance", f64), ("sigma_color", f64)]


class RptLightmapFilterArrays(C.Structure):
    """include/rpt_gpu_lightmap_filter.h RptLightmapFilterArrays (rptgpu_filter_lightmap's arrays, host or device)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("owner", C.POINTER(C.c_int32)), ("position", C.POINTER(f64)),
                ("normal", C.POINTER(f64)), ("values", C.POINTER(f64)), ("variance", C.POINTER(f64)), ("out", C.POINTER(f64)),
                ("out_variance", C.POINTER(f64))]


class RptLightmapBinding(C.Structure):
    """include/rpt_gpu_lightmap_lookup.h RptLightmapBinding (one map tied to one top-level mesh object)."""
    _fields_ = [("struct_size", C.c_uint32), ("object", C.c_uint32), ("n_tris", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("components", C.c_uint32), ("reserved", C.c_uint32), ("uvs", C.POINTER(f64)),
                ("map", C.POINTER(f64)), ("valid", C.POINTER(C.c_uint8))]


class RptLookupQuery(C.Structure):
    """include/rpt_gpu_lightmap_lookup.h RptLookupQuery (rptgpu_lookup_lightmap's parameters)."""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_uint32), ("filter", C.c_uint32), ("fallback", V3),
                ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptLookupArrays(C.Structure):
    """include/rpt_gpu_lightmap_lookup.h RptLookupArrays (rptgpu_lookup_lightmap's output arrays, host or device)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("t", C.POINTER(f64)), ("object", C.POINTER(C.c_int32)),
                ("binding", C.POINTER(C.c_int32)), ("covered", C.POINTER(C.c_uint8)), ("uv", C.POINTER(f64)),
                ("value", C.POINTER(f64))]


class RptViewsLightmapQuery(C.Structure):
    """include/rpt_gpu_lightmap_lookup.h RptViewsLightmapQuery (rptgpu_render_views_lightmapped's parameters beside RptViewQuery)."""
    _fields_ = [("struct_size", C.c_uint32), ("filter", C.c_uint32), ("unbound_irradiance", V3)]


class RptProbeVolume(C.Structure):
    """include/rpt_gpu_probe_volume.h RptProbeVolume (a regular grid of SH9 probes)."""
    _fields_ = [("struct_size", C.c_uint32), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32), ("reserved", C.c_uint32),
                ("origin", V3), ("spacing", V3), ("coeffs", C.POINTER(f64)), ("valid", C.POINTER(C.c_uint8))]


class RptVolumeQuery(C.Structure):
    """include/rpt_gpu_probe_volume.h RptVolumeQuery (rptgpu_sample_ / rptgpu_lookup_probe_volume's parameters)."""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_uint32), ("normal_bias", f64), ("fallback", V3),
                ("precision_mode", C.c_uint32), ("flags", C.c_uint32)]


class RptVolumeArrays(C.Structure):
    """include/rpt_gpu_probe_volume.h RptVolumeArrays (the two calls' output arrays, host or device)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("t", C.POINTER(f64)), ("object", C.POINTER(C.c_int32)),
                ("position", C.POINTER(f64)), ("normal", C.POINTER(f64)), ("value", C.POINTER(f64)),
                ("covered", C.POINTER(C.c_uint8)), ("inside", C.POINTER(C.c_uint8))]


class RptViewsProbeLitQuery(C.Structure):
    """include/rpt_gpu_probe_volume.h RptViewsProbeLitQuery (rptgpu_render_views_probe_lit's parameters beside RptViewQuery)."""
    _fields_ = [("struct_size", C.c_uint32), ("filter", C.c_uint32), ("normal_bias", f64), ("unbound_irradiance", V3)]


# every symbol include/rpt_gpu.h declares: (name, restype, argtypes)
_VP = C.c_void_p
_PD = C.POINTER(f64)
SYMBOLS = [
    ("rptgpu_abi_version", C.c_int, []),
    ("rptgpu_strerror", C.c_char_p, [C.c_int]),
    ("rptgpu_last_error_detail", C.c_char_p, [_VP]),
    ("rptgpu_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("rptgpu_scene_create", C.c_int, [C.POINTER(RptScene), C.c_int, C.POINTER(_VP)]),
    ("rptgpu_scene_destroy", None, [_VP]),
    ("rptgpu_scene_options_default", None, [C.POINTER(RptSceneOptions)]),
    ("rptgpu_scene_options_default_sized", C.c_int, [C.POINTER(RptSceneOptions), C.c_uint32]),
    ("rptgpu_scene_create_opts", C.c_int, [C.POINTER(RptScene), C.c_int, C.POINTER(RptSceneOptions), C.POINTER(_VP)]),
    ("rptgpu_scene_get_options", C.c_int, [_VP, C.POINTER(RptSceneOptions)]),
    ("rptgpu_scene_set_objects", C.c_int, [_VP, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(RptObject)]),
    ("rptgpu_scene_set_lights", C.c_int, [_VP, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(RptLight)]),
    ("rptgpu_scene_set_mesh", C.c_int, [_VP, C.c_uint32, C.c_uint64, C.POINTER(RptTriangle)]),
    ("rptgpu_scene_set_mesh_device", C.c_int, [_VP, C.c_uint32, C.c_uint64, _VP, _VP]),
    ("rptgpu_scene_set_group", C.c_int, [_VP, C.c_uint32, C.c_uint64, C.POINTER(RptShape)]),
    ("rptgpu_scene_set_group_device", C.c_int, [_VP, C.c_uint32, C.c_uint64, _VP, _VP]),
    ("rptgpu_render_batch", C.c_int, [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams), _PD]),
    ("rptgpu_render_batch_device", C.c_int,
     [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams), _VP, C.c_int, _VP]),
    ("rptgpu_comm_unique_id", C.c_int, [C.POINTER(C.c_uint8)]),
    ("rptgpu_comm_init", C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    ("rptgpu_comm_destroy", C.c_int, [_VP]),
    ("rptgpu_render_batch_reduce", C.c_int,
     [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams), C.c_int, C.POINTER(C.c_float)]),
    ("rptgpu_render_batch_emulate_ranks", C.c_int,
     [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams), C.c_int, C.POINTER(C.c_float)]),
    ("rptgpu_closest_hit", C.c_int,
     [_VP, C.c_uint64, _PD, _PD, C.c_uint32, _PD, _PD, C.POINTER(C.c_int32)]),
    ("rptgpu_trace_rays", C.c_int, [_VP, C.c_uint64, _PD, _PD, C.POINTER(C.c_uint32), C.POINTER(RptRayQuery), _PD]),
    ("rptgpu_trace_rays_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptRayQuery), _VP, _VP]),
    ("rptgpu_bake_probes", C.c_int, [_VP, C.c_uint64, _PD, _PD, C.POINTER(C.c_uint32), C.POINTER(RptProbeQuery), _PD]),
    ("rptgpu_bake_probes_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptProbeQuery), _VP, _VP]),
    ("rptgpu_occluded", C.c_int, [_VP, C.c_uint64, _PD, _PD, _PD, C.POINTER(RptVisibilityQuery), C.POINTER(C.c_uint8)]),
    ("rptgpu_occluded_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptVisibilityQuery), _VP, _VP]),
    ("rptgpu_bake_ao", C.c_int, [_VP, C.c_uint64, _PD, _PD, C.POINTER(C.c_uint32), C.POINTER(RptAoQuery), _PD, _PD]),
    ("rptgpu_bake_ao_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptAoQuery), _VP, _VP, _VP]),
    ("rptgpu_render_views", C.c_int, [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), _PD]),
    ("rptgpu_render_views_device", C.c_int, [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), _VP, C.c_int, _VP]),
    ("rptgpu_first_hits", C.c_int, [_VP, C.c_uint64, _PD, _PD, C.POINTER(RptHitQuery), C.POINTER(RptHitArrays)]),
    ("rptgpu_first_hits_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, C.POINTER(RptHitQuery), C.POINTER(RptHitArrays), _VP]),
    ("rptgpu_render_views_aov", C.c_int, [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(RptAovBuffers)]),
    ("rptgpu_render_views_aov_device", C.c_int,
     [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(RptAovBuffers), _VP]),
    ("rptgpu_eval_math", C.c_int, [_VP, C.c_int, C.c_uint64, _PD, _PD, _PD]),
    ("rptgpu_kdtree_build", C.c_int, [_PD, C.c_uint64, C.POINTER(RptKdTree)]),
    ("rptgpu_kdtree_build_device", C.c_int, [_PD, C.c_uint64, C.c_int, C.POINTER(RptKdTree)]),
    ("rptgpu_kdtree_free", None, [C.POINTER(RptKdTree)]),
    ("rptgpu_buffer_create", C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_VP)]),
    ("rptgpu_buffer_destroy", None, [_VP]),
    ("rptgpu_buffer_sample", C.c_int, [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams)]),
    ("rptgpu_buffer_image", C.c_int, [_VP, C.POINTER(C.c_uint8)]),
    ("rptgpu_buffer_variance", C.c_int, [_VP, _PD]),
    ("rptgpu_buffer_num_batches", C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    ("rptgpu_buffer_sample_adaptive", C.c_int,
     [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams), C.POINTER(RptAdaptive), C.POINTER(C.c_uint32)]),
    ("rptgpu_buffer_sample_counts", C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    ("rptgpu_buffer_totals", C.c_int, [_VP, _PD]),
    ("rptgpu_render_aov", C.c_int,
     [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams), C.POINTER(RptAovBuffers)]),
    ("rptgpu_buffer_features", C.c_int, [_VP, C.POINTER(RptCamera), C.POINTER(RptRenderParams)]),
    ("rptgpu_buffer_feature_sums", C.c_int, [_VP, C.POINTER(RptAovBuffers)]),
    ("rptgpu_buffer_denoise", C.c_int, [_VP, C.POINTER(RptDenoise), _PD, C.POINTER(C.c_uint8)]),
    ("rptgpu_get_stats", C.c_int, [_VP, C.POINTER(RptStats)]),
    ("rptgpu_reset_stats", C.c_int, [_VP]),
    ("rptgpu_kernel_name", C.c_char_p, [C.c_int]),
    ("rptgpu_particles_time_derivative", C.c_int,
     [C.c_int, C.POINTER(RptParticleSystem), C.c_uint64, _PD, _PD, _PD, _PD]),
    ("rptgpu_particles_integrate", C.c_int,
     [C.c_int, C.POINTER(RptParticleSystem), C.c_uint64, _PD, _PD, f64, f64]),
    ("rptgpu_monomial_closest_point", C.c_int, [C.c_int, f64, C.c_uint32, C.c_uint64, _PD, _PD]),
    ("rptgpu_particles_eval_hypot", C.c_int, [C.c_int, C.c_uint64, _PD, _PD, _PD]),
]
# ... and every symbol include/rpt_gpu_views_seeded.h declares: the optional additions within ABI 7 that a binding detects by
# symbol.  This package's own library always has them, so load_library binds them like the rest
SEEDED_SYMBOLS = [
    ("rptgpu_render_views_seeded", C.c_int,
     [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(C.c_uint64), _PD]),
    ("rptgpu_render_views_seeded_device", C.c_int,
     [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(C.c_uint64), _VP, C.c_int, _VP]),
    ("rptgpu_render_views_aov_seeded", C.c_int,
     [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(C.c_uint64), C.POINTER(RptAovBuffers)]),
    ("rptgpu_render_views_aov_seeded_device", C.c_int,
     [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(C.c_uint64), C.POINTER(RptAovBuffers), _VP]),
]
# ... and every symbol include/rpt_gpu_views_denoised.h declares, optional in the same way
DENOISED_SYMBOLS = [
    ("rptgpu_render_views_denoised", C.c_int,
     [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(C.c_uint64), C.POINTER(RptViewDenoise),
      C.POINTER(RptViewDenoiseOut)]),
    ("rptgpu_render_views_denoised_device", C.c_int,
     [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.POINTER(C.c_uint64), C.POINTER(RptViewDenoise),
      C.POINTER(RptViewDenoiseOut), _VP]),
]
# ... and every symbol include/rpt_gpu_vertices.h declares, optional in the same way
VERTICES_SYMBOLS = [
    ("rptgpu_trace_vertices", C.c_int,
     [_VP, C.c_uint64, _PD, _PD, C.POINTER(C.c_uint32), C.POINTER(RptVertexQuery), C.POINTER(RptVertexArrays)]),
    ("rptgpu_trace_vertices_device", C.c_int,
     [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptVertexQuery), C.POINTER(RptVertexArrays), _VP]),
]
# ... and the symbol include/rpt_gpu_views_persistent.h declares, optional in the same way: a library without it ignores
# RPT_FLAG_VIEWS_PERSISTENT and runs the wavefront pipeline (views_persistent_supported)
VIEWS_PERSISTENT_SYMBOLS = [
    ("rptgpu_views_persistent_supported", C.c_int, []),
]
# ... and the symbol include/rpt_gpu_rays_persistent.h declares, optional in the same way: a library without it ignores
# RPT_FLAG_RAYS_PERSISTENT and runs the wavefront pipeline (rays_persistent_supported) — and load_library tolerates such a
# library (an older build, for a comparison)
RAYS_PERSISTENT_SYMBOLS = [
    ("rptgpu_rays_persistent_supported", C.c_int, []),
]
# ... and the symbol include/rpt_gpu_vertices_persistent.h declares, optional in the same way: a library without it ignores
# RPT_FLAG_VERTICES_PERSISTENT and runs the wavefront pipeline (vertices_persistent_supported)
VERTICES_PERSISTENT_SYMBOLS = [
    ("rptgpu_vertices_persistent_supported", C.c_int, []),
]
# ... and every symbol include/rpt_gpu_hit_surface.h declares, optional in the same way: load_library tolerates a library
# without them (an older build, for a comparison), and hit_surface_supported() says which it is
HIT_SURFACE_SYMBOLS = [
    ("rptgpu_hit_surface", C.c_int, [_VP, C.c_uint64, _PD, _PD, C.POINTER(RptSurfaceQuery), C.POINTER(RptSurfaceArrays)]),
    ("rptgpu_hit_surface_device", C.c_int,
     [_VP, C.c_uint64, _VP, _VP, C.POINTER(RptSurfaceQuery), C.POINTER(RptSurfaceArrays), _VP]),
]
# ... and every symbol include/rpt_gpu_lightmap.h declares, optional in the same way (lightmap_supported())
LIGHTMAP_SYMBOLS = [
    ("rptgpu_bake_lightmap", C.c_int,
     [_VP, C.c_uint64, _PD, _PD, _PD, C.POINTER(RptLightmapQuery), C.POINTER(RptLightmapArrays)]),
    ("rptgpu_bake_lightmap_device", C.c_int,
     [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptLightmapQuery), C.POINTER(RptLightmapArrays), _VP]),
]
# ... and every symbol include/rpt_gpu_lightmap_filter.h declares, optional in the same way (lightmap_filter_supported())
LIGHTMAP_FILTER_SYMBOLS = [
    ("rptgpu_filter_lightmap", C.c_int, [_VP, C.POINTER(RptLightmapFilter), C.POINTER(RptLightmapFilterArrays)]),
    ("rptgpu_filter_lightmap_device", C.c_int, [_VP, C.POINTER(RptLightmapFilter), C.POINTER(RptLightmapFilterArrays), _VP]),
]
# ... and every symbol include/rpt_gpu_direct.h declares, optional in the same way (direct_supported())
DIRECT_SYMBOLS = [
    ("rptgpu_bake_direct", C.c_int, [_VP, C.c_uint64, _PD, _PD, C.POINTER(C.c_uint32), C.POINTER(RptDirectQuery), _PD]),
    ("rptgpu_bake_direct_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptDirectQuery), _VP, _VP]),
    ("rptgpu_bake_lightmap_direct", C.c_int, [_VP, C.c_uint64, _PD, _PD, _PD, C.POINTER(RptLightmapQuery), _PD]),
    ("rptgpu_bake_lightmap_direct_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, _VP, C.POINTER(RptLightmapQuery), _VP, _VP]),
]
# ... and every symbol include/rpt_gpu_lightmap_lookup.h declares, optional in the same way (lightmap_lookup_supported())
LIGHTMAP_LOOKUP_SYMBOLS = [
    ("rptgpu_lookup_lightmap", C.c_int, [_VP, C.c_uint64, _PD, _PD, C.c_uint32, C.POINTER(RptLightmapBinding),
                                         C.POINTER(RptLookupQuery), C.POINTER(RptLookupArrays)]),
    ("rptgpu_lookup_lightmap_device", C.c_int, [_VP, C.c_uint64, _VP, _VP, C.c_uint32, C.POINTER(RptLightmapBinding),
                                                C.POINTER(RptLookupQuery), C.POINTER(RptLookupArrays), _VP]),
    ("rptgpu_render_views_lightmapped", C.c_int, [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.c_uint32,
                                                  C.POINTER(RptLightmapBinding), C.POINTER(RptViewsLightmapQuery), _PD]),
    ("rptgpu_render_views_lightmapped_device", C.c_int, [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.c_uint32,
                                                         C.POINTER(RptLightmapBinding), C.POINTER(RptViewsLightmapQuery), _VP, _VP]),
]
# ... and every symbol include/rpt_gpu_probe_volume.h declares, optional in the same way (probe_volume_supported())
_VOLUME_ARGS = [C.POINTER(RptProbeVolume), C.POINTER(RptVolumeQuery), C.POINTER(RptVolumeArrays)]
_VIEWS_PROBE_LIT_ARGS = [_VP, C.c_uint64, C.POINTER(RptView), C.POINTER(RptViewQuery), C.c_uint32, C.POINTER(RptLightmapBinding),
                         C.POINTER(RptProbeVolume), C.POINTER(RptViewsProbeLitQuery)]
PROBE_VOLUME_SYMBOLS = [
    ("rptgpu_sample_probe_volume", C.c_int, [_VP, C.c_uint64, _PD, _PD] + _VOLUME_ARGS),
    ("rptgpu_sample_probe_volume_device", C.c_int, [_VP, C.c_uint64, _VP, _VP] + _VOLUME_ARGS + [_VP]),
    ("rptgpu_lookup_probe_volume", C.c_int, [_VP, C.c_uint64, _PD, _PD] + _VOLUME_ARGS),
    ("rptgpu_lookup_probe_volume_device", C.c_int, [_VP, C.c_uint64, _VP, _VP] + _VOLUME_ARGS + [_VP]),
    ("rptgpu_render_views_probe_lit", C.c_int, _VIEWS_PROBE_LIT_ARGS + [_PD]),
    ("rptgpu_render_views_probe_lit_device", C.c_int, _VIEWS_PROBE_LIT_ARGS + [_VP, _VP]),
]


class RptGpuError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        self.detail = detail
        super().__init__("rptgpu error %d: %s" % (code, detail))


_lib = None


def load_library(path=None):
    """Load librptgpu.so and bind every declared symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            "rpt_amd: %s not found — the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "There is no CPU fallback." % p)
    lib = C.CDLL(p)
    for name, restype, argtypes in SYMBOLS + SEEDED_SYMBOLS + DENOISED_SYMBOLS + VERTICES_SYMBOLS + VIEWS_PERSISTENT_SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    for name, restype, argtypes in RAYS_PERSISTENT_SYMBOLS + VERTICES_PERSISTENT_SYMBOLS + HIT_SURFACE_SYMBOLS + LIGHTMAP_SYMBOLS + LIGHTMAP_FILTER_SYMBOLS + DIRECT_SYMBOLS + LIGHTMAP_LOOKUP_SYMBOLS + PROBE_VOLUME_SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue  # (an older library, by path or RPTGPU_LIB: still ABI 7 — rays_ / vertices_persistent_supported(), hit_surface_supported(), lightmap_supported(), lightmap_filter_supported(), direct_supported(), lightmap_lookup_supported(), probe_volume_supported() say no)
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.rptgpu_abi_version() != ABI_VERSION:
        raise ImportError("rpt_amd: ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def views_persistent_supported(lib=None):
    """Does the library read RPT_FLAG_VIEWS_PERSISTENT (include/rpt_gpu_views_persistent.h)?  Detected by symbol, as a C
    caller does with dlsym: a library without it is still ABI 7, ignores the bit and runs the wavefront pipeline."""
    lib = lib or load_library()
    try:
        fn = lib.rptgpu_views_persistent_supported
    except AttributeError:
        return False
    fn.restype, fn.argtypes = C.c_int, []
    return fn() == 1


def rays_persistent_supported(lib=None):
    """Does the library read RPT_FLAG_RAYS_PERSISTENT (include/rpt_gpu_rays_persistent.h)?  Detected by symbol, as a C
    caller does with dlsym: a library without it is still ABI 7, ignores the bit and runs the wavefront pipeline."""
    lib = lib or load_library()
    try:
        fn = lib.rptgpu_rays_persistent_supported
    except AttributeError:
        return False
    fn.restype, fn.argtypes = C.c_int, []
    return fn() == 1


def vertices_persistent_supported(lib=None):
    """Does the library read RPT_FLAG_VERTICES_PERSISTENT (include/rpt_gpu_vertices_persistent.h)?  Detected by symbol, as a C
    caller does with dlsym: a library without it is still ABI 7, ignores the bit and runs the wavefront pipeline."""
    lib = lib or load_library()
    try:
        fn = lib.rptgpu_vertices_persistent_supported
    except AttributeError:
        return False
    fn.restype, fn.argtypes = C.c_int, []
    return fn() == 1


def hit_surface_supported(lib=None):
    """Does the library export rptgpu_hit_surface[_device] (include/rpt_gpu_hit_surface.h)?  Detected by symbol, as a C
    caller does with dlsym: a library without them is still ABI 7."""
    lib = lib or load_library()
    return all(hasattr(lib, name) for name, _, _ in HIT_SURFACE_SYMBOLS)


def lightmap_supported(lib=None):
    """Does the library export rptgpu_bake_lightmap[_device] (include/rpt_gpu_lightmap.h)?  Detected by symbol, as a C
    caller does with dlsym: a library without them is still ABI 7."""
    lib = lib or load_library()
    return all(hasattr(lib, name) for name, _, _ in LIGHTMAP_SYMBOLS)


def lightmap_filter_supported(lib=None):
    """Does the library export rptgpu_filter_lightmap[_device] (include/rpt_gpu_lightmap_filter.h)?  Detected by symbol, as
    a C caller does with dlsym: a library without them is still ABI 7."""
    lib = lib or load_library()
    return all(hasattr(lib, name) for name, _, _ in LIGHTMAP_FILTER_SYMBOLS)


def direct_supported(lib=None):
    """Does the library export rptgpu_bake_direct[_device] and rptgpu_bake_lightmap_direct[_device]
    (include/rpt_gpu_direct.h)?  Detected by symbol, as a C caller does with dlsym: a library without them is still ABI 7."""
    lib = lib or load_library()
    return all(hasattr(lib, name) for name, _, _ in DIRECT_SYMBOLS)


def probe_volume_supported(lib=None):
    """Does the library export rptgpu_sample_probe_volume and the other five symbols of include/rpt_gpu_probe_volume.h?
    Detected by symbol, as a C caller does with dlsym: a library without them is still ABI 7."""
    lib = lib or load_library()
    return all(hasattr(lib, name) for name, _, _ in PROBE_VOLUME_SYMBOLS)


def lightmap_lookup_supported(lib=None):
    """Does the library export rptgpu_lookup_lightmap[_device] (include/rpt_gpu_lightmap_lookup.h)?  Detected by symbol, as a
    C caller does with dlsym: a library without them is still ABI 7."""
    lib = lib or load_library()
    return all(hasattr(lib, name) for name, _, _ in LIGHTMAP_LOOKUP_SYMBOLS)


def check(code, handle=None):
    if code != RPTGPU_OK:
        lib = load_library()
        msg = lib.rptgpu_strerror(code).decode()
        det = lib.rptgpu_last_error_detail(handle)
        if det:
            msg += " — " + det.decode()
        raise RptGpuError(code, msg)
