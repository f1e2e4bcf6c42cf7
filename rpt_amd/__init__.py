"""rpt_amd — the MI355X-native back-end for rpt's hot path, behind rpt's own builder API.

`from rpt_amd import *` gives the names a user of the reference crate has after
`use rpt::*` (reference src/lib.rs:9-21) for everything on the path:
Scene, Object, Light, Material, Camera, Renderer, Buffer, Filter, Environment, Hdri,
sphere, plane, cube, polygon, Mesh, KdTree, Triangle, Transformed, hex_color, color_bytes,
and rpt::ode's ParticleState, ParticleSystem, SolidGravitySystem, MarblesSystem.
The path tracer and the particle systems are HIP (rpt_amd/csrc) behind the C ABI in include/rpt_gpu.h.
Beyond the reference: GpuScene.trace_rays runs the path estimator along rays of the caller's own making (numpy arrays,
or torch tensors on the device), and GpuScene.bake_probes turns positions into light probes on the device — SH9 radiance or
surface irradiance — which sh9_basis / sh9_irradiance (numpy) evaluate; GpuScene.render_views renders a batch of frames in one
call, each from a View: a camera under a perspective, orthographic or panoramic projection (a panorama is an Hdri's texels);
GpuScene.occluded answers "is anything between here and there?" for the caller's rays with the shadow rays' own query, and
GpuScene.bake_ao bakes ambient occlusion (and bent normals) from directions drawn on the device; GpuScene.trace_vertices gives
the vertices of the paths trace_rays runs — where each bounced, what it picked up there and with what it went on;
GpuScene.hit_surface names the triangle, the barycentrics and the group's child behind a ray's first hit, and
surface.interpolate carries a per-vertex attribute there; GpuScene.bake_lightmap rasterises a mesh's UV charts into a map and
gathers irradiance and ambient occlusion at the covered texels, gutters filled (lightmap.load_obj_texcoords reads the uvs).
"""
from . import glm  # noqa: F401
from ._abi import RptGpuError  # noqa: F401
from ._abi import (RPT_AOV_ALBEDO, RPT_AOV_ALL, RPT_AOV_DEPTH, RPT_AOV_NORMAL, RPT_AOV_OBJECT,  # noqa: F401
                   RPT_AOV_POSITION, RPT_HIT_ALBEDO, RPT_HIT_ALL, RPT_HIT_NORMAL, RPT_HIT_OBJECT, RPT_HIT_POSITION, RPT_HIT_T,
                   RPT_PROBE_IRRADIANCE, RPT_PROBE_SH9, RPT_VIEW_ORTHOGRAPHIC, RPT_VIEW_PANORAMA,
                   RPT_VIEW_PERSPECTIVE)
from ._abi import (RPT_VERTEX_ABS_COS, RPT_VERTEX_ALL, RPT_VERTEX_BSDF, RPT_VERTEX_DIRECTION, RPT_VERTEX_DRAW,  # noqa: F401
                   RPT_VERTEX_INV_PDF, RPT_VERTEX_LENGTH, RPT_VERTEX_NORMAL, RPT_VERTEX_OBJECT, RPT_VERTEX_POSITION,
                   RPT_VERTEX_RADIANCE, RPT_VERTEX_RGB, RPT_VERTEX_T)
from ._abi import (RPT_SURFACE_ALL, RPT_SURFACE_BARYCENTRIC, RPT_SURFACE_CHILD, RPT_SURFACE_OBJECT,  # noqa: F401
                   RPT_SURFACE_PRIMITIVE, RPT_SURFACE_T)
from ._abi import (RPT_VOLUME_ALL, RPT_VOLUME_COVERED, RPT_VOLUME_INSIDE, RPT_VOLUME_NORMAL, RPT_VOLUME_OBJECT,  # noqa: F401
                   RPT_VOLUME_POINT, RPT_VOLUME_POSITION, RPT_VOLUME_T, RPT_VOLUME_VALUE)
from ._abi import (RPT_LOOKUP_ALL, RPT_LOOKUP_BILINEAR, RPT_LOOKUP_BINDING, RPT_LOOKUP_COVERED, RPT_LOOKUP_NEAREST,  # noqa: F401
                   RPT_LOOKUP_OBJECT, RPT_LOOKUP_T, RPT_LOOKUP_UV, RPT_LOOKUP_VALUE)
from ._abi import (RPT_LIGHTMAP_ALL, RPT_LIGHTMAP_AO, RPT_LIGHTMAP_BARYCENTRIC, RPT_LIGHTMAP_IRRADIANCE,  # noqa: F401
                   RPT_LIGHTMAP_NORMAL, RPT_LIGHTMAP_OWNER, RPT_LIGHTMAP_POSITION)
from .buffer import Buffer, Filter  # noqa: F401
from .camera import Camera, View  # noqa: F401
from .color import color_bytes, hex_color  # noqa: F401
from .device import DeviceBuffer, GpuScene, PathVertices, device_count, make_params  # noqa: F401
from .environment import Environment, Hdri  # noqa: F401
from .io import load_mtl, load_obj, load_obj_with_mtl, load_stl  # noqa: F401
from .light import Light  # noqa: F401
from .material import Material  # noqa: F401
from .object import Object  # noqa: F401
from .ode import MarblesSystem, ParticleState, ParticleSystem, SolidGravitySystem  # noqa: F401
from .probes import ProbeVolume, sh9_basis, sh9_irradiance  # noqa: F401
from . import probes  # noqa: F401
from .renderer import Renderer  # noqa: F401
from .scene import Scene  # noqa: F401
from . import scenes  # noqa: F401
from . import surface  # noqa: F401
from . import lightmap  # noqa: F401
from .shape import (Cube, KdTree, Mesh, MonomialSurface, Plane, Shape, Sphere, Transformed, Triangle,  # noqa: F401
                    cube, monomial_surface, plane, polygon, sphere, transform_records)
