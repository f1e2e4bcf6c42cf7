"""`Camera` (reference src/camera.rs:8-62).  `cast_ray` (camera.rs:64-81) runs on the device
(ray-generation kernel)."""
import math

from . import _abi, glm


class Camera:
    def __init__(self, eye=(0.0, 0.0, 10.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0),
                 fov=math.pi / 6.0, aperture=0.0, focal_distance=0.0):  # Default camera.rs:28-39
        self.eye, self.direction, self.up = glm.vec3(*eye), glm.vec3(*direction), glm.vec3(*up)
        self.fov, self.aperture, self.focal_distance = float(fov), float(aperture), float(focal_distance)

    @staticmethod
    def look_at(eye, center, up, fov):  # camera.rs:43-54
        eye, center, up = glm.vec3(*eye), glm.vec3(*center), glm.vec3(*up)
        direction = glm.normalize(glm.sub(center, eye))
        up = glm.normalize(glm.sub(up, glm.scale(direction, glm.dot(up, direction))))
        return Camera(eye, direction, up, fov, 0.0, 0.0)

    def focus(self, focal_point, aperture):  # camera.rs:57-61
        self.focal_distance = glm.dot(glm.sub(glm.vec3(*focal_point), self.eye), self.direction)
        self.aperture = float(aperture)
        return self

    def lower(self):
        c = _abi.RptCamera()
        c.eye[:], c.direction[:], c.up[:] = self.eye, self.direction, self.up
        c.fov, c.aperture, c.focal_distance = self.fov, self.aperture, self.focal_distance
        return c


class View:
    """One view of GpuScene.render_views (include/rpt_gpu.h RptView): a camera under a projection — RPT_VIEW_PERSPECTIVE
    (the reference's camera, lens included), RPT_VIEW_ORTHOGRAPHIC (parallel rays along camera.direction; ortho_scale is
    the half-extent of the longer image side in world units) or RPT_VIEW_PANORAMA (360 degrees around camera.eye,
    world-aligned, in Hdri's texel convention)."""

    def __init__(self, camera, projection=_abi.RPT_VIEW_PERSPECTIVE, ortho_scale=0.0):
        self.camera, self.projection, self.ortho_scale = camera, int(projection), float(ortho_scale)

    @staticmethod
    def orthographic(camera, ortho_scale):
        return View(camera, _abi.RPT_VIEW_ORTHOGRAPHIC, ortho_scale)

    @staticmethod
    def panorama(eye):
        return View(Camera(eye=eye), _abi.RPT_VIEW_PANORAMA)

    def lower(self):
        v = _abi.RptView()
        v.camera = self.camera.lower() if hasattr(self.camera, "lower") else self.camera
        v.projection, v.ortho_scale = self.projection, self.ortho_scale
        return v
