"""`Scene` / `SceneAdd` (reference src/scene.rs:7-41): two lists and an environment."""
import numpy as np

from . import _abi
from .environment import Environment
from .light import Light
from .object import Object
from .shape import Cube, KdTree, MonomialSurface, Plane, Sphere, Transformed


class Scene:
    def __init__(self):  # Scene::new, scene.rs:20-23
        self.objects = []
        self.lights = []
        self.environment = Environment()

    def add(self, node):  # SceneAdd<Object> / SceneAdd<Light>, scene.rs:31-41
        if isinstance(node, Object):
            self.objects.append(node)
        elif isinstance(node, Light):
            self.lights.append(node)
        else:
            raise TypeError("Scene.add takes an Object or a Light")

    def lower(self):
        """-> (RptScene, keepalive list)"""
        keep = []
        s = _abi.RptScene()
        objs = (_abi.RptObject * max(1, len(self.objects)))()
        for i, o in enumerate(self.objects):
            o.lower_into(objs[i], keep)
        lights = (_abi.RptLight * max(1, len(self.lights)))()
        for i, l in enumerate(self.lights):
            l.lower_into(lights[i], keep)
        keep += [objs, lights]
        s.objects, s.num_objects = objs, len(self.objects)
        s.lights, s.num_lights = lights, len(self.lights)
        self.environment.lower_into(s.environment, keep)
        return s, keep


# ---- what a live scene handle keeps (GpuScene.update, rptgpu_scene_set_objects / _lights): everything but the top-level
# placements and the materials.  The comparison is pure Python so that it can be checked without a GPU.
def _same(a, b):
    """bit-for-bit the same doubles (NaN equals NaN)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _shape_mismatch(a, b, where, top):
    """None when shape `b` has the geometry of `a`; else what differs.  `top`: a top-level object's or a light's shape,
    whose Transformed fields may change (only whether it is Transformed may not); inside a group a child's placement is
    geometry too."""
    if isinstance(a, Transformed) != isinstance(b, Transformed):
        return "%s: the shape is %sTransformed and was %sat creation" % (
            where, "" if isinstance(b, Transformed) else "not ", "" if isinstance(a, Transformed) else "not ")
    if isinstance(a, Transformed):
        if not top and a is not b and not _same(a.transform_m, b.transform_m):
            return "%s: its placement inside the group differs" % where
        a, b = a.shape, b.shape
    if a is b:
        return None
    ka = "Mesh" if isinstance(a, KdTree) and a.triangles is not None else type(a).__name__
    kb = "Mesh" if isinstance(b, KdTree) and b.triangles is not None else type(b).__name__
    if ka != kb:
        return "%s: a %s became a %s" % (where, ka, kb)
    if isinstance(a, (Sphere, Cube)):
        return None
    if isinstance(a, Plane):
        if not (_same(a.normal, b.normal) and _same(a.value, b.value)):
            return "%s: the plane's normal or value differs" % where
        return None
    if isinstance(a, MonomialSurface):
        if not (_same(a.height, b.height) and _same(a.exp, b.exp)):
            return "%s: the monomial surface's height or exponent differs" % where
        return None
    if isinstance(a, KdTree):
        if a.triangles is not None:
            if a.triangles is not b.triangles and not _same(a.triangles, b.triangles):
                return "%s: the mesh's triangles differ (%d -> %d triangles)" % (where, len(a.triangles), len(b.triangles))
            return None
        if len(a.objects) != len(b.objects):
            return "%s: the group has %d children, was %d" % (where, len(b.objects), len(a.objects))
        for k, (ca, cb) in enumerate(zip(a.objects, b.objects)):
            why = _shape_mismatch(ca, cb, "%s, child %d" % (where, k), False)
            if why:
                return why
        return None
    return "%s: unknown shape %s" % (where, type(a).__name__)


def _environment_mismatch(a, b):
    if a is b:
        return None
    if not _same(a.color, b.color):
        return "the environment's colour differs"
    if (a.hdri is None) != (b.hdri is None):
        return "the environment is %s HDRI and was %s at creation" % ("an" if b.hdri is not None else "no",
                                                                       "one" if a.hdri is not None else "none")
    if a.hdri is not None and a.hdri is not b.hdri:
        ha, hb = a.hdri, b.hdri
        if (ha.width, ha.height) != (hb.width, hb.height) or (ha.buf is not hb.buf and not _same(ha.buf, hb.buf)):
            return "the environment's HDRI differs"
    return None


def geometry_mismatch(old, new):
    """None when Scene `new` differs from `old` only in what a live handle can update — the top-level objects'
    Transformed fields and materials, the lights' colours, vectors, placements and materials — else a message naming
    the first difference: the object or light counts, the environment, a shape's kind or geometry (compared by identity
    first, then by value: triangle arrays, group children recursively, plane and monomial parameters), a Transformed
    dropped or added, a light's kind."""
    if len(old.objects) != len(new.objects):
        return "the scene has %d objects, was %d" % (len(new.objects), len(old.objects))
    if len(old.lights) != len(new.lights):
        return "the scene has %d lights, was %d" % (len(new.lights), len(old.lights))
    why = _environment_mismatch(old.environment, new.environment)
    if why:
        return why
    for i, (a, b) in enumerate(zip(old.objects, new.objects)):
        why = _shape_mismatch(a.shape, b.shape, "object %d" % i, True)
        if why:
            return why
    for i, (a, b) in enumerate(zip(old.lights, new.lights)):
        if a.kind != b.kind:
            return "light %d: its kind %d differs from the kind at creation (%d)" % (i, b.kind, a.kind)
        if a.kind == _abi.RPT_LIGHT_OBJECT:
            why = _shape_mismatch(a.object.shape, b.object.shape, "light %d" % i, True)
            if why:
                return why
    return None


def geometry_snapshot(scene):
    """A Scene that keeps `scene`'s shapes, light kinds and environment as they are now (later changes of `scene`'s
    lists or of its Objects' `shape` attributes do not reach it) — what geometry_mismatch compares against."""
    snap = Scene()
    snap.objects = [Object(o.shape) for o in scene.objects]
    snap.lights = [Light(l.kind, obj=Object(l.object.shape) if l.object is not None else None) for l in scene.lights]
    snap.environment = Environment(scene.environment.color, scene.environment.hdri)
    return snap
