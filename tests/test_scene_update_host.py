"""Live scene updates without a GPU: the library exports rptgpu_scene_set_objects / _lights and _abi binds them, and
GpuScene.update's geometry comparison (rpt_amd.scene.geometry_mismatch) accepts what a handle can update and names the
first thing it cannot."""
import numpy as np
import pytest

from rpt_amd import Environment, KdTree, Light, Material, Mesh, Object, Scene, _abi, cube, polygon, scenes, sphere
from rpt_amd.ode import ParticleState
from rpt_amd.scene import geometry_mismatch, geometry_snapshot

NAMES = ("rptgpu_scene_set_objects", "rptgpu_scene_set_lights")


def test_library_exports_the_update_entry_points():
    lib = _abi.load_library()
    declared = {s[0]: s for s in _abi.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        _, restype, argtypes = declared[name]
        assert restype is _abi.C.c_int and len(argtypes) == 4
    assert declared[NAMES[0]][2][3]._type_ is _abi.RptObject
    assert declared[NAMES[1]][2][3]._type_ is _abi.RptLight


def test_library_refuses_a_null_handle():
    lib = _abi.load_library()
    assert lib.rptgpu_scene_set_objects(None, 0, None, None) == _abi.RPTGPU_E_INVALID_ARGUMENT
    assert lib.rptgpu_scene_set_lights(None, 0, None, None) == _abi.RPTGPU_E_INVALID_ARGUMENT
    assert b"null handle" in lib.rptgpu_last_error_detail(None)


def test_same_geometry_is_accepted():
    for f in (1, 37, 59):
        assert geometry_mismatch(scenes.simple_video(0)[0], scenes.simple_video(f)[0]) is None
    # two marbles frames: the glass and the table are rebuilt per frame, equal by value
    a = scenes.marbles(scenes.marbles_start(), test=True)[0]
    st = scenes.marbles_start()
    st = ParticleState(st.pos + 0.25, st.vel)
    assert geometry_mismatch(a, scenes.marbles(st, test=True)[0]) is None
    # the same mesh moved and re-materialled, a light moved and recoloured
    m, _, _ = scenes.metal(hdri_size=(8, 4))
    mesh = m.objects[0].shape.shape
    n = Scene()
    n.environment = m.environment
    n.add(Object(mesh.rotate_y(1.0)).material(Material.diffuse((0.1, 0.2, 0.3))))
    n.add(Object(mesh.translate((1.0, 2.0, 3.0))))
    assert geometry_mismatch(m, n) is None
    s1, s2 = Scene(), Scene()
    s1.add(Light.Object(Object(sphere().translate((0.0, 3.0, 0.0))).material(Material.light((1.0, 1.0, 1.0), 5.0))))
    s2.add(Light.Object(Object(sphere().scale((2.0, 2.0, 2.0))).material(Material.light((0.0, 1.0, 0.0), 9.0))))
    s1.add(Light.Point((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
    s2.add(Light.Point((5.0, 1.0, 1.0), (3.0, 2.0, 1.0)))
    assert geometry_mismatch(s1, s2) is None


def one(shape, env=None):
    s = Scene()
    s.add(Object(shape))
    if env is not None:
        s.environment = env
    return s


TRIS = np.arange(2 * 18, dtype=np.float64).reshape(2, 18)


@pytest.mark.parametrize("old, new, message", [
    (lambda: scenes.simple_video(0)[0], lambda: (lambda s: (s.add(Object(sphere())), s)[1])(scenes.simple_video(0)[0]),
     "the scene has 6 objects, was 5"),
    (lambda: one(sphere()), lambda: one(sphere(), Environment.Color((0.1, 0.1, 0.1))), "environment's colour"),
    (lambda: one(sphere(), Environment.Hdri(scenes.synthetic_hdri(8, 4))),
     lambda: one(sphere(), Environment.Hdri(scenes.synthetic_hdri(8, 4, seed=1))), "HDRI differs"),
    (lambda: one(Mesh(TRIS).translate((1.0, 0.0, 0.0))),
     lambda: one(Mesh(np.where(np.arange(36).reshape(2, 18) == 20, 99.0, TRIS)).translate((1.0, 0.0, 0.0))),
     "object 0: the mesh's triangles differ"),
    (lambda: one(KdTree([sphere(), cube().translate((2.0, 0.0, 0.0))])),
     lambda: one(KdTree([sphere(), sphere().translate((2.0, 0.0, 0.0))])), "object 0, child 1: a Cube became a Sphere"),
    (lambda: one(KdTree([sphere(), cube().translate((2.0, 0.0, 0.0))])),
     lambda: one(KdTree([sphere(), cube().translate((3.0, 0.0, 0.0))])), "child 1: its placement inside the group"),
    (lambda: one(sphere().translate((1.0, 0.0, 0.0))), lambda: one(cube().translate((1.0, 0.0, 0.0))),
     "object 0: a Sphere became a Cube"),
    (lambda: one(sphere().translate((1.0, 0.0, 0.0))), lambda: one(sphere()),
     "object 0: the shape is not Transformed and was at creation"),
    (lambda: one(polygon([(0, 0, 0), (1, 0, 0), (1, 1, 0)])), lambda: one(KdTree([sphere()])), "a Mesh became a KdTree"),
])
def test_different_geometry_is_named(old, new, message):
    why = geometry_mismatch(old(), new())
    assert why is not None and message in why, why


def test_light_kind_and_count_are_named():
    a, b = Scene(), Scene()
    a.add(Light.Point((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))
    b.add(Light.Directional((1.0, 1.0, 1.0), (0.0, -1.0, 0.0)))
    assert "light 0: its kind" in geometry_mismatch(a, b)
    b.add(Light.Ambient((0.1, 0.1, 0.1)))
    assert "2 lights, was 1" in geometry_mismatch(a, b)


def test_snapshot_keeps_the_creations_shapes():
    s = scenes.simple_video(0)[0]
    snap = geometry_snapshot(s)
    s.objects[0].shape = cube()  # a change of the caller's scene after the snapshot does not reach it
    assert "a Sphere became a Cube" in geometry_mismatch(snap, s)


def test_cpp_renderer_update_scene_compiles(tmp_path):
    """include/rpt.hpp's Renderer::update_scene goes through the two entry points of the header"""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "update_scene.cpp"
    src.write_text('#include "include/rpt.hpp"\n'
                   "int main() {\n"
                   "  rpt::Scene scene;\n"
                   "  scene.add(rpt::Object(rpt::sphere()));\n"
                   "  rpt::Renderer r(scene, rpt::Camera{});\n"
                   "  scene.objects[0] = rpt::Object(rpt::sphere().translate({1.0, 0.0, 0.0}));\n"
                   "  r.update_scene();\n"
                   "  return 0;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", root, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
