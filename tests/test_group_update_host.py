"""rptgpu_scene_set_group[_device] without a GPU: the library exports the two entry points and _abi binds them, a null
handle is refused with its detail, GpuScene.set_group checks shape, dtype and device before the library is called,
rpt_amd.transform_records is the lowering's RptTransform fields, include/rpt.hpp's Renderer::update_group compiles, and
the record header that scene creation and the update's kernels share (rpt_amd/csrc/shape_records.h) computes what
host_scene.cpp computed before it existed (tests/cpp/group_records_check.cpp, stand-alone, built like host_scene.o)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rpt_amd import GpuScene, KdTree, Object, Scene, _abi, cube, sphere, transform_records
from rpt_amd.scene import geometry_snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rptgpu_scene_set_group", "rptgpu_scene_set_group_device")


def test_library_exports_the_group_entry_points():
    lib = _abi.load_library()
    declared = {s[0]: s for s in _abi.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert declared[name][1] is _abi.C.c_int
    assert declared[NAMES[0]][2][1:] == [_abi.C.c_uint32, _abi.C.c_uint64, _abi.C.POINTER(_abi.RptShape)]
    assert declared[NAMES[1]][2][1:] == [_abi.C.c_uint32, _abi.C.c_uint64, _abi.C.c_void_p, _abi.C.c_void_p]
    header = open(os.path.join(ROOT, "include", "rpt_gpu.h")).read()
    rust = open(os.path.join(ROOT, "rust", "rpt-gpu-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert "int %s(" % name in header and "pub fn %s(" % name in rust
    assert _abi.C.sizeof(_abi.RptTransform) == 51 * 8  # the device entry's record


def test_library_refuses_a_null_handle():
    lib = _abi.load_library()
    kids = (_abi.RptShape * 1)()
    for name, args in ((NAMES[0], (None, 0, 1, kids)), (NAMES[1], (None, 0, 1, None, None))):
        assert getattr(lib, name)(*args) == _abi.RPTGPU_E_INVALID_ARGUMENT
        assert lib.rptgpu_last_error_detail(None) == (name + ": null handle").encode()


class _NoLibrary:
    """stands in for the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _children(n=4):
    return [(cube() if i % 2 else sphere()).scale((0.5, 0.25, 2.0)).rotate_y(0.3 * i).translate((float(i), 0.5, -1.0)) if i != 2 else sphere()
            for i in range(n)]


def _wrapper(device=0, lib=None):
    g = GpuScene.__new__(GpuScene)
    g.lib, g.handle, g.device = lib or _NoLibrary(), None, device
    s = Scene()
    s.add(Object(sphere()))
    s.add(Object(KdTree(_children()).translate((0.0, 1.0, 0.0))))
    g._geometry = geometry_snapshot(s)
    return g


@pytest.mark.parametrize("records, error, message", [
    (np.zeros((4, 51), dtype=np.float32), TypeError, "must be float64, not float32"),
    (np.zeros((4, 51), dtype=np.int64), TypeError, "must be float64"),
    (np.zeros((4, 50)), ValueError, "shape (n, 51), not (4, 50)"),
    (np.zeros(204), ValueError, "shape (n, 51), not (204,)"),
    (np.zeros((2, 2, 51)), ValueError, "shape (n, 51)"),
    (np.zeros((3, 51)), ValueError, "3 transform records for the 4 children of object 1"),
])
def test_wrapper_checks_numpy_input_before_the_library(records, error, message):
    with pytest.raises(error) as e:
        _wrapper().set_group(1, records)
    assert message in str(e.value)


def test_wrapper_checks_the_index_and_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    g = _wrapper()
    with pytest.raises(ValueError, match="negative"):
        g.set_group(-1, np.zeros((1, 51)))
    with pytest.raises(ValueError, match="object 0 is not a KdTree of shapes"):
        g.set_group(0, np.zeros((1, 51)))
    with pytest.raises(ValueError, match="object 7 is not a KdTree of shapes"):
        g.set_group(7, np.zeros((1, 51)))
    with pytest.raises(TypeError, match="must be float64, not torch.float32"):
        g.set_group(1, torch.zeros((4, 51), dtype=torch.float32))
    with pytest.raises(ValueError, match=r"shape \(n, 51\), not \(4, 18\)"):
        g.set_group(1, torch.zeros((4, 18), dtype=torch.float64))
    with pytest.raises(ValueError, match="the tensor is on cpu, the handle on device 0"):
        g.set_group(1, torch.zeros((4, 51), dtype=torch.float64))


def _fields(s):
    return np.concatenate([np.array(s.xf.transform[:]), np.array(s.xf.linear[:]), np.array(s.xf.inverse_transform[:]),
                           np.array(s.xf.normal_transform[:]), [s.xf.scale]])


def test_transform_records_are_the_fields_lower_writes():
    kids = _children(7)
    rec = transform_records(kids)
    assert rec.shape == (7, 51) and rec.dtype == np.float64
    for i, k in enumerate(kids):
        s = k.lower([])
        if s.transformed:
            assert rec[i].tobytes() == _fields(s).tobytes()
        else:
            assert i == 2 and not rec[i].any()
    assert transform_records([]).shape == (0, 51)


def test_wrapper_passes_shapes_and_records_on():
    calls = []

    class Lib:
        def rptgpu_scene_set_group(self, handle, index, n, arr):
            calls.append((index, n, [(arr[i].kind, arr[i].transformed, _fields(arr[i]).tobytes()) for i in range(n)]))
            return 0

    g = _wrapper(lib=Lib())
    kids = _children()
    later = [k.translate((0.0, 0.0, 0.5)) for k in kids]  # (child 2 becomes Transformed: a sequence of shapes is passed as it is)
    g.set_group(1, later)
    assert calls[-1][:2] == (1, 4) and [c[:2] for c in calls[-1][2]] == [(0, 1), (2, 1), (0, 1), (2, 1)]
    rec = transform_records(later)
    g.set_group(1, np.concatenate([rec, rec], axis=1)[:, :51])  # (a view: the wrapper makes it contiguous)
    index, n, passed = calls[-1]
    assert (index, n) == (1, 4)
    # kinds and `transformed` are the creation's; the records are the caller's (the library ignores child 2's)
    assert [c[:2] for c in passed] == [(0, 1), (2, 1), (0, 0), (2, 1)]
    for i in (0, 1, 3):
        assert passed[i][2] == rec[i].tobytes()


def test_cpp_renderer_update_group_compiles(tmp_path):
    """include/rpt.hpp's Renderer::update_group goes through the header's entry point"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = tmp_path / "update_group.cpp"
    src.write_text('#include "include/rpt.hpp"\n'
                   "int main() {\n"
                   "  rpt::Scene scene;\n"
                   "  scene.add(rpt::Object(rpt::sphere()));\n"
                   "  rpt::Renderer r(scene, rpt::Camera{});\n"
                   "  std::vector<rpt::Shape> children{rpt::sphere(), rpt::cube()};\n"
                   "  r.update_group(0, children);\n"
                   "  int (*f)(rptgpu_scene*, uint32_t, uint64_t, const RptShape*) = rptgpu_scene_set_group;\n"
                   "  int (*d)(rptgpu_scene*, uint32_t, uint64_t, const void*, void*) = rptgpu_scene_set_group_device;\n"
                   "  return f == nullptr || d == nullptr;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", ROOT, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc (%s): the record check is built with host_scene.o's compiler" % hipcc)
    return hipcc


def test_shared_records_equal_the_flatteners_expressions(tmp_path):
    """tests/cpp/group_records_check.cpp, compiled as rpt_amd/csrc/Makefile compiles host_scene.o: xf_point, the kinds' local
    boxes, Transformed::bounding_box and quadric_too_small over identity, singular, non-finite and 10^6 random matrices —
    bit for bit (its header says what a NaN from arithmetic is held to)"""
    exe = str(tmp_path / "group_records_check")
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "group_records_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 3 and all(l.endswith("equal") for l in lines), r.stdout + r.stderr


def test_host_flattener_and_kernels_use_the_shared_records():
    """one copy of each expression: host_scene.cpp and group_update.hip take them from shape_records.h, and the two update
    files share the spare-set storage"""
    csrc = os.path.join(ROOT, "rpt_amd", "csrc")
    host = open(os.path.join(csrc, "host_scene.cpp")).read()
    dev = open(os.path.join(csrc, "group_update.hip")).read()
    for name in ("transformed_box", "local_box", "quadric_too_small"):
        assert "rptrec::" + name in host and "rptrec::" + name in dev, name
    assert "std::sqrt(b)" not in host and "m[12 + k] * 1.0" not in host and "m[12 + k] * 1.0" not in dev
    assert "-ffp-contract=off -c group_update.hip" in open(os.path.join(csrc, "Makefile")).read()
    for name in ("api_mesh.cpp", "api_group.cpp"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "tree_splice.h"' in text and "void copy_around(" not in text and "std::swap(h->nodes" not in text
