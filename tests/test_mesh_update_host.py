"""rptgpu_scene_set_mesh[_device] without a GPU: the library exports the two entry points and _abi binds them, a null
handle is refused with its detail, GpuScene.set_mesh checks shape, dtype and device before the library is called,
include/rpt.hpp's Renderer::update_mesh compiles, and the record header that scene creation and the update's kernels
share (rpt_amd/csrc/mesh_records.h) computes what host_scene.cpp computed before it existed
(tests/cpp/mesh_records_check.cpp, stand-alone, built like host_scene.o)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rpt_amd import GpuScene, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rptgpu_scene_set_mesh", "rptgpu_scene_set_mesh_device")


def test_library_exports_the_mesh_entry_points():
    lib = _abi.load_library()
    declared = {s[0]: s for s in _abi.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert declared[name][1] is _abi.C.c_int
    assert declared[NAMES[0]][2][1:] == [_abi.C.c_uint32, _abi.C.c_uint64, _abi.C.POINTER(_abi.RptTriangle)]
    assert len(declared[NAMES[1]][2]) == 5
    header = open(os.path.join(ROOT, "include", "rpt_gpu.h")).read()
    rust = open(os.path.join(ROOT, "rust", "rpt-gpu-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert "int %s(" % name in header and "pub fn %s(" % name in rust


def test_library_refuses_a_null_handle():
    lib = _abi.load_library()
    tris = np.zeros((1, 18))
    for name, args in ((NAMES[0], (None, 0, 1, tris.ctypes.data_as(_abi.C.POINTER(_abi.RptTriangle)))),
                       (NAMES[1], (None, 0, 1, None, None))):
        assert getattr(lib, name)(*args) == _abi.RPTGPU_E_INVALID_ARGUMENT
        assert lib.rptgpu_last_error_detail(None) == (name + ": null handle").encode()


class _NoLibrary:
    """stands in for the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _wrapper(device=0):
    g = GpuScene.__new__(GpuScene)
    g.lib, g.handle, g.device = _NoLibrary(), None, device
    return g


@pytest.mark.parametrize("triangles, error, message", [
    (np.zeros((4, 18), dtype=np.float32), TypeError, "must be float64, not float32"),
    (np.zeros((4, 18), dtype=np.int64), TypeError, "must be float64"),
    (np.zeros((4, 9)), ValueError, "shape (n, 18), not (4, 9)"),
    (np.zeros(72), ValueError, "shape (n, 18), not (72,)"),
    (np.zeros((2, 2, 18)), ValueError, "shape (n, 18)"),
    ([[0.0] * 17], ValueError, "shape (n, 18), not (1, 17)"),
])
def test_wrapper_checks_numpy_input_before_the_library(triangles, error, message):
    with pytest.raises(error) as e:
        _wrapper().set_mesh(0, triangles)
    assert message in str(e.value)


def test_wrapper_checks_the_index_and_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    g = _wrapper()
    with pytest.raises(ValueError, match="negative"):
        g.set_mesh(-1, np.zeros((1, 18)))
    with pytest.raises(TypeError, match="must be float64, not torch.float32"):
        g.set_mesh(0, torch.zeros((4, 18), dtype=torch.float32))
    with pytest.raises(ValueError, match=r"shape \(n, 18\), not \(4, 9\)"):
        g.set_mesh(0, torch.zeros((4, 9), dtype=torch.float64))
    with pytest.raises(ValueError, match="the tensor is on cpu, the handle on device 0"):
        g.set_mesh(0, torch.zeros((4, 18), dtype=torch.float64))


def test_wrapper_passes_good_numpy_input_on():
    calls = []

    class Lib:
        def rptgpu_scene_set_mesh(self, handle, index, n, ptr):
            calls.append((index, n))
            return 0

    g = _wrapper()
    g.lib = Lib()
    g.set_mesh(3, np.zeros((5, 36))[:, ::2])  # (not contiguous: the wrapper makes it so)
    assert calls == [(3, 5)]


def test_cpp_renderer_update_mesh_compiles(tmp_path):
    """include/rpt.hpp's Renderer::update_mesh goes through the header's entry point"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = tmp_path / "update_mesh.cpp"
    src.write_text('#include "include/rpt.hpp"\n'
                   "int main() {\n"
                   "  rpt::Scene scene;\n"
                   "  scene.add(rpt::Object(rpt::sphere()));\n"
                   "  rpt::Renderer r(scene, rpt::Camera{});\n"
                   "  std::vector<RptTriangle> tris(2);\n"
                   "  r.update_mesh(0, tris);\n"
                   "  int (*f)(rptgpu_scene*, uint32_t, uint64_t, const void*, void*) = rptgpu_scene_set_mesh_device;\n"
                   "  return f == nullptr;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", ROOT, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc (%s): the record check is built with host_scene.o's compiler" % hipcc)
    return hipcc


def test_shared_records_equal_the_flatteners_expressions(tmp_path):
    """tests/cpp/mesh_records_check.cpp, compiled as rpt_amd/csrc/Makefile compiles host_scene.o: min / max and the bounds
    fold over +-0, NaN and infinities; fill_trix, the triangle box, grid_over, quantise_box and sliver over special,
    degenerate and 10^6 random triangles — bit for bit (its header says what a NaN from arithmetic is held to)"""
    exe = str(tmp_path / "mesh_records_check")
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "mesh_records_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 3 and all(l.endswith("equal") for l in lines), r.stdout + r.stderr


def test_host_flattener_uses_the_shared_records():
    """one copy of each expression: host_scene.cpp and mesh_update.hip take them from mesh_records.h"""
    csrc = os.path.join(ROOT, "rpt_amd", "csrc")
    host = open(os.path.join(csrc, "host_scene.cpp")).read()
    dev = open(os.path.join(csrc, "mesh_update.hip")).read()
    for name in ("fill_trix", "tri_box", "grid_over", "quantise_box", "sliver", "merge_box"):
        assert "rptrec::" + name in host, name
    for name in ("fill_trix", "tri_box", "quantise_box", "sliver"):
        assert "rptrec::" + name in dev, name
    assert "std::fmin(std::fmin(" not in host and "/ 65529.0" not in host and "1e-10 * (" not in host
