"""Builds and binds tests/cpp/ode_check.cpp, the host checker of the particle systems (a restatement of the reference's
src/ode written independently of the kernels), compiled like tests/test_math_converged.py's checker: -O2
-ffp-contract=off, no FMA instruction set.  g++ where there is one, else ROCm's clang++ with the same flags."""
import ctypes as C
import os
import platform
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "ode_check.cpp")
GRAVITY, MARBLES, CIRCLE = 0, 1, 2

_lib = None


def compiler():
    for c in ("g++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c) or os.path.exists(c):
            return c
    raise RuntimeError("no C++ compiler (g++ or /opt/rocm/llvm/bin/clang++) for tests/cpp/ode_check.cpp")


def flags():
    f = ["-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-pthread"]
    if platform.machine() in ("x86_64", "AMD64"):
        f.append("-mno-fma")  # the default x86-64 target has none; say so in case a compiler's default differs
    return f


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ode_check_"), "libode_check.so")
        subprocess.run([compiler()] + flags() + ["-o", out, SRC], check=True)
        L = C.CDLL(out)
        D, PD, U64 = C.c_double, C.POINTER(C.c_double), C.c_uint64
        for name, res, args in (
                ("chk_hypot", D, [D, D]), ("chk_std_hypot", D, [D, D]), ("chk_hypot_sweep", U64, [U64, U64]),
                ("chk_hypot_array", None, [U64, PD, PD, PD, PD]),
                ("chk_closest_point", None, [D, C.c_int, U64, PD, PD]),
                ("chk_time_derivative", None, [C.c_int, D, U64, PD, PD, PD, PD]),
                ("chk_rk4_integrate", U64, [C.c_int, D, U64, PD, PD, D, D]),
                ("chk_schedule", U64, [D, D, PD, U64])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        L.path = out
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _arr(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def hypot(x, y):
    """-> (the checker's glibc restatement, the host libm's std::hypot) for the argument arrays"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    a, b = np.empty_like(x), np.empty_like(x)
    lib().chk_hypot_array(len(x), _p(x), _p(y), _p(a), _p(b))
    return a, b


def closest_point(height, points, steps=100):
    pts = _arr(points)
    out = np.empty_like(pts)
    lib().chk_closest_point(height, steps, len(pts), _p(pts), _p(out))
    return out


def time_derivative(kind, pos, vel, radius=0.0):
    pos, vel = _arr(pos), _arr(vel)
    dp, dv = np.empty_like(pos), np.empty_like(vel)
    lib().chk_time_derivative(kind, radius, len(pos), _p(pos), _p(vel), _p(dp), _p(dv))
    return dp, dv


def rk4_integrate(kind, pos, vel, time, step, radius=0.0):
    """-> (pos, vel, number of steps) after rk4_integrate(time, step) from (pos, vel) (the inputs are not changed)"""
    pos, vel = _arr(pos).copy(), _arr(vel).copy()
    c = lib().chk_rk4_integrate(kind, radius, len(pos), _p(pos), _p(vel), time, step)
    return pos, vel, c


def schedule(time, step, cap=1 << 20):
    out = np.empty(cap)
    c = lib().chk_schedule(time, step, _p(out), cap)
    return out[:min(c, cap)]


def same_bits(a, b):
    """bit-equal arrays, a NaN equal to any NaN (their payloads are not the arithmetic's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())


def mismatches(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return int(bad.sum())
