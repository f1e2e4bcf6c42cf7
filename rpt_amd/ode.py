"""The reference's `rpt::ode` (src/ode.rs, src/ode/particle_state.rs, src/ode/particle_system.rs): particle states,
the ParticleSystem trait with its fixed-step RK4 driver, and the systems of the crate.

SolidGravitySystem and MarblesSystem (and SimpleCircleSystem, the reference's test system) run on the GPU through the
C ABI (include/rpt_gpu.h rptgpu_particles_*): their time_derivative and rk4_integrate are HIP kernels, bit-identical to
the reference's f64 arithmetic.  A ParticleSystem subclass written in Python that defines only
time_derivative gets the trait's default rk4_integrate, run on the host in numpy with the reference's schedule.
"""
import ctypes as C

import numpy as np

from . import _abi


def _vec3s(a):
    a = np.array(a, dtype=np.float64, order="C", copy=True)
    return a.reshape(-1, 3)


class ParticleState:
    """ParticleState { pos: Vec<DVec3>, vel: Vec<DVec3> } (particle_state.rs:4-10): two (N, 3) float64 arrays.
    `+` another state, `* f64` and `/ f64` act elementwise, which is what the Rust operators do (:16-58)."""

    def __init__(self, pos, vel):
        self.pos = _vec3s(pos)
        self.vel = _vec3s(vel)
        if self.pos.shape != self.vel.shape:
            raise ValueError("pos and vel must have the same number of particles")

    def __len__(self):
        return len(self.pos)

    def __add__(self, other):
        if not isinstance(other, ParticleState):
            return NotImplemented
        return ParticleState(self.pos + other.pos, self.vel + other.vel)

    def __mul__(self, s):
        if isinstance(s, ParticleState):
            return NotImplemented
        s = float(s)
        return ParticleState(self.pos * s, self.vel * s)

    def __truediv__(self, s):
        if isinstance(s, ParticleState):
            return NotImplemented
        s = float(s)
        return ParticleState(self.pos / s, self.vel / s)

    def clone(self):
        return ParticleState(self.pos, self.vel)

    def __repr__(self):
        return "ParticleState(n=%d)" % len(self)


class ParticleSystem:
    """The trait ParticleSystem (particle_system.rs:5-25).  Subclasses define time_derivative(state) -> ParticleState;
    rk4_integrate is the trait's default method, here on the host."""

    def time_derivative(self, state):
        raise NotImplementedError

    def rk4_integrate(self, state, time, step):
        """Integrate `state` in place for `time` with fixed steps of `step` (:10-24):
        `while time > step { step(step); time -= step; } step(time)`."""
        time, step = float(time), float(step)

        def integrate_step(h):
            k1 = self.time_derivative(state)
            k2 = self.time_derivative(state + k1 * (h / 2.0))
            k3 = self.time_derivative(state + k2 * (h / 2.0))
            k4 = self.time_derivative(state + k3 * h)
            new = state + (k1 + k2 * 2.0 + k3 * 2.0 + k4) * (h / 6.0)
            state.pos[...] = new.pos
            state.vel[...] = new.vel

        while time > step:
            integrate_step(step)
            time -= step
        integrate_step(time)


class _DeviceSystem(ParticleSystem):
    """A system of the closed device set: both methods run on HIP device `device` (no host fallback).
    `schedule`: None (by size), "single" (one workgroup, n <= RPT_PARTICLES_SINGLE_MAX) or "grid"."""
    KIND = None

    def __init__(self, radius=0.0, device=0, schedule=None):
        self.radius = float(radius)
        self.device = int(device)
        self.schedule = schedule

    def _desc(self):
        flags = {None: 0, "single": _abi.RPT_PARTICLES_FLAG_SINGLE_GROUP, "grid": _abi.RPT_PARTICLES_FLAG_GRID}
        if self.schedule not in flags:
            raise ValueError("schedule must be None, 'single' or 'grid'")
        return _abi.RptParticleSystem(self.KIND, flags[self.schedule], self.radius)

    def time_derivative(self, state):
        lib = _abi.load_library()
        pos, vel = _vec3s(state.pos), _vec3s(state.vel)
        dpos, dvel = np.empty_like(pos), np.empty_like(vel)
        desc = self._desc()
        _abi.check(lib.rptgpu_particles_time_derivative(self.device, C.byref(desc), len(pos), _ptr(pos), _ptr(vel),
                                                        _ptr(dpos), _ptr(dvel)))
        return ParticleState(dpos, dvel)

    def rk4_integrate(self, state, time, step):
        lib = _abi.load_library()
        pos, vel = _vec3s(state.pos), _vec3s(state.vel)
        desc = self._desc()
        _abi.check(lib.rptgpu_particles_integrate(self.device, C.byref(desc), len(pos), _ptr(pos), _ptr(vel),
                                                  float(time), float(step)))
        state.pos[...] = pos
        state.vel[...] = vel


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class SolidGravitySystem(_DeviceSystem):
    """SolidGravitySystem (particle_system.rs:42-62): O(N^2) gravity with a short-range 1e-4 / r^5 repulsion."""
    KIND = _abi.RPT_PARTICLES_SOLID_GRAVITY

    def __init__(self, device=0, schedule=None):
        super().__init__(0.0, device, schedule)


class MarblesSystem(_DeviceSystem):
    """MarblesSystem { radius } (particle_system.rs:64-127): marble contacts, the MonomialSurface { 2, 4 } glass, a
    table at y = -0.06 and drag."""
    KIND = _abi.RPT_PARTICLES_MARBLES

    def __init__(self, radius, device=0, schedule=None):
        super().__init__(radius, device, schedule)


class SimpleCircleSystem(_DeviceSystem):
    """SimpleCircleSystem (particle_system.rs:27-40), the system of the reference's own test rk4_works."""
    KIND = _abi.RPT_PARTICLES_CIRCLE

    def __init__(self, device=0, schedule=None):
        super().__init__(0.0, device, schedule)
