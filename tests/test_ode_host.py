"""rpt::ode without a GPU: the independent checker (tests/cpp/ode_check.cpp) against the reference's own test and the
oracle, its glibc hypot against the host's, the Python ParticleState / ParticleSystem, and the C-ABI entry points'
argument checks (no device here: a valid call is RPTGPU_E_NO_DEVICE, never a host fallback)."""
import ctypes as C
import math

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi, scenes
from rpt_amd.ode import MarblesSystem, ParticleState, ParticleSystem, SimpleCircleSystem, SolidGravitySystem

import ode_checker as K


def test_checker_passes_the_references_rk4_works():
    # particle_system.rs:136-149: the circle returns after tau and reaches (-1, 0, 0) after pi, both within 1e-3
    for t, target in ((2 * math.pi, (1.0, 0.0, 0.0)), (math.pi, (-1.0, 0.0, 0.0))):
        pos, _, _ = K.rk4_integrate(K.CIRCLE, [[1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], t, 0.005)
        assert np.linalg.norm(pos[0] - np.array(target)) < 1e-3


def _closest_points(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.5, 1.5, (n, 3)) * np.array([1.0, 2.0, 1.0]) + np.array([0.0, 1.0, 0.0])
    k = n // 10
    pts[:k, 0] = 0.0   # on the y axis: the 2-vector normalises to NaN
    pts[:k, 2] = 0.0
    pts[k:2 * k] *= 1e-13  # inside the 1e-12 ball: returned unchanged
    pts[2 * k] = 0.0
    pts[2 * k + 1] = (-0.0, 0.0, -0.0)
    pts[2 * k + 2] = (0.0, 5.0, 0.0)
    pts[2 * k + 3] = (np.nan, 1.0, 0.0)
    pts[2 * k + 4] = (np.inf, 1.0, 0.0)
    pts[2 * k + 5] = (1e200, 1e200, 1e200)  # every distance overflows: best_x stays -1
    return pts


def test_checker_closest_point_is_the_oracles(oracle):
    pts = _closest_points(100_000, 1)
    got = K.closest_point(2.0, pts, 100)
    ref = np.array([oracle.monomial_closest_point(2.0, p, 100) for p in pts])
    assert K.mismatches(got, ref) == 0
    # closest_point_precise on a subset, other heights
    for h, steps in ((1.0, 10000), (2.0, 10000), (0.5, 7)):
        sub = pts[::97]
        got = K.closest_point(h, sub, steps)
        ref = np.array([oracle.monomial_closest_point(h, p, steps) for p in sub])
        assert K.mismatches(got, ref) == 0, (h, steps)


def test_restated_hypot_is_the_host_libms():
    lib = K.lib()
    assert lib.chk_hypot_sweep(10_000_000, 20261015) == 0
    tiny, big = 5e-324, 1.7976931348623157e308
    special = [0.0, -0.0, tiny, -tiny, 2.2250738585072014e-308, 1e-310, 1e-300, 2.0 ** -511, 2.0 ** -512, 2.0 ** 511,
               2.0 ** 512, 1e300, big, -big, 1.0, -1.0, 3.0, 4.0, 1.5, math.inf, -math.inf, math.nan, 0.1, 1e-17]
    snan = np.array([0x7FF0000000000001], dtype=np.uint64).view(np.float64)[0]
    special.append(float(snan))
    for x in special:
        for y in special:
            a, b = lib.chk_hypot(x, y), lib.chk_std_hypot(x, y)
            assert K.same_bits(a, b), (x, y, a, b)
    # equal arguments, and the glibc result that is NOT the correctly rounded one
    for x in np.random.default_rng(3).uniform(0, 10, 10000):
        assert K.same_bits(lib.chk_hypot(x, x), lib.chk_std_hypot(x, x))


def test_particle_state_operators():
    rng = np.random.default_rng(0)
    a = ParticleState(rng.normal(size=(7, 3)), rng.normal(size=(7, 3)))
    b = ParticleState(rng.normal(size=(7, 3)), rng.normal(size=(7, 3)))
    s = a + b
    assert K.same_bits(s.pos, a.pos + b.pos) and K.same_bits(s.vel, a.vel + b.vel)
    m = a * 0.1
    assert K.same_bits(m.pos, a.pos * 0.1) and K.same_bits(m.vel, a.vel * 0.1)
    d = a / 5.0
    assert K.same_bits(d.pos, a.pos / 5.0) and not K.same_bits(d.pos, a.pos * 0.2)  # a division
    assert a.pos.dtype == np.float64 and a.pos.shape == (7, 3) and len(a) == 7
    with pytest.raises(ValueError):
        ParticleState(np.zeros((2, 3)), np.zeros((3, 3)))
    src = np.zeros((2, 3))
    c = ParticleState(src, src)
    c.pos[0, 0] = 1.0
    assert src[0, 0] == 0.0  # the state owns its arrays


class PyCircle(ParticleSystem):
    """SimpleCircleSystem written as a user would: only time_derivative; rk4_integrate is the trait's default"""

    def time_derivative(self, state):
        p = state.pos
        return ParticleState(np.stack([-p[:, 1], p[:, 0], np.zeros(len(p))], axis=1), np.zeros_like(state.vel))


def test_python_system_uses_the_traits_rk4_on_the_host():
    for t in (2 * math.pi, math.pi, 0.3, 0.0):
        st = ParticleState([[1.0, 0.0, 0.0], [0.3, -0.7, 2.0]], np.zeros((2, 3)))
        PyCircle().rk4_integrate(st, t, 0.005)
        pos, vel, _ = K.rk4_integrate(K.CIRCLE, [[1.0, 0.0, 0.0], [0.3, -0.7, 2.0]], np.zeros((2, 3)), t, 0.005)
        assert K.same_bits(st.pos, pos) and K.same_bits(st.vel, vel), t


def test_step_schedule_of_a_marbles_frame():
    steps = K.schedule(1.0 / 16.0, 1.0 / 10000.0)
    assert len(steps) == 625
    assert (steps[:624] == 1e-4).all()
    assert steps[624] == 9.999999999924044e-05
    # the Python driver takes the same steps
    seen = []

    class Probe(ParticleSystem):
        def time_derivative(self, state):
            return ParticleState(np.zeros_like(state.pos), np.zeros_like(state.vel))

        def rk4_integrate(self, state, time, step):
            orig = self.time_derivative
            count = [0]

            def td(s):
                count[0] += 1
                return orig(s)
            self.time_derivative = td
            ParticleSystem.rk4_integrate(self, state, time, step)
            seen.append(count[0])
    Probe().rk4_integrate(ParticleState(np.zeros((1, 3)), np.zeros((1, 3))), 1.0 / 16.0, 1.0 / 10000.0)
    assert seen == [4 * 625]


def test_checker_marbles_frame_is_deterministic_and_moves():
    st = scenes.marbles_start()
    p1, v1, c = K.rk4_integrate(K.MARBLES, st.pos, st.vel, 1.0 / 16.0, 1e-4, radius=scenes.MARBLES_R)
    p2, v2, _ = K.rk4_integrate(K.MARBLES, st.pos, st.vel, 1.0 / 16.0, 1e-4, radius=scenes.MARBLES_R)
    assert c == 625 and K.same_bits(p1, p2) and K.same_bits(v1, v2)
    assert np.isfinite(p1).all() and p1[:, 1].mean() < st.pos[:, 1].mean()  # falling (and touching: 0.2 apart, 2R = 0.3)


def _sys(kind, flags=0, radius=0.15):
    return _abi.RptParticleSystem(kind, flags, radius)


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entry_points_check_arguments_and_need_a_device():
    lib = _abi.load_library()
    n = 4
    pos, vel, out1, out2 = (np.zeros((n, 3)) for _ in range(4))
    ok = _sys(_abi.RPT_PARTICLES_MARBLES)
    E, ND, OK = _abi.RPTGPU_E_INVALID_ARGUMENT, _abi.RPTGPU_E_NO_DEVICE, _abi.RPTGPU_OK

    def deriv(sys, n=n, p=pos, v=vel, a=out1, b=out2):
        return lib.rptgpu_particles_time_derivative(0, C.byref(sys) if sys is not None else None, n,
                                                    _pd(p) if p is not None else None, _pd(v) if v is not None else None,
                                                    _pd(a) if a is not None else None, _pd(b) if b is not None else None)

    def integ(sys, time=1.0, step=0.1, n=n, p=pos, v=vel):
        return lib.rptgpu_particles_integrate(0, C.byref(sys) if sys is not None else None, n,
                                              _pd(p) if p is not None else None, _pd(v) if v is not None else None,
                                              time, step)
    # bad arguments are refused before the device is looked for
    assert deriv(None) == E and integ(None) == E
    assert deriv(_sys(3)) == E and integ(_sys(7)) == E
    assert deriv(_sys(0, 4)) == E and integ(_sys(0, 3)) == E
    assert integ(_sys(0, _abi.RPT_PARTICLES_FLAG_SINGLE_GROUP), n=_abi.RPT_PARTICLES_SINGLE_MAX + 1) == E
    for name in ("p", "v", "a", "b"):
        assert deriv(ok, **{name: None}) == E, name
    assert integ(ok, p=None) == E and integ(ok, v=None) == E
    for step in (0.0, -1e-4, math.inf, math.nan):
        assert integ(ok, step=step) == E, step
        assert integ(ok, step=step, n=0, p=None, v=None) == E
    for t in (math.inf, -math.inf, math.nan):
        assert integ(ok, time=t) == E
    # schedules that never end (time - step == time: the reference loops for ever) or run past RPT_PARTICLES_MAX_STEPS
    for t, step in ((1.0, 1e-17), (1e300, 1.0), (1e16, 1.0), (float(_abi.RPT_PARTICLES_MAX_STEPS) + 8.0, 1.0)):
        assert integ(ok, time=t, step=step) == E, (t, step)
        assert integ(ok, time=t, step=step, n=0, p=None, v=None) == E
    assert b"RPT_PARTICLES_MAX_STEPS" in lib.rptgpu_last_error_detail(None)
    assert integ(ok, time=float(_abi.RPT_PARTICLES_MAX_STEPS) - 8.0, step=1.0) == ND  # a long schedule that ends is fine
    assert integ(ok, time=1.0, step=1e-17, n=0, p=None, v=None) == E
    # more particles than the kernels index: refused before anything is read
    big = _abi.RPT_PARTICLES_MAX_N + 1
    assert deriv(ok, n=big) == E and integ(ok, n=big) == E
    assert lib.rptgpu_monomial_closest_point(0, 2.0, 100, big, _pd(out1), _pd(out2)) == E
    # n == 0 is nothing to do
    assert deriv(ok, n=0, p=None, v=None, a=None, b=None) == OK
    assert integ(ok, n=0, p=None, v=None) == OK
    # good arguments: no device, no fallback
    for kind in (_abi.RPT_PARTICLES_SOLID_GRAVITY, _abi.RPT_PARTICLES_MARBLES, _abi.RPT_PARTICLES_CIRCLE):
        for flags in (0, _abi.RPT_PARTICLES_FLAG_SINGLE_GROUP, _abi.RPT_PARTICLES_FLAG_GRID):
            assert deriv(_sys(kind, flags)) == ND
            assert integ(_sys(kind, flags)) == ND
            assert integ(_sys(kind, flags), time=-1.0) == ND  # a negative time is one step of that size
    pts = np.zeros((3, 3))
    assert lib.rptgpu_monomial_closest_point(0, 2.0, 100, 3, _pd(pts), None) == E
    assert lib.rptgpu_monomial_closest_point(0, 2.0, 0, 3, _pd(pts), _pd(out1)) == E
    assert lib.rptgpu_monomial_closest_point(0, 2.0, 100, 0, None, None) == OK
    assert lib.rptgpu_monomial_closest_point(0, 2.0, 100, 3, _pd(pts), _pd(out1)) == ND
    x = np.zeros(3)
    assert lib.rptgpu_particles_eval_hypot(0, 3, _pd(x), None, _pd(x)) == E
    assert lib.rptgpu_particles_eval_hypot(0, 0, None, None, None) == OK
    assert lib.rptgpu_particles_eval_hypot(0, 3, _pd(x), _pd(x), _pd(x)) == ND
    assert pos.sum() == 0 and vel.sum() == 0  # nothing was written


def test_python_systems_refuse_a_schedule_that_never_ends():
    st = ParticleState(np.zeros((2, 3)), np.zeros((2, 3)))
    for system in (SolidGravitySystem(), MarblesSystem(0.15), SimpleCircleSystem()):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            system.rk4_integrate(st, 1.0, 1e-17)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT


def test_marbles_push_out_is_the_oracles_closest_point_precise(oracle):
    # the push-out's x.hypot(z) is libm's, as in the reference (Python's math.hypot is not)
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1.2, 1.2, (400, 3)) + np.array([0.0, 0.8, 0.0])
    pts[0], pts[1], pts[2], pts[3] = (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1e200, 1e200, 1e200), (1e-13, 0.0, 0.0)
    for p in pts:
        got = np.array(scenes.marbles_closest_point_precise(p))
        assert K.same_bits(got, oracle.monomial_closest_point(2.0, p, 10000)), p
    x = rng.uniform(-1.5, 1.5, 200_000)
    z = rng.uniform(-1.5, 1.5, 200_000)
    _, libm = K.hypot(x, z)
    assert K.same_bits(np.array([scenes._libm_hypot(a, b) for a, b in zip(x[:20000], z[:20000])]), libm[:20000])


def test_python_systems_raise_without_a_device():
    st = ParticleState(np.zeros((2, 3)), np.zeros((2, 3)))
    for system in (SolidGravitySystem(), MarblesSystem(0.15), SimpleCircleSystem()):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            system.rk4_integrate(st, 0.1, 0.01)
        assert e.value.code == _abi.RPTGPU_E_NO_DEVICE
        with pytest.raises(rpt_amd.RptGpuError) as e:
            system.time_derivative(st)
        assert e.value.code == _abi.RPTGPU_E_NO_DEVICE
    with pytest.raises(ValueError):
        SolidGravitySystem(schedule="fast").time_derivative(st)
    assert rpt_amd.ParticleState is ParticleState and rpt_amd.MarblesSystem is MarblesSystem


def test_marbles_scene_is_the_examples():
    st = scenes.marbles_start()
    assert st.pos.shape == (25, 3) and (st.pos[:, 1] >= 4.0).all() and (st.pos[:, 1] < 6.0).all()
    assert st.pos[7, 0] == 1 / 5 - 0.375 and st.pos[7, 2] == 2 / 5 - 0.375
    moved = st.clone()
    moved.pos[0] = (0.0, 0.05, 0.3)   # in the glass's wall: pushed out along the surface normal
    moved.pos[1] = (3.0, -1.0, 0.0)   # under the table: clamped to it
    scene, cam, cfg = scenes.marbles(moved, hdri_size=(16, 8), test=True)
    assert cfg == dict(width=200, height=150, max_bounces=7, num_samples=1)
    assert len(scene.objects) == 1 + 25 + 1
