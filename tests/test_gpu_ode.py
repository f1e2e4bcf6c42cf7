"""rpt::ode on a real MI355X: the particle-system kernels (rpt_amd/csrc/particles.hip) against the independent host
checker (tests/cpp/ode_check.cpp, compiled here) and the oracle, BIT-EQUAL (a NaN equals any NaN), under both
schedules; and a marbles frame rendered from the device-integrated state against the oracle's render of the checker's."""
import ctypes as C
import math

import numpy as np
import pytest

import rpt_amd
from rpt_amd import GpuScene, _abi, make_params, scenes
from rpt_amd.ode import MarblesSystem, ParticleState, SimpleCircleSystem, SolidGravitySystem

import ode_checker as K

pytestmark = pytest.mark.gpu

R = scenes.MARBLES_R
SYSTEMS = {K.GRAVITY: SolidGravitySystem, K.MARBLES: MarblesSystem, K.CIRCLE: SimpleCircleSystem}


def device_closest(height, pts, steps):
    lib = _abi.load_library()
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.empty_like(pts)
    _abi.check(lib.rptgpu_monomial_closest_point(0, height, steps, len(pts), pts.ctypes.data_as(C.POINTER(C.c_double)),
                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def closest_inputs(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.3, 1.3, (n, 3)) * np.array([1.0, 2.0, 1.0]) + np.array([0.0, 1.0, 0.0])
    k = n // 20
    pts[:k, 0] = 0.0
    pts[:k, 2] = 0.0                       # on the y axis (NaN)
    pts[k:2 * k] *= 1e-13                  # inside the 1e-12 ball
    pts[2 * k:3 * k, 1] = 2.0 * (pts[2 * k:3 * k, 0] ** 2 + pts[2 * k:3 * k, 2] ** 2) ** 2  # on the surface
    pts[3 * k] = (0.0, 0.0, 0.0)
    pts[3 * k + 1] = (1e200, 1e200, 1e200)  # no grid point beats 1e18: best_x = -1
    pts[3 * k + 2] = (np.nan, 0.5, 0.1)
    pts[3 * k + 3] = (1e-310, 0.3, -1e-310)  # subnormal hypot
    return pts


def test_closest_point_is_the_oracles(oracle):
    pts = closest_inputs(1_000_000, 7)
    got = device_closest(2.0, pts, 100)
    ref = np.array([oracle.monomial_closest_point(2.0, p, 100) for p in pts])
    assert K.mismatches(got, ref) == 0
    # closest_point_precise: the full million against the checker (the oracle's restatement, proved equal to it on
    # the host by tests/test_ode_host.py), and 20 000 of them against the oracle itself
    got = device_closest(2.0, pts, 10000)
    assert K.mismatches(got, K.closest_point(2.0, pts, 10000)) == 0
    sub = pts[::50]
    assert K.mismatches(got[::50], np.array([oracle.monomial_closest_point(2.0, p, 10000) for p in sub])) == 0
    assert K.mismatches(device_closest(1.0, pts[:1000], 7), K.closest_point(1.0, pts[:1000], 7)) == 0


def hypot_arguments(n, seed):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-4.0, 4.0, n), rng.uniform(-4.0, 4.0, n)
    q = n // 4
    x[:q] = rng.integers(0, 2 ** 64, q, dtype=np.uint64).view(np.float64)  # raw bit patterns: every exponent, NaN, inf
    y[:q] = rng.integers(0, 2 ** 64, q, dtype=np.uint64).view(np.float64)
    y[q:2 * q] = np.nextafter(x[q:2 * q], np.inf) * np.where(np.arange(q) % 2, -1.0, 1.0)  # near-equal
    e = rng.integers(-1074, 1024, (2, q))
    x[2 * q:3 * q] = np.ldexp(rng.uniform(-1, 1, q), e[0])  # far-apart exponents (the 2^-600 / 2^600 scalings)
    y[2 * q:3 * q] = np.ldexp(rng.uniform(-1, 1, q), e[1])
    special = np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308, 2.0 ** -511, 2.0 ** -512, 2.0 ** 511, 2.0 ** 512,
                        1.7976931348623157e308, 1.0, 3.0, 4.0, np.inf, -np.inf, np.nan])
    sx, sy = np.meshgrid(special, special)
    return np.concatenate([x, sx.ravel()]), np.concatenate([y, sy.ravel()])


def test_device_hypot_is_the_host_libms():
    # the closest-point scan's x.hypot(z), evaluated directly: the device restatement of glibc's dbl-64 hypot against
    # the host's std::hypot and the checker's restatement, 10^7 argument pairs
    x, y = hypot_arguments(10_000_000, 31)
    lib = _abi.load_library()
    out = np.empty_like(x)
    P = C.POINTER(C.c_double)
    _abi.check(lib.rptgpu_particles_eval_hypot(0, len(x), x.ctypes.data_as(P), y.ctypes.data_as(P), out.ctypes.data_as(P)))
    restated, libm = K.hypot(x, y)
    assert K.mismatches(out, libm) == 0
    assert K.mismatches(out, restated) == 0
    # the arguments where glibc is not the correctly rounded result are among them: a sqrt(x*x + y*y) would not pass
    with np.errstate(over="ignore", invalid="ignore"):
        naive = np.sqrt(x * x + y * y)
    assert K.mismatches(naive, libm) > 0


def states(kind, n, seed):
    """random states with the traps: coincident particles, the origin, the y axis; marbles packed so that they touch,
    some in the glass's wall band and some on the table"""
    rng = np.random.default_rng(seed)
    if kind == K.MARBLES:
        side = max(1.0, (n * 0.03) ** (1 / 3))  # ~0.03 volume per marble: many contacts (2R = 0.3)
        pos = rng.uniform(-0.5, 0.5, (n, 3)) * side + np.array([0.0, 0.6, 0.0])
        vel = rng.normal(0.0, 0.5, (n, 3))
        if n >= 8:
            xz = rng.uniform(-0.8, 0.8, (n // 8, 2))
            r2 = (xz ** 2).sum(axis=1)
            pos[: n // 8, 0], pos[: n // 8, 2] = xz[:, 0], xz[:, 1]
            pos[: n // 8, 1] = 2.0 * r2 ** 2 + rng.uniform(-0.2, 0.2, n // 8)   # near the surface
            pos[n // 8: n // 4, 1] = rng.uniform(-0.1, 0.12, n // 4 - n // 8)  # on the table
    else:
        pos = rng.uniform(-2.0, 2.0, (n, 3))
        vel = rng.normal(0.0, 1.0, (n, 3))
    if n >= 2:
        pos[n - 1] = pos[0]                 # coincident pair: 0 / 0
    if n >= 3:
        pos[1] = (0.0, 0.0, 0.0)            # the origin
    if n >= 4:
        pos[2] = (0.0, pos[2, 1], 0.0)      # on the y axis
    return pos, vel


NS = [1, 2, 25, 48, 49, 63, 64, 65, 1024, 1025, 5000]


@pytest.mark.parametrize("kind", [K.GRAVITY, K.MARBLES, K.CIRCLE])
@pytest.mark.parametrize("n", NS)
def test_time_derivative_is_the_checkers(kind, n):
    pos, vel = states(kind, n, 100 + n)
    dp_ref, dv_ref = K.time_derivative(kind, pos, vel, R)
    st = ParticleState(pos, vel)
    schedules = [None, "grid"] + (["single"] if n <= _abi.RPT_PARTICLES_SINGLE_MAX else [])
    for sched in schedules:
        sys = SYSTEMS[kind](R, schedule=sched) if kind == K.MARBLES else SYSTEMS[kind](schedule=sched)
        d = sys.time_derivative(st)
        assert K.mismatches(d.pos, dp_ref) == 0, sched
        assert K.mismatches(d.vel, dv_ref) == 0, (sched, K.mismatches(d.vel, dv_ref))
    if kind != K.CIRCLE and n >= 2:
        assert np.isnan(dv_ref[0]).all()  # the coincident pair's NaN reached the reference's result too


def test_marbles_180_frames_of_the_example():
    start = scenes.marbles_start()
    gpu = start.clone()
    pos, vel = start.pos.copy(), start.vel.copy()
    system = MarblesSystem(R)
    for frame in range(180):
        system.rk4_integrate(gpu, 1.0 / 16.0, 1.0 / 10000.0)
        pos, vel, c = K.rk4_integrate(K.MARBLES, pos, vel, 1.0 / 16.0, 1.0 / 10000.0, R)
        assert c == 625
        assert K.mismatches(gpu.pos, pos) == 0 and K.mismatches(gpu.vel, vel) == 0, frame
    assert np.isfinite(pos).all()


def test_marbles_frame_on_the_grid_schedule():
    start = scenes.marbles_start()
    a, b = start.clone(), start.clone()
    MarblesSystem(R, schedule="grid").rk4_integrate(a, 1.0 / 16.0, 1.0 / 10000.0)
    MarblesSystem(R).rk4_integrate(b, 1.0 / 16.0, 1.0 / 10000.0)
    assert K.same_bits(a.pos, b.pos) and K.same_bits(a.vel, b.vel)


def test_gravity_2048_eight_steps_both_schedules():
    pos, vel = states(K.GRAVITY, 2048, 11)
    pos[-1] = pos[-2] + 1e-3  # no coincident pair: NaN would make the comparison trivial
    rpos, rvel, c = K.rk4_integrate(K.GRAVITY, pos, vel, 8e-4, 1e-4)
    out = {}
    for sched in ("single", "grid"):
        st = ParticleState(pos, vel)
        SolidGravitySystem(schedule=sched).rk4_integrate(st, 8e-4, 1e-4)
        out[sched] = st
        assert K.mismatches(st.pos, rpos) == 0 and K.mismatches(st.vel, rvel) == 0, sched
    assert K.same_bits(out["single"].pos, out["grid"].pos) and K.same_bits(out["single"].vel, out["grid"].vel)
    assert np.isfinite(rpos).all() and c in (8, 9)


def test_single_workgroup_schedule_split_over_dispatches():
    # n = 256 takes 64 steps per dispatch: 100 steps are two dispatches with the state carried through memory
    pos, vel = states(K.GRAVITY, 256, 23)
    pos[-1] = pos[-2] + 1e-2
    rpos, rvel, c = K.rk4_integrate(K.GRAVITY, pos, vel, 100.5e-4, 1e-4)
    assert c in (100, 101, 102)
    for sched in ("single", "grid"):
        st = ParticleState(pos, vel)
        SolidGravitySystem(schedule=sched).rk4_integrate(st, 100.5e-4, 1e-4)
        assert K.mismatches(st.pos, rpos) == 0 and K.mismatches(st.vel, rvel) == 0, sched


def test_schedules_that_never_end_are_refused_before_any_launch():
    st = ParticleState([[1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]])
    for sched in (None, "grid"):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            SimpleCircleSystem(schedule=sched).rk4_integrate(st, 1.0, 1e-17)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT
    assert st.pos[0, 0] == 1.0


@pytest.mark.parametrize("sched", [None, "grid"])
def test_circle_passes_rk4_works_on_the_device(sched):
    # particle_system.rs:136-149
    for t, target in ((2 * math.pi, (1.0, 0.0, 0.0)), (math.pi, (-1.0, 0.0, 0.0))):
        st = ParticleState([[1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]])
        SimpleCircleSystem(schedule=sched).rk4_integrate(st, t, 0.005)
        assert np.linalg.norm(st.pos[0] - np.array(target)) < 1e-3
        pos, vel, _ = K.rk4_integrate(K.CIRCLE, [[1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], t, 0.005)
        assert K.same_bits(st.pos, pos) and K.same_bits(st.vel, vel)


def test_marbles_frame_30_renders_like_the_oracle(oracle):
    start = scenes.marbles_start()
    gpu = start.clone()
    pos, vel = start.pos.copy(), start.vel.copy()
    for _ in range(30):
        MarblesSystem(R).rk4_integrate(gpu, 1.0 / 16.0, 1.0 / 10000.0)
        pos, vel, _ = K.rk4_integrate(K.MARBLES, pos, vel, 1.0 / 16.0, 1.0 / 10000.0, R)
    assert K.mismatches(gpu.pos, pos) == 0
    scene, cam, _ = scenes.marbles(gpu, hdri_size=(64, 32))
    ref_scene, _, _ = scenes.marbles(ParticleState(pos, vel), hdri_size=(64, 32))
    p = make_params(80, 60, 4, 2, seed=0x4D41)
    g = GpuScene(scene, 0)
    img = g.render_batch(cam, p)
    g.close()
    ref = oracle.OracleScene(ref_scene).render(cam, p, threads=0)
    assert np.isfinite(img).all() and img.max() > 0
    assert (img == ref).all()
