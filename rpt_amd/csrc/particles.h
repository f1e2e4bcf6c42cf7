// particles.h — the launchers of particles.hip (the reference's `rpt::ode` on the device) that api_particles.cpp calls.
// All pointers are device pointers; a state is n particles of 3 doubles (x, y, z) for pos and 3 for vel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rptparticles {

struct Sys {
  uint32_t kind; // RPT_PARTICLES_*
  double radius; // MarblesSystem::radius
};

// the single-workgroup schedule.  state and out are 6n doubles [pos 3n | vel 3n].  derivative_only: the derivative of
// state into out; otherwise, in place on state, nfull RK4 steps of `step` and then, if do_last, one of `last` (a
// share of rk4_integrate's schedule, which the caller splits into bounded dispatches).  n <= RPT_PARTICLES_SINGLE_MAX.
hipError_t launch_single(const Sys& sys, uint32_t n, double* state, double* out, bool derivative_only, uint32_t nfull,
                         double step, bool do_last, double last, hipStream_t st);

// the grid schedule.  Work arrays: s (the state: pos, vel), ks (the RK4 sum), a and b (stage states), 6n doubles
// each laid out as [pos 3n | vel 3n].
struct GridState {
  double *s, *ks, *a, *b;
};
// time_derivative of src (6n) into out (6n)
hipError_t launch_derivative(const Sys& sys, uint32_t n, const double* src, double* out, hipStream_t st);
// one RK4 step of size h on g.s: four launches, each a derivative with the stage update fused behind it
hipError_t launch_rk4_step(const Sys& sys, uint32_t n, const GridState& g, double h, hipStream_t st);

// MonomialSurface::closest_point for n points (3n doubles in, 3n out)
hipError_t launch_closest_point(double height, uint32_t steps, uint64_t n, const double* pts, double* out,
                                hipStream_t st);

// the device's restatement of glibc's hypot (the closest-point scan's px) for n argument pairs: diagnostics
hipError_t launch_hypot(uint64_t n, const double* x, const double* y, double* out, hipStream_t st);

} // namespace rptparticles
