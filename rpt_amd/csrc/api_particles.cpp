// api_particles.cpp — the particle-system entry points of include/rpt_gpu.h (the reference's `rpt::ode`): argument
// checks on the host, one copy of the state to the device and one back, the kernels of particles.hip in between.
#include <cmath>

#include "api_internal.h"
#include "particles.h"

namespace {

using rptparticles::Sys;

constexpr uint32_t KNOWN_FLAGS = RPT_PARTICLES_FLAG_SINGLE_GROUP | RPT_PARTICLES_FLAG_GRID;
constexpr uint64_t DEFAULT_SINGLE_MAX = 256; // the single-workgroup schedule by default up to here

// RPTGPU_OK, or the code of what is wrong with the system and the size (the device is not looked at)
int check_system(const RptParticleSystem* sys, uint64_t n, bool& single) {
  if (!sys) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "sys is NULL");
  if (sys->kind > RPT_PARTICLES_CIRCLE) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "unknown particle system kind");
  if (sys->flags & ~KNOWN_FLAGS) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "unknown RPT_PARTICLES_FLAG_* bit");
  if (sys->flags == KNOWN_FLAGS)
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "both schedules forced (RPT_PARTICLES_FLAG_SINGLE_GROUP | _GRID)");
  if ((sys->flags & RPT_PARTICLES_FLAG_SINGLE_GROUP) && n > RPT_PARTICLES_SINGLE_MAX)
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "the single-workgroup schedule takes at most RPT_PARTICLES_SINGLE_MAX particles");
  if (n > RPT_PARTICLES_MAX_N)
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "more than RPT_PARTICLES_MAX_N particles (the kernels index 3n in 32 bits)");
  single = (sys->flags & RPT_PARTICLES_FLAG_SINGLE_GROUP) ||
           (!(sys->flags & RPT_PARTICLES_FLAG_GRID) && n <= DEFAULT_SINGLE_MAX);
  return RPTGPU_OK;
}

int check_device(int device) {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
    return fail(nullptr, RPTGPU_E_NO_DEVICE, "no HIP device is visible (hipGetDeviceCount); there is no CPU fallback");
  if (device < 0 || device >= nd) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "device index out of range");
  return RPTGPU_OK;
}

// rk4_integrate's schedule (particle_system.rs:19-23) with the reference's own f64 decrements: `full` steps of `step`,
// then one of `last`.  RPTGPU_E_INVALID_ARGUMENT if it never ends (time - step == time: the reference loops for ever)
// or has more than RPT_PARTICLES_MAX_STEPS steps.
struct Schedule {
  uint64_t full = 0;
  double last = 0.0;
};
int schedule_of(double time, double step, Schedule& out) {
  if (time > step && time / step > (double)RPT_PARTICLES_MAX_STEPS + 2.0)
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "time / step exceeds RPT_PARTICLES_MAX_STEPS");
  uint64_t full = 0;
  while (time > step) {
    double next = time - step;
    if (!(next < time) || full >= RPT_PARTICLES_MAX_STEPS)
      return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT,
                  "the step schedule does not end within RPT_PARTICLES_MAX_STEPS (time - step == time loops for ever)");
    time = next;
    full++;
  }
  out.full = full;
  out.last = time;
  return RPTGPU_OK;
}

// full steps per single-workgroup dispatch: about 2^22 pair evaluations per stage-chain, at least one step (a marbles
// frame, n = 25 and 625 steps, is one dispatch; n = 2048 is one step per dispatch)
uint64_t steps_per_dispatch(uint64_t n) { return std::max<uint64_t>(1, (1ull << 22) / (n * n)); }

// a stream of the call's own, destroyed on every way out
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

// [pos 3n | vel 3n] on the device from / to the caller's two arrays
void upload(DevBuf<double>& d, uint64_t n, const double* pos, const double* vel, hipStream_t st) {
  d.alloc(6 * n);
  HIP_TRY(hipMemcpyAsync(d.p, pos, 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.p + 3 * n, vel, 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
}
void download(const double* d, uint64_t n, double* pos, double* vel, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(pos, d, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(vel, d + 3 * n, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
}

} // namespace

extern "C" {

int rptgpu_particles_time_derivative(int device, const RptParticleSystem* sys, uint64_t n, const double* pos,
                                     const double* vel, double* out_dpos, double* out_dvel) {
  bool single = false;
  if (int e = check_system(sys, n, single)) return e;
  if (n == 0) return RPTGPU_OK;
  if (!pos || !vel || !out_dpos || !out_dvel) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "NULL array with n > 0");
  if (int e = check_device(device)) return e;
  return guarded(nullptr, device, [&]() -> int {
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DevBuf<double> state, out;
    upload(state, n, pos, vel, st.s);
    out.alloc(6 * n);
    Sys s{sys->kind, sys->radius};
    if (single) HIP_TRY(rptparticles::launch_single(s, (uint32_t)n, state.p, out.p, true, 0, 0.0, false, 0.0, st.s));
    else HIP_TRY(rptparticles::launch_derivative(s, (uint32_t)n, state.p, out.p, st.s));
    download(out.p, n, out_dpos, out_dvel, st.s);
    return RPTGPU_OK;
  });
}

int rptgpu_particles_integrate(int device, const RptParticleSystem* sys, uint64_t n, double* pos, double* vel,
                                   double time, double step) {
  bool single = false;
  if (int e = check_system(sys, n, single)) return e;
  if (!std::isfinite(time)) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "time is not finite");
  if (!std::isfinite(step) || !(step > 0.0))
    return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "step must be finite and > 0 (the reference loops for ever otherwise)");
  Schedule sched;
  if (int e = schedule_of(time, step, sched)) return e;
  if (n == 0) return RPTGPU_OK;
  if (!pos || !vel) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "NULL array with n > 0");
  if (int e = check_device(device)) return e;
  return guarded(nullptr, device, [&]() -> int {
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DevBuf<double> s, ks, a, b;
    upload(s, n, pos, vel, st.s);
    Sys d{sys->kind, sys->radius};
    if (single) {
      // the schedule in dispatches of at most steps_per_dispatch(n) steps; the final step goes with the last one
      const uint64_t chunk = steps_per_dispatch(n);
      uint64_t done = 0;
      do {
        const uint64_t m = std::min(chunk, sched.full - done);
        done += m;
        const bool final_dispatch = done == sched.full;
        HIP_TRY(rptparticles::launch_single(d, (uint32_t)n, s.p, nullptr, false, (uint32_t)m, step, final_dispatch,
                                            sched.last, st.s));
      } while (done < sched.full);
    } else {
      ks.alloc(6 * n);
      a.alloc(6 * n);
      b.alloc(6 * n);
      rptparticles::GridState g{s.p, ks.p, a.p, b.p};
      for (uint64_t i = 0; i < sched.full; i++) HIP_TRY(rptparticles::launch_rk4_step(d, (uint32_t)n, g, step, st.s));
      HIP_TRY(rptparticles::launch_rk4_step(d, (uint32_t)n, g, sched.last, st.s));
    }
    download(s.p, n, pos, vel, st.s);
    return RPTGPU_OK;
  });
}

int rptgpu_monomial_closest_point(int device, double height, uint32_t steps, uint64_t n, const double* points,
                                  double* out) {
  if (steps == 0 || steps > (1u << 24)) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "steps must be in 1..2^24");
  if (n > RPT_PARTICLES_MAX_N) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "more than RPT_PARTICLES_MAX_N points");
  if (n == 0) return RPTGPU_OK;
  if (!points || !out) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "NULL array with n > 0");
  if (int e = check_device(device)) return e;
  return guarded(nullptr, device, [&]() -> int {
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DevBuf<double> in, res;
    in.alloc(3 * n);
    res.alloc(3 * n);
    HIP_TRY(hipMemcpyAsync(in.p, points, 3 * n * sizeof(double), hipMemcpyHostToDevice, st.s));
    HIP_TRY(rptparticles::launch_closest_point(height, steps, n, in.p, res.p, st.s));
    HIP_TRY(hipMemcpyAsync(out, res.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    return RPTGPU_OK;
  });
}

int rptgpu_particles_eval_hypot(int device, uint64_t n, const double* x, const double* y, double* out) {
  if (n > RPT_PARTICLES_MAX_N) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "more than RPT_PARTICLES_MAX_N arguments");
  if (n == 0) return RPTGPU_OK;
  if (!x || !y || !out) return fail(nullptr, RPTGPU_E_INVALID_ARGUMENT, "NULL array with n > 0");
  if (int e = check_device(device)) return e;
  return guarded(nullptr, device, [&]() -> int {
    Stream st;
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    DevBuf<double> buf;
    buf.alloc(3 * n);
    HIP_TRY(hipMemcpyAsync(buf.p, x, n * sizeof(double), hipMemcpyHostToDevice, st.s));
    HIP_TRY(hipMemcpyAsync(buf.p + n, y, n * sizeof(double), hipMemcpyHostToDevice, st.s));
    HIP_TRY(rptparticles::launch_hypot(n, buf.p, buf.p + n, buf.p + 2 * n, st.s));
    HIP_TRY(hipMemcpyAsync(out, buf.p + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, st.s));
    HIP_TRY(hipStreamSynchronize(st.s));
    return RPTGPU_OK;
  });
}

} // extern "C"
