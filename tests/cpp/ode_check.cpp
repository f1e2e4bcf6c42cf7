// ode_check.cpp — the independent checker of the particle systems: a line-by-line restatement of the reference's
// src/ode/particle_state.rs, src/ode/particle_system.rs and MonomialSurface::closest_point (monomial_surface.rs:126-181)
// on the host, written from the reference and NOT from the kernels (it includes nothing of rpt_amd/csrc).  Built by
// tests/ode_checker.py with -O2 -ffp-contract=off (and no FMA instruction set) as a shared library used through ctypes.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

namespace {

struct V3 {
  double x, y, z;
};
V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
V3 operator/(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
V3& operator+=(V3& a, V3 b) { return a = a + b; }
V3& operator-=(V3& a, V3 b) { return a = a - b; }
double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; } // nalgebra: x, then y, then z
double length(V3 a) { return std::sqrt(dot(a, a)); }
V3 normalize(V3 a) { return a / length(a); } // nalgebra normalize: self / self.norm()

// f64::powi: LLVM's llvm.powi, i.e. compiler-rt __powidf2 (square-and-multiply from the low bit, reciprocal last)
double powi(double a, int b) {
  const bool recip = b < 0;
  double r = 1;
  for (;;) {
    if (b & 1) r *= a;
    b /= 2;
    if (b == 0) break;
    a *= a;
  }
  return recip ? 1 / r : r;
}

// glibc 2.35 sysdeps/ieee754/dbl-64/e_hypot.c, the x86-64 build (no __FP_FAST_FMA)
double hypot_kernel(double ax, double ay) {
  double t1, t2;
  double h = std::sqrt(ax * ax + ay * ay);
  if (h <= 2.0 * ay) {
    double delta = h - ay;
    t1 = ax * (2.0 * delta - ax);
    t2 = (delta - 2.0 * (ax - ay)) * delta;
  } else {
    double delta = h - ax;
    t1 = 2.0 * delta * (ax - 2.0 * ay);
    t2 = (4.0 * delta - ay) * ay + delta * delta;
  }
  h -= (t1 + t2) / (2.0 * h);
  return h;
}
bool issignaling(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  b &= 0x7fffffffffffffffull;
  return b > 0x7ff0000000000000ull && !(b & 0x0008000000000000ull);
}
double glibc_hypot(double x, double y) {
  if (!std::isfinite(x) || !std::isfinite(y)) {
    if ((std::isinf(x) || std::isinf(y)) && !issignaling(x) && !issignaling(y)) return INFINITY;
    return x + y;
  }
  x = std::fabs(x);
  y = std::fabs(y);
  double ax = x < y ? y : x;
  double ay = x < y ? x : y;
  if (ax > 0x1p+511) {
    if (ay <= ax * 0x1p-54) return ax + ay;
    return hypot_kernel(ax * 0x1p-600, ay * 0x1p-600) / 0x1p-600;
  }
  if (ay < 0x1p-511) {
    if (ax >= ay / 0x1p-54) return ax + ay;
    return hypot_kernel(ax / 0x1p-600, ay / 0x1p-600) * 0x1p-600;
  }
  if (ay <= ax * 0x1p-54) return ax + ay;
  return hypot_kernel(ax, ay);
}

// MonomialSurface::closest_point (steps 100) / closest_point_precise (steps 10000), monomial_surface.rs:126-181
V3 closest_point(double height, V3 point, int steps) {
  if (length(point) < 1e-12) return point;
  double px = glibc_hypot(point.x, point.z);
  double py = point.y;
  double res0 = 1e18, res1 = -1.;
  for (int x = -steps; x < steps + 1; x++) {
    double xf = (double)x / (double)steps;
    double gy = height * powi(xf, 4);
    double dx = xf - px, dy = gy - py; // glm::distance2(&pt, &q) = (q - pt).norm_squared()
    double dist2 = dx * dx + dy * dy;
    if (dist2 < res0) {
      res0 = dist2;
      res1 = xf;
    }
  }
  double n = std::sqrt(point.x * point.x + point.z * point.z); // glm::normalize(&vec2(x, z))
  double nx = point.x / n, nz = point.z / n;
  double xzx = res1 * nx, xzy = res1 * nz;
  return {xzx, height * powi(powi(xzx, 2) + powi(xzy, 2), 2), xzy};
}

struct State {
  std::vector<V3> pos, vel;
};
State add(const State& a, const State& b) {
  State r{a.pos, a.vel};
  for (size_t i = 0; i < a.pos.size(); i++) {
    r.pos[i] = a.pos[i] + b.pos[i];
    r.vel[i] = a.vel[i] + b.vel[i];
  }
  return r;
}
State mul(const State& a, double s) {
  State r{a.pos, a.vel};
  for (size_t i = 0; i < a.pos.size(); i++) {
    r.pos[i] = a.pos[i] * s;
    r.vel[i] = a.vel[i] * s;
  }
  return r;
}

enum { GRAVITY = 0, MARBLES = 1, CIRCLE = 2 };

State time_derivative(int kind, double radius, const State& state) {
  size_t n = state.pos.size();
  if (kind == CIRCLE) { // particle_system.rs:29-39
    State r{state.pos, std::vector<V3>(n, V3{0.0, 0.0, 0.0})};
    for (size_t i = 0; i < n; i++) r.pos[i] = V3{-state.pos[i].y, state.pos[i].x, 0.0};
    return r;
  }
  if (kind == GRAVITY) { // :44-61
    std::vector<V3> acc(n, V3{0.0, 0.0, 0.0});
    for (size_t i = 0; i < n; i++)
      for (size_t j = 0; j < i; j++) {
        V3 dir = normalize(state.pos[i] - state.pos[j]);
        double len = length(state.pos[i] - state.pos[j]);
        V3 force = dir * (powi(len, -2) - 0.0001 * powi(len, -5));
        acc[j] += force;
        acc[i] -= force;
      }
    return {state.vel, acc};
  }
  // MarblesSystem, :72-126
  std::vector<V3> acc(n, V3{0.0, -1., 0.0});
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < i; j++) {
      V3 dir = normalize(state.pos[i] - state.pos[j]);
      double len = length(state.pos[i] - state.pos[j]);
      if (len < 2. * radius) {
        V3 force = -dir * 5. * powi((2. * radius - len) / radius, 1);
        acc[j] += force;
        acc[j] -= state.vel[j] * 0.5;
        acc[i] -= force;
        acc[i] -= state.vel[i] * 0.5;
      }
    }
  for (size_t i = 0; i < n; i++) {
    V3 closest = closest_point(2., state.pos[i], 100);
    V3 vec = state.pos[i] - closest;
    V3 normal = normalize(vec);
    double ratio_intersecting = (radius - length(vec)) / radius;
    double normal_vel = dot(state.vel[i], normal);
    if (-0.1 < ratio_intersecting && ratio_intersecting < 0.) acc[i] -= 30. * normal * powi(normal_vel, 3);
    else if (ratio_intersecting >= 0.) acc[i] += 100. * normal * powi(ratio_intersecting, 1);
  }
  for (size_t i = 0; i < n; i++) {
    V3 normal{0., 1., 0.};
    double ratio_intersecting = ((radius - 0.06) - state.pos[i].y) / radius;
    double normal_vel = dot(state.vel[i], normal);
    if (length(state.pos[i]) > 0.1) {
      if (-0.1 < ratio_intersecting && ratio_intersecting < 0.) acc[i] -= 20. * normal * normal_vel;
      else if (ratio_intersecting >= 0.) acc[i] += 300000. * normal * powi(ratio_intersecting, 1);
    }
  }
  for (size_t i = 0; i < n; i++) acc[i] -= state.vel[i] / 5.;
  return {state.vel, acc};
}

// ParticleSystem::rk4_integrate (:10-24); returns the number of integration steps taken
uint64_t rk4_integrate(int kind, double radius, State& state, double time, double step) {
  uint64_t count = 0;
  auto integrate_step = [&](double step) {
    State k1 = time_derivative(kind, radius, state);
    State k2 = time_derivative(kind, radius, add(state, mul(k1, step / 2.0)));
    State k3 = time_derivative(kind, radius, add(state, mul(k2, step / 2.0)));
    State k4 = time_derivative(kind, radius, add(state, mul(k3, step)));
    state = add(state, mul(add(add(add(k1, mul(k2, 2.0)), mul(k3, 2.0)), k4), step / 6.0));
    count++;
  };
  while (time > step) {
    integrate_step(step);
    time -= step;
  }
  integrate_step(time);
  return count;
}

State load(uint64_t n, const double* pos, const double* vel) {
  State s{std::vector<V3>(n), std::vector<V3>(n)};
  for (uint64_t i = 0; i < n; i++) {
    s.pos[i] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    s.vel[i] = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
  }
  return s;
}
void store(const std::vector<V3>& v, double* out) {
  for (size_t i = 0; i < v.size(); i++) {
    out[3 * i] = v[i].x;
    out[3 * i + 1] = v[i].y;
    out[3 * i + 2] = v[i].z;
  }
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

} // namespace

extern "C" {

double chk_hypot(double x, double y) { return glibc_hypot(x, y); }
double chk_std_hypot(double x, double y) { return std::hypot(x, y); }
void chk_hypot_array(uint64_t n, const double* x, const double* y, double* restated, double* libm) {
  for (uint64_t i = 0; i < n; i++) {
    restated[i] = glibc_hypot(x[i], y[i]);
    libm[i] = std::hypot(x[i], y[i]);
  }
}

// n random argument pairs from four families (uniform, raw bit patterns, near-equal, wide exponent spread); the
// number of pairs where the restatement's bits differ from std::hypot's (both NaN counts as equal)
uint64_t chk_hypot_sweep(uint64_t n, uint64_t seed) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> u(-4.0, 4.0);
  std::uniform_int_distribution<int> ex(-1074, 1023);
  uint64_t bad = 0;
  for (uint64_t i = 0; i < n; i++) {
    double x, y;
    switch (i & 3) {
      case 0: x = u(g); y = u(g); break;
      case 1: {
        uint64_t a = g(), b = g();
        std::memcpy(&x, &a, 8);
        std::memcpy(&y, &b, 8);
        break;
      }
      case 2: x = u(g); y = std::nextafter(x, (i & 4) ? INFINITY : -INFINITY) * ((i & 8) ? -1 : 1); break;
      default: x = std::ldexp(u(g), ex(g)); y = std::ldexp(u(g), ex(g)); break;
    }
    if (!same_bits(glibc_hypot(x, y), std::hypot(x, y))) bad++;
  }
  return bad;
}

void chk_closest_point(double height, int steps, uint64_t n, const double* pts, double* out) {
  unsigned nt = std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++)
    th.emplace_back([=] {
      for (uint64_t i = t; i < n; i += nt) {
        V3 r = closest_point(height, V3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, steps);
        out[3 * i] = r.x;
        out[3 * i + 1] = r.y;
        out[3 * i + 2] = r.z;
      }
    });
  for (auto& t : th) t.join();
}

void chk_time_derivative(int kind, double radius, uint64_t n, const double* pos, const double* vel, double* dpos,
                         double* dvel) {
  State d = time_derivative(kind, radius, load(n, pos, vel));
  store(d.pos, dpos);
  store(d.vel, dvel);
}

uint64_t chk_rk4_integrate(int kind, double radius, uint64_t n, double* pos, double* vel, double time, double step) {
  State s = load(n, pos, vel);
  uint64_t c = rk4_integrate(kind, radius, s, time, step);
  store(s.pos, pos);
  store(s.vel, vel);
  return c;
}

// the step sizes rk4_integrate takes for (time, step): writes up to `cap` of them, returns how many there are
uint64_t chk_schedule(double time, double step, double* out, uint64_t cap) {
  uint64_t c = 0;
  while (time > step) {
    if (c < cap) out[c] = step;
    c++;
    time -= step;
  }
  if (c < cap) out[c] = time;
  return c + 1;
}

} // extern "C"
