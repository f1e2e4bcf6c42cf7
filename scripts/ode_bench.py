"""Measures rpt::ode on the GPU and prints one JSON line (bench.py measures the renderer; this is its companion for
the particle systems):

  * a marbles frame (examples/marbles.rs: rk4_integrate(1/16, 1e-4) = 625 RK4 steps, N = 25) on device 0, next to
    the host checker (tests/cpp/ode_check.cpp, -O2 -ffp-contract=off, one core);
  * SolidGravitySystem at N = 4096, 16384, 65536 on the grid schedule: ms per RK4 step and pair evaluations per
    second (each of the 4 stages evaluates every ordered pair, N * (N - 1), as the one-thread-per-body kernel does:
    each distinct pair twice, once for each of its bodies); distinct_pairs_per_s counts N * (N - 1) / 2, the
    reference's loop.

Usage: python scripts/ode_bench.py [--frames F] [--sizes 4096,16384,65536] [--only marbles|gravity]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rpt_amd import scenes  # noqa: E402
from rpt_amd.ode import MarblesSystem, ParticleState, SolidGravitySystem  # noqa: E402


def marbles(frames):
    import ode_checker as K
    system = MarblesSystem(scenes.MARBLES_R)
    st = scenes.marbles_start()
    system.rk4_integrate(st, 1.0 / 16.0, 1e-4)  # warm-up: module load, first launch
    ts = []
    for _ in range(frames):
        t0 = time.perf_counter()
        system.rk4_integrate(st, 1.0 / 16.0, 1e-4)
        ts.append(time.perf_counter() - t0)
    pos, vel = scenes.marbles_start().pos, scenes.marbles_start().vel
    K.rk4_integrate(K.MARBLES, pos, vel, 1.0 / 16.0, 1e-4, scenes.MARBLES_R)
    hs = []
    for _ in range(max(3, frames // 4)):
        t0 = time.perf_counter()
        pos, vel, _ = K.rk4_integrate(K.MARBLES, pos, vel, 1.0 / 16.0, 1e-4, scenes.MARBLES_R)
        hs.append(time.perf_counter() - t0)
    return {"marbles_frame_ms_gpu": 1e3 * float(np.median(ts)), "marbles_frame_ms_host_checker_1core": 1e3 * float(np.median(hs)),
            "marbles_frames": frames}


def gravity(n, steps=4):
    rng = np.random.default_rng(n)
    pos = rng.uniform(-10.0, 10.0, (n, 3))
    vel = rng.normal(0.0, 0.1, (n, 3))
    system = SolidGravitySystem(schedule="grid")
    h = 1e-4

    def run(k):
        st = ParticleState(pos, vel)
        t0 = time.perf_counter()
        system.rk4_integrate(st, (k - 0.5) * h, h)  # k steps: k - 1 full ones and a last of h / 2
        return time.perf_counter() - t0
    run(1)
    one = min(run(1) for _ in range(2))
    many = min(run(1 + steps) for _ in range(2))
    ms = 1e3 * (many - one) / steps
    return {"n": n, "ms_per_rk4_step": ms, "pair_evals_per_s": 4.0 * n * (n - 1) / (ms * 1e-3),
            "distinct_pairs_per_s": 4.0 * n * (n - 1) / 2.0 / (ms * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--only", choices=["marbles", "gravity"])
    a = ap.parse_args()
    out = {"metric": "rpt_ode"}
    if a.only != "gravity":
        out.update(marbles(a.frames))
    if a.only != "marbles":
        out["gravity"] = [gravity(int(s)) for s in a.sizes.split(",")]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
