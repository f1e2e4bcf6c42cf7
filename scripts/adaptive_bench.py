"""Adaptive against uniform sampling on the device-resident Buffer: C2 (cornell, 1920x1080, 8 bounces)
and the C5 mesh (wine_glass, 3840x2160, 16 bounces), as rpt_amd/scenes.py and bench.py define them.

Per scene one JSON line: a uniform DeviceBuffer run of N batches of S samples and adaptive runs capped at N batches
(DeviceBuffer.sample_adaptive) for a few relative tolerances, each with its wall time per round (every call returns after
a device synchronise), the samples traced, the fraction of pixels active after each round and the RMSE of the linear
mean (totals / sample_counts) against a uniform reference of more samples rendered with another seed.
uniform_time_to_same_rmse_s: the wall time the uniform run needs to reach an adaptive run's final RMSE (linear between
its rounds; null if it does not within N batches).

    python scripts/adaptive_bench.py [--scene cornell|wine_glass] [--out profiles/adaptive_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rpt_amd  # noqa: E402
from rpt_amd import GpuScene, make_params, scenes  # noqa: E402

# scene: (samples per batch, batches, reference spp)
CONFIGS = {"cornell": (8, 16, 1024), "wine_glass": (4, 16, 256)}
REL_TOLS = (0.05, 0.01)
MIN_BATCHES = 4
SEED = 0x52505447


def rmse(dev, ref):
    """(linear, clamped to [0, 1]) RMSE of the buffer's per-pixel mean against the reference frame"""
    n = dev.sample_counts().reshape(-1, 1).astype(np.float64)
    mean = dev.totals().reshape(-1, 3) / n
    d = mean - ref
    dc = np.clip(mean, 0.0, 1.0) - np.clip(ref, 0.0, 1.0)
    return float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean(dc * dc)))


def run(g, cam, W, H, B, S, N, ref, rel_tol=None):
    """one buffer, uniform (rel_tol None) or adaptive: per round its wall time, the samples it traced, the active fraction
    afterwards and the RMSE"""
    dev = rpt_amd.DeviceBuffer(g, W, H)
    rounds, active = [], W * H
    for k in range(N):
        p = make_params(W, H, B, S, seed=SEED, sample_index_base=k * S)
        t0 = time.perf_counter()
        if rel_tol is None:
            dev.sample(cam, p)
            left = W * H
        else:
            left = dev.sample_adaptive(cam, p, MIN_BATCHES, 0.0, rel_tol)
        dt = time.perf_counter() - t0
        e, ec = rmse(dev, ref)  # (outside the timed call)
        rounds.append(dict(wall_s=dt, samples=active * S, active_after=left / (W * H), rmse=e, rmse_clamped=ec))
        active = left
        if not active:
            break
    dev.close()
    return rounds


def time_to(uniform, target):
    t, prev_t, prev_e = 0.0, 0.0, None
    for r in uniform:
        t += r["wall_s"]
        if r["rmse"] <= target:
            if prev_e is None or prev_e == r["rmse"]:
                return t
            return prev_t + (t - prev_t) * (prev_e - target) / (prev_e - r["rmse"])
        prev_t, prev_e = t, r["rmse"]
    return None


def summary(rounds):
    return dict(rounds=len(rounds), wall_s=round(sum(r["wall_s"] for r in rounds), 4),
                samples=sum(r["samples"] for r in rounds), rmse=rounds[-1]["rmse"],
                rmse_clamped=rounds[-1]["rmse_clamped"], active_fraction=[round(r["active_after"], 5) for r in rounds],
                rmse_per_round=[round(r["rmse"], 7) for r in rounds], wall_per_round=[round(r["wall_s"], 5) for r in rounds])


def bench(name):
    scene, cam, cfg = getattr(scenes, name)()
    W, H, B = cfg["width"], cfg["height"], cfg["max_bounces"]
    S, N, ref_spp = CONFIGS[name]
    g = GpuScene(scene, 0)
    g.render_batch(cam, make_params(W, H, B, S, seed=SEED))  # warm-up: code objects, workspace, learned pass sizes
    t0 = time.perf_counter()
    ref = g.render_batch(cam, make_params(W, H, B, ref_spp, seed=SEED + 1))  # independent of the runs' samples
    ref_s = time.perf_counter() - t0
    uniform = run(g, cam, W, H, B, S, N, ref)
    out = dict(scene=name, width=W, height=H, max_bounces=B, spp_per_batch=S, batches_cap=N, min_batches=MIN_BATCHES,
               reference=dict(spp=ref_spp, seed=SEED + 1, wall_s=round(ref_s, 3)), uniform=summary(uniform), adaptive=[])
    for rel in REL_TOLS:
        a = run(g, cam, W, H, B, S, N, ref, rel)
        s = dict(abs_tol=0.0, rel_tol=rel, **summary(a))
        tt = time_to(uniform, s["rmse"])
        s["uniform_time_to_same_rmse_s"] = None if tt is None else round(tt, 4)
        s["speedup_at_same_rmse"] = None if tt is None else round(tt / s["wall_s"], 3)
        out["adaptive"].append(s)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for name in [args.scene] if args.scene else ["cornell", "wine_glass"]:
        line = json.dumps(bench(name))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
