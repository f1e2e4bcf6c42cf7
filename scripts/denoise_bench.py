"""The device Buffer's feature-guided denoising filter (rptgpu_buffer_features / _denoise) on the two
configurations of DESIGN.md §10: C2 (cornell, 1920x1080, 8 bounces, 16 batches of 8 spp, reference 1024 spp) and C5
(wine_glass, 3840x2160, 16 bounces, 16 batches of 4 spp, reference 256 spp), as rpt_amd/scenes.py defines them.

Wall times (the default mode), per scene and per repeat (REPEATS repeats, each a fresh buffer, so the variants alternate):
  batches       the buffer's 16 synchronous rptgpu_buffer_sample calls, summed;
  features      rptgpu_buffer_features, 4 spp, all four channels, nothing to the host;
  aov_dn        rptgpu_render_aov with DEPTH | NORMAL at the same 4 spp (DESIGN.md §11's call: its copies to the host included);
  denoise3 / 5  rptgpu_buffer_denoise, 3 and 5 levels, linear output (its copy to the host included).
Quality: RMSE (values clamped at 4.0) against a uniform reference of another seed for the raw mean, the Box(1) mean and
the denoised frames, and `uniform_samples_to_same_rmse`: the samples per pixel a plain run needs to reach the denoised
frame's RMSE — measured by sampling on (up to UNIFORM_CAP batches); beyond the cap it is extrapolated by rmse ~ 1/sqrt(n)
from the last batch and marked so.

Kernel times: one run under the profiler, the program after `--`, no counters in that run,
    rocprofv3 --kernel-trace --stats -d DIR -o <scene> --output-format csv -- python scripts/denoise_bench.py --scene S --trace
(two batches of 1 spp, features, then denoise with 3 levels twice), then
    python scripts/denoise_bench.py --merge-stats DIR --out profiles/denoise_bench.json
adds the mean time per launch of each rpt_denoise_* kernel and, for rpt_denoise_level, the bytes a level MUST move by
its shapes (every input column once, 113 B, and its 32 B of output per pixel — not a measured traffic) over that time
as a share of the HBM peak.

    python scripts/denoise_bench.py [--scene cornell|wine_glass] [--out profiles/denoise_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpt_amd import DeviceBuffer, GpuScene, _abi, make_params, scenes  # noqa: E402

# scene: (max_bounces, samples per batch, batches, reference spp)
CONFIGS = {"cornell": (8, 8, 16, 1024), "wine_glass": (16, 4, 16, 256)}
SEED = 0x52505447
REPEATS = 3
FEATURE_SPP = 4
UNIFORM_CAP = 96  # batches
HBM_PEAK_GBS = 8000.0
LEVEL_BYTES_PER_PIXEL = (3 + 1 + 3 + 3 + 3 + 1) * 8 + 1 + 4 * 8


def stats(ts):
    return dict(wall_s=[round(t, 5) for t in ts], median_s=round(float(np.median(ts)), 5), spread_s=round(max(ts) - min(ts), 5))


def rmse(a, ref):
    return float(np.sqrt(np.mean((np.minimum(a, 4.0) - np.minimum(ref, 4.0)) ** 2)))


def box1(totals, counts):
    """the Box(1) mean of buffer.rs:75-93 in linear values (the order of the additions does not matter to an RMSE)"""
    h, w = counts.shape
    tp = np.zeros((h + 2, w + 2, 3))
    tp[1:-1, 1:-1] = totals
    cp = np.zeros((h + 2, w + 2))
    cp[1:-1, 1:-1] = counts
    num, den = np.zeros((h, w, 3)), np.zeros((h, w))
    for i in range(3):
        for j in range(3):
            num += tp[j:j + h, i:i + w]
            den += cp[j:j + h, i:i + w]
    return num / den[..., None]


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def bench(name):
    scene, camera, cfg = getattr(scenes, name)()
    W, H = cfg["width"], cfg["height"]
    B, S, N, ref_spp = CONFIGS[name]
    g = GpuScene(scene, 0)
    ref_s, ref = timed(lambda: g.render_batch(camera, make_params(W, H, B, ref_spp, seed=SEED + 1)).reshape(H, W, 3))
    pf = make_params(W, H, B, FEATURE_SPP, seed=SEED)
    dn = _abi.RPT_AOV_DEPTH | _abi.RPT_AOV_NORMAL
    g.render_aov(camera, pf, dn)  # warm-up: code objects, the handle's arrays
    times = {k: [] for k in ("batches", "features", "aov_dn", "denoise3", "denoise5")}
    quality = {}
    for r in range(REPEATS + 1):  # (repeat 0 warms every call up and is not reported)
        buf = DeviceBuffer(g, W, H)
        t_b = 0.0
        for b in range(N):
            t_b += timed(lambda: buf.sample(camera, make_params(W, H, B, S, seed=SEED, sample_index_base=b * S)))[0]
        t_f = timed(lambda: buf.features(camera, pf))[0]
        t_a = timed(lambda: g.render_aov(camera, pf, dn))[0]
        t_3, d3 = timed(lambda: buf.denoise(levels=3))
        t_5, d5 = timed(lambda: buf.denoise(levels=5))
        if r:
            for k, t in zip(times, (t_b, t_f, t_a, t_3, t_5)):
                times[k].append(t)
        if r == REPEATS:
            totals, counts = buf.totals(), buf.sample_counts()
            quality = dict(raw=rmse(totals / counts[..., None], ref), box1=rmse(box1(totals, counts), ref),
                           denoise3=rmse(d3, ref), denoise5=rmse(d5, ref))
            # a plain run's way to the denoised frames' RMSE: go on sampling
            target = min(quality["denoise3"], quality["denoise5"])
            curve = {N: quality["raw"]}
            n = N
            while curve[n] > target and n < UNIFORM_CAP:
                buf.sample(camera, make_params(W, H, B, S, seed=SEED, sample_index_base=n * S))
                n += 1
                if n % 8 == 0 or n == UNIFORM_CAP:
                    curve[n] = rmse(buf.totals() / float(n), ref)
                else:
                    curve[n] = curve[n - 1]
            same = {}
            for k in ("denoise3", "denoise5"):
                reached = [m for m in sorted(curve) if m % 8 == 0 and curve[m] <= quality[k]]
                if reached:
                    same[k] = dict(samples_per_pixel=reached[0] * S, measured=True)
                else:  # rmse ~ 1 / sqrt(n) from the last measured point
                    same[k] = dict(samples_per_pixel=int(round(n * S * (curve[n] / quality[k]) ** 2)), measured=False)
            quality["uniform_rmse_by_batches"] = {str(m): round(curve[m], 6) for m in sorted(curve) if m % 8 == 0}
            quality["uniform_samples_to_same_rmse"] = same
            quality["samples_per_pixel"] = N * S
        buf.close()
    g.close()
    wall = {k: stats(v) for k, v in times.items()}
    fd = wall["features"]["median_s"]
    return dict(scene=name, width=W, height=H, max_bounces=B, spp_per_batch=S, batches=N, feature_spp=FEATURE_SPP,
                repeats=REPEATS, reference=dict(spp=ref_spp, seed=SEED + 1, wall_s=round(ref_s, 3)), wall=wall,
                features_plus_denoise3_over_batches=round((fd + wall["denoise3"]["median_s"]) / wall["batches"]["median_s"], 4),
                features_plus_denoise5_over_batches=round((fd + wall["denoise5"]["median_s"]) / wall["batches"]["median_s"], 4),
                features_over_aov_dn=round(fd / wall["aov_dn"]["median_s"], 4),
                rmse={k: (round(v, 6) if isinstance(v, float) else v) for k, v in quality.items()})


def trace(name):
    scene, camera, cfg = getattr(scenes, name)()
    W, H = cfg["width"], cfg["height"]
    B = CONFIGS[name][0]
    g = GpuScene(scene, 0)
    buf = DeviceBuffer(g, W, H)
    for b in range(2):
        buf.sample(camera, make_params(W, H, B, 1, seed=SEED, sample_index_base=b))
    buf.features(camera, make_params(W, H, B, FEATURE_SPP, seed=SEED))
    for _ in range(2):
        buf.denoise(levels=3)
    buf.close()
    g.close()


def merge_stats(directory, out_path):
    lines = [json.loads(l) for l in open(out_path)] if os.path.exists(out_path) else []
    by_scene = {l["scene"]: l for l in lines if "scene" in l}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*_kernel_stats.csv"), recursive=True)):
        scene = os.path.basename(path)[:-len("_kernel_stats.csv")]
        if scene not in CONFIGS:
            continue
        l = by_scene.setdefault(scene, dict(scene=scene))
        npix = l.get("width", 0) * l.get("height", 0)
        kernels = {}
        for r in csv.DictReader(open(path)):
            if "rpt_denoise" not in r["Name"] and "rpt_aov" not in r["Name"]:
                continue
            short = r["Name"].split("(")[0].split("::")[-1]
            ms = float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e6
            kernels[short] = dict(calls=int(r["Calls"]), mean_ms=round(ms, 4))
            if short == "rpt_denoise_level" and npix:
                gb = npix * LEVEL_BYTES_PER_PIXEL / 1e9
                kernels[short].update(bytes_a_level_must_move_gb=round(gb, 4), gbs_by_shape=round(gb / (ms / 1e3), 1),
                                      share_of_hbm_peak_by_shape=round(gb / (ms / 1e3) / HBM_PEAK_GBS, 4))
        l["kernel"] = kernels
    with open(out_path, "w") as f:
        for l in by_scene.values():
            f.write(json.dumps(l) + "\n")
            print(json.dumps(l))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--merge-stats", default=None, metavar="DIR")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (--merge-stats: rewrite it)")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out or os.path.join(ROOT, "profiles", "denoise_bench.json"))
    for name in ([args.scene] if args.scene else ["cornell", "wine_glass"]):
        if args.trace:
            trace(name)
            continue
        line = json.dumps(bench(name))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
