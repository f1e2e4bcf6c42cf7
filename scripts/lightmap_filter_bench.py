"""Wall time of rptgpu_filter_lightmap_device against what a caller writes today: the same filter as torch
operations on the same device — 25 taps times the levels, each a handful of array operations over the whole map.

Workloads, both a --size^2 IRRADIANCE map of rptgpu_bake_lightmap_device at --samples and --bounces, filtered at --levels levels
in device memory with sigma_distance = 3 texel extents and sigma_plane = 1 (lightmap.texel_extent), no variance, no dilation:
  atlas   the C3 mesh (scenes.dragon's knot, in world space) under lightmap_bench's synthetic atlas
  quad    one two-triangle chart over the whole map, on scenes.cornell's floor
The two sides run in one process, alternating: after two warm-ups of each, five repeats of host wall time around the
synchronous calls: median, min and max.  torch's exp is not rpt_exp, so the two results are not bit-equal: the line reports
the largest relative difference between them over the owned texels.  The one gate: the call on the map's first 128 x 128
texels must equal tests/lightmap_filter_model.py, the header restated in numpy, in every bit — the script exits with status 1
after writing its lines when it does not.  No threshold otherwise: the figures are recorded as they come.

    python scripts/lightmap_filter_bench.py [--size 2048] [--samples 64] [--bounces 8] [--levels 3]
                                            [--workloads atlas quad] [--out profiles/lightmap_filter_bench.json]

--trace: per workload one bake and two calls of the filter and nothing else — the process to profile, in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python scripts/lightmap_filter_bench.py --trace
--summarize CSV: from that run's kernel statistics the level kernel's time per launch, the filter's share of the run's
kernel time per (bake + one filter call), and the level kernel's ACHIEVED bytes per second — the bytes of the columns a
level must read and write once (1 validity byte, 3 + 3 guide columns, `words` value columns in and out, 97 B per texel at 3
words) over its time, against the 8.0 TB/s HBM3E peak; taps re-read columns through the L2, so this is a lower bound on the
traffic and the figure is named achieved_min_bytes_per_s.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rpt_amd import GpuScene, _abi, lightmap, scenes  # noqa: E402
from lightmap_bench import atlas, summary, world_triangles  # noqa: E402

SEED = 0x52505447
REPEATS, WARMUPS = 5, 2
CHANNELS = _abi.RPT_LIGHTMAP_IRRADIANCE | _abi.RPT_LIGHTMAP_OWNER | _abi.RPT_LIGHTMAP_POSITION | _abi.RPT_LIGHTMAP_NORMAL
HBM_PEAK = 8.0e12
K = {-2: 0.0625, -1: 0.25, 0: 0.375, 1: 0.25, 2: 0.0625}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def torch_filter(torch, c, valid, P, N, levels, sigma_normal, sigma_plane, sigma_distance):
    """the header's levels (no variance) as torch operations over the map: what a caller writes today"""
    h, w = valid.shape
    inf = float("inf")

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    for l in range(levels):
        step = 1 << l
        sd = sigma_distance * float(step)
        C, W = torch.zeros_like(c), torch.zeros_like(c[..., 0])
        for dx in range(-2, 3):
            for dy in range(-2, 3):
                ox, oy = dx * step, dy * step
                x0, x1, y0, y1 = max(0, -ox), min(w, w - ox), max(0, -oy), min(h, h - oy)
                if x0 >= x1 or y0 >= y1:
                    continue
                p, q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                w0 = K[dx] * K[dy]
                cq, ok = c[q], valid[q]
                if dx == 0 and dy == 0:
                    wt = torch.full_like(W[p], w0)
                else:
                    ok = ok & (cq.abs() < inf).all(dim=-1)
                    D = P[q] - P[p]
                    t = 1.0 - dot(N[p], N[q])
                    e = (torch.where(t > 0.0, t, torch.zeros_like(t)) / sigma_normal + dot(N[p], D).abs() / sigma_plane) + dot(D, D) / (sd * sd)
                    ok = ok & (e >= 0.0) & (e < inf)
                    wt = w0 * torch.exp(-torch.where(ok, e, torch.zeros_like(e)))
                C[p] = torch.where(ok[..., None], C[p] + wt[..., None] * cq, C[p])
                W[p] = torch.where(ok, W[p] + wt, W[p])
        c = torch.where(valid[..., None], C / W[..., None], c)
    return c


def workload(name, size):
    if name == "atlas":
        scene = scenes.dragon()[0]
        positions = world_triangles(scene.objects[0].shape)
        uvs, _ = atlas(len(positions), size)
    else:
        scene = scenes.cornell()[0]
        positions = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 559.2], [556.0, 0.0, 559.2]],
                              [[0.0, 0.0, 0.0], [556.0, 0.0, 559.2], [556.0, 0.0, 0.0]]])
        uvs = np.array([[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]])
    return scene, positions, np.ascontiguousarray(uvs, dtype=np.float64)


def bench(name, args, dev):
    import torch
    import lightmap_filter_model as model
    size, levels = args.size, args.levels
    scene, positions, uvs = workload(name, size)
    g = GpuScene(scene, 0)
    offset = 1e-4 * float(np.abs(positions).max())
    bake = g.bake_lightmap(torch.from_numpy(positions).to(dev), torch.from_numpy(uvs).to(dev), size, size, samples=args.samples,
                           max_bounces=args.bounces, seed=SEED, offset=offset, channels=CHANNELS)
    values, owner, position, normal = bake["irradiance"], bake["owner"], bake["position"], bake["normal"]
    extent = lightmap.texel_extent(position.cpu().numpy(), owner.cpu().numpy())
    kw = dict(sigma_distance=3.0 * extent, sigma_plane=extent, sigma_normal=0.1, levels=levels)
    state = {}

    def this():
        state["this"] = g.filter_lightmap(values, owner, position, normal, **kw)

    def before():
        state["before"] = torch_filter(torch, values, owner >= 0, position, normal, levels, kw["sigma_normal"], kw["sigma_plane"],
                                       kw["sigma_distance"])
        torch.cuda.synchronize()

    if args.trace:
        this()
        this()
        g.close()
        return None
    runs = {"filter_lightmap_device": this, "torch_ops_same_device": before}
    for f in runs.values():
        for _ in range(WARMUPS):
            f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    a, b = state["this"].cpu().numpy(), state["before"].cpu().numpy()
    own = owner.cpu().numpy() >= 0
    with np.errstate(all="ignore"):
        rel = np.abs(a[own] - b[own]) / np.maximum(np.abs(b[own]), 1e-300)
    rel = rel[np.isfinite(rel)]
    # the gate: the first 128 x 128 texels, a map of their own, against the numpy model
    k = min(128, size)
    crop = [np.ascontiguousarray(t[:k, :k].cpu().numpy()) for t in (values, owner, position, normal)]
    got = g.filter_lightmap(*crop, **kw)
    equal = bool(np.array_equal(bits(got), bits(model.filter_lightmap(*crop, **kw))))
    res = dict(bench="lightmap_filter", workload=name, map=[size, size], owned_texels=int(own.sum()), words=3, levels=levels,
               variance=False, dilate=0, bake_samples=args.samples, bake_max_bounces=args.bounces, texel_extent=extent,
               sigma_distance=kw["sigma_distance"], sigma_plane=kw["sigma_plane"], sigma_normal=kw["sigma_normal"],
               repeats=REPEATS, warmups=WARMUPS, gpu=torch.cuda.get_device_name(0), runs={v: summary(wall[v]) for v in runs},
               max_relative_difference_to_torch=float(rel.max()) if len(rel) else 0.0, crop=[k, k], crop_bit_equal_to_model=equal)
    res["speedup"] = round(res["runs"]["torch_ops_same_device"]["wall_median_s"] / res["runs"]["filter_lightmap_device"]["wall_median_s"], 2)
    res["mtexels_per_s"] = round(size * size / res["runs"]["filter_lightmap_device"]["wall_median_s"] / 1e6, 1)
    g.close()
    return res


def summarize(path, size, words, levels, workloads):
    """rocprofv3's kernel_stats CSV of a --trace run -> one line"""
    rows = {}
    if path.endswith(".db"):  # rocprofv3's default output: the database's top_kernels view
        import sqlite3
        for name, calls, total in sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"):
            rows[name] = (int(calls), float(total))
    else:                     # --output-format csv: <name>_kernel_stats.csv
        with open(path) as f:
            for r in csv.DictReader(f):
                rows[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    total = sum(t for _, t in rows.values())
    mine = {k: v for k, v in rows.items() if "rpt_lightmap_filter_" in k}
    level = [(c, t) for k, (c, t) in mine.items() if "filter_level" in k]
    calls, ns = sum(c for c, _ in level), sum(t for _, t in level)
    filter_ns = sum(t for _, t in mine.values())
    n = size * size
    per_launch = ns / calls if calls else float("nan")
    min_bytes = n * (1 + 8 * (6 + 2 * words))
    # the run: per workload one bake and two filter calls
    one_filter = filter_ns / (2.0 * workloads)
    bake_ns = total - filter_ns
    return dict(bench="lightmap_filter_trace", map=[size, size], words=words, levels=levels, level_kernel_launches=calls,
                level_kernel_ns_per_launch=round(per_launch, 1), filter_kernels_ns_per_call=round(one_filter, 1),
                other_kernels_ns=round(bake_ns, 1),
                filter_share_of_bake_plus_filter_kernel_time=round(one_filter * workloads / (bake_ns + one_filter * workloads), 4),
                level_min_bytes=min_bytes, achieved_min_bytes_per_s=round(min_bytes / (per_launch * 1e-9), 1),
                hbm_peak_bytes_per_s=HBM_PEAK, achieved_min_fraction_of_hbm_peak=round(min_bytes / (per_launch * 1e-9) / HBM_PEAK, 4),
                kernels={k: dict(calls=c, total_ns=t) for k, (c, t) in sorted(mine.items())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["atlas", "quad"], choices=["atlas", "quad"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None, metavar="CSV")
    args = ap.parse_args()
    if args.summarize:
        line = json.dumps(summarize(args.summarize, args.size, 3, args.levels, len(args.workloads)))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        return 0
    import torch
    dev = torch.device("cuda", 0)
    lines, ok = [], True
    for name in args.workloads:
        res = bench(name, args, dev)
        if res is None:
            continue
        ok = ok and res["crop_bit_equal_to_model"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
