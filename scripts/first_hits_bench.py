"""Wall time of rptgpu_first_hits_device against what a caller did before it existed: the same rays through
rptgpu_closest_hit — host arrays — plus the numpy that forms position and albedo.  The baseline runs through another build of
the library with --parent-lib (the parent commit's: a kept copy, or scripts/build_variant.sh on that commit), else through
this one.

The workload is scripts/occlusion_bench.py's: the C3 mesh (scenes.dragon), scenes.fractal_spheres and scenes.cornell; one
point per pixel of a 1920x1080 frame (sample 0's first hit, lifted off its surface), 16 cosine-weighted directions each — the
rays of rptgpu_bake_ao, read back from the library once, outside the timed region: 33.2 M rays.
  (a) first_hits_device, T | OBJECT      rays in device memory -> t and object per ray
  (b) first_hits_device, all channels    ... -> t, normal, object, position, albedo
  (c) closest_hit + numpy                the same rays from host memory -> t, normal, object; position = o + t * d and
                                         albedo = colour[object] in numpy (misses +0.0)
  (d) occluded_device                    the same rays through the any-hit query, beside them as the floor
(b) and (c) must agree in every bit of all five channels, (a) with (b) in its two, and (d) with `t <= DBL_MAX`; the script
exits with status 1 after writing its lines when they do not.  After one warm-up of each, five alternating repeats of host
wall time around the synchronous calls: median, min and max, M rays/s from the median, and the bytes per ray that cross the ABI
either way.  No threshold: the figures are recorded as they come.

    python scripts/first_hits_bench.py [--parent-lib LIB] [--size 1920 1080] [--samples 16] [--scenes dragon fractal_spheres cornell]
                                       [--out profiles/first_hits_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rpt_amd import GpuScene, _abi, scenes  # noqa: E402
from occlusion_bench import DBL_MAX, REPEATS, SEED, RawScene, points_of, summary  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def bench(name, scene, camera, width, height, S, parent_lib, dev):
    import torch
    g = GpuScene(scene, 0)
    base = RawScene(parent_lib or _abi.LIB_PATH, scene)
    pos, nrm, hit_share = points_of(g, camera, width, height)
    n = len(pos)
    d_pos, d_nrm = torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev)
    d_dirs = torch.empty((n, S, 3), dtype=torch.float64, device=dev)
    ao1, bent1 = torch.empty(n, dtype=torch.float64, device=dev), torch.empty((n, 3), dtype=torch.float64, device=dev)
    for k in range(S):  # direction k of every point from the library itself (occlusion_bench.py says how)
        g.bake_ao(d_pos, d_nrm, samples=1, seed=SEED, sample_index_base=k, max_distance=-1.0, bent_normals=True, out=(ao1, bent1))
        d_dirs[:, k] = bent1
    d_o = d_pos[:, None, :].expand(n, S, 3).reshape(-1, 3).contiguous()
    d_d = d_dirs.reshape(-1, 3)
    h_o, h_d = d_o.cpu().numpy(), d_d.cpu().numpy()
    torch.cuda.synchronize(dev)
    N = n * S
    colour = np.array([list(ob._material.lower().color) for ob in scene.objects], dtype=np.float64).reshape(-1, 3)
    t, hn, obj = np.empty(N), np.empty((N, 3)), np.empty(N, dtype=np.int32)
    out_occ = torch.empty(N, dtype=torch.uint8, device=dev)
    answers = {}

    def first_hits_t_object():
        answers["first_hits_t_object"] = g.first_hits(d_o, d_d, channels=_abi.RPT_HIT_T | _abi.RPT_HIT_OBJECT)

    def first_hits_all():
        answers["first_hits_all"] = g.first_hits(d_o, d_d)

    def closest_hit_host():
        base.closest_hit(h_o, h_d, t, hn, obj)
        hit = obj >= 0
        with np.errstate(all="ignore"):
            position = np.where(hit[:, None], h_o + t[:, None] * h_d, 0.0)
        albedo = np.where(hit[:, None], colour[np.maximum(obj, 0)], 0.0)
        answers["closest_hit_host"] = {"t": t, "normal": hn, "object": obj, "position": position, "albedo": albedo}

    def occluded_device():
        g.occluded(d_o, d_d, out=out_occ)
        answers["occluded_device"] = out_occ

    runs = {"first_hits_t_object": first_hits_t_object, "first_hits_all": first_hits_all, "closest_hit_host": closest_hit_host,
            "occluded_device": occluded_device}
    for f in runs.values():  # warm-up: code objects, workspace, staging arrays
        f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):
        for v, f in runs.items():
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    want = answers["closest_hit_host"]
    full = {k: v.cpu().numpy() for k, v in answers["first_hits_all"].items()}
    two = {k: v.cpu().numpy() for k, v in answers["first_hits_t_object"].items()}
    equal = all(np.array_equal(bits(full[k]), bits(want[k])) for k in want) and sorted(two) == ["object", "t"] and \
        all(np.array_equal(bits(two[k]), bits(want[k])) for k in two) and \
        np.array_equal(answers["occluded_device"].cpu().numpy(), (~(want["t"] > DBL_MAX)).astype(np.uint8))
    res = dict(bench="first_hits", scene=name, width=width, height=height, points=n, samples=S, rays=N, repeats=REPEATS,
               baseline_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               pixels_with_a_hit=round(hit_share, 4), rays_with_a_hit=round(float((want["object"] >= 0).mean()), 4),
               runs={v: summary(wall[v], N) for v in runs}, answers_bit_equal=bool(equal),
               bytes_per_ray={"first_hits_t_object": {"in": 48, "out": 12}, "first_hits_all": {"in": 48, "out": 100},
                              "closest_hit_host": {"in": 48, "out": 36}, "occluded_device": {"in": 48, "out": 1}})
    for v in ("first_hits_t_object", "first_hits_all"):
        res[v + "_over_closest_hit_host"] = round(res["runs"][v]["mrays_per_s"] / res["runs"]["closest_hit_host"]["mrays_per_s"], 2)
        res[v + "_over_occluded_device"] = round(res["runs"][v]["mrays_per_s"] / res["runs"]["occluded_device"]["mrays_per_s"], 3)
    base.close()
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--scenes", nargs="+", default=["dragon", "fractal_spheres", "cornell"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name in args.scenes:
        scene, camera, _ = getattr(scenes, name)()
        res = bench(name, scene, camera, args.size[0], args.size[1], args.samples, args.parent_lib, dev)
        if not res["answers_bit_equal"]:
            bad.append("%s: the answers differ" % name)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for b in bad:
        print("FAILED: " + b, file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
