"""Wall time of rptgpu_bake_direct_device against the floor of its query: rptgpu_bake_ao_device through the
parent commit's build (--parent-lib: a kept copy; else through this build, and the line says so) on the same points with
S x (non-ambient lights) directions — the same number of shadow rays, without the light samples in front of them and
without the queues that leave out the rays of lights facing away.

Workloads: the C3 mesh (scenes.dragon), scenes.fractal_spheres and scenes.cornell.  One point per pixel of a 1920x1080
frame, scripts/occlusion_bench.py's: the first hit of sample 0 and its normal, lifted off the surface; a pixel that sees
nothing stands at the camera.  S = 16 light samples per point and light.  Positions, normals and results in device memory.
After two warm-ups of each side, five alternating repeats of host wall time around the synchronous calls: median, min and
max.  The direct results of all repeats must be equal in every bit; the script exits with status 1 after writing its lines
when they are not.  No threshold: the figures are recorded as they come; a run that was not made is "not measured".

    python scripts/direct_bench.py [--parent-lib LIB] [--size 1920 1080] [--samples 16] [--scenes dragon fractal_spheres cornell]
                                   [--out profiles/direct_bench.json]
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

from rpt_amd import GpuScene, _abi  # noqa: E402
from rpt_amd import scenes  # noqa: E402
from hit_surface_bench import open_scene  # noqa: E402
from occlusion_bench import points_of  # noqa: E402

SEED = 0x52505447
REPEATS, WARMUPS = 5, 2


def summary(wall, n_rays):
    med = float(np.median(wall))
    return dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(med, 5), wall_min_s=round(min(wall), 5),
                wall_max_s=round(max(wall), 5), mrays_per_s=round(n_rays / med / 1e6, 1))


def bench(name, scene, camera, width, height, S, parent_lib, dev):
    import torch
    g = GpuScene(scene, 0)
    gp = open_scene(parent_lib, scene) if parent_lib else g
    pos, nrm, hit_share = points_of(g, camera, width, height)
    n = len(pos)
    casting = sum(l.kind != _abi.RPT_LIGHT_AMBIENT for l in scene.lights)
    d_pos, d_nrm = torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev)
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    out_ao = torch.empty(n, dtype=torch.float64, device=dev)
    results = []

    def bake_direct_device():
        g.bake_direct(d_pos, d_nrm, samples=S, seed=SEED, out=out)

    def bake_ao_device_parent():
        gp.bake_ao(d_pos, d_nrm, samples=S * casting, seed=SEED, out=out_ao)

    runs = {"bake_direct_device": bake_direct_device, "bake_ao_device_parent": bake_ao_device_parent}
    for f in runs.values():  # warm-up: code objects, workspace
        for _ in range(WARMUPS):
            f()
    g.reset_stats()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            wall[v].append(time.perf_counter() - t0)
            if f is bake_direct_device:  # (outside the timed region: the repeat's result, for the comparison below)
                results.append(out.cpu().numpy().tobytes())
    st = g.stats()
    a = np.frombuffer(results[0], dtype=np.float64).reshape(n, 3)
    res = dict(bench="direct", scene=name, width=width, height=height, points=n, samples=S, casting_lights=casting,
               shadow_rays=n * S * casting, shadow_rays_traced_per_call=int(st.shadow_rays_traced // REPEATS), repeats=REPEATS,
               warmups=WARMUPS, gpu=torch.cuda.get_device_name(0),
               parent_lib=os.path.basename(parent_lib) if parent_lib else "not measured (the baseline ran on this build)",
               pixels_with_a_hit=round(hit_share, 4), lit_points=round(float((a != 0.0).any(axis=1).mean()), 4),
               mean_direct=[round(float(c), 6) for c in a.mean(axis=0)],
               runs={v: summary(wall[v], n * S * casting) for v in runs}, repeats_bit_equal=all(r == results[0] for r in results))
    res["direct_over_ao_floor"] = round(res["runs"]["bake_direct_device"]["wall_median_s"] /
                                        res["runs"]["bake_ao_device_parent"]["wall_median_s"], 3)
    g.close()
    if gp is not g:
        gp.close()
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
        if not res["repeats_bit_equal"]:
            bad.append("%s: the direct results of the repeats differ" % name)
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
