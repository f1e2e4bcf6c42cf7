"""Wall time of rptgpu_hit_surface_device against its floor: the same rays through rptgpu_first_hits_device with
T | OBJECT — the query the call runs first, unchanged — in the parent commit's build (--parent-lib; else this one's, and the
line says so).  What the resolve walk costs on top is the ratio.

The workload: the 1920x1080 pinhole rays of the camera of the C3 mesh (scenes.dragon), scenes.fractal_spheres and
scenes.cornell, through pixel centres, in device memory: 2.07 M rays.
  (a) hit_surface_device, all channels              t, object, child, primitive, barycentric
  (b) hit_surface_device, PRIMITIVE | BARYCENTRIC   T and OBJECT go to the handle's own pair
  (c) first_hits_device, T | OBJECT                 the floor, --parent-lib's build
  (d) (a) through --from-inf-lib                    a build with -DRPT_SURFACE_FROM_INF=1: the resolve walk started from +inf
                                                    instead of the next double above t — what the cut is worth
(a)'s t and object must equal (c)'s, (b)'s two channels (a)'s, and (d) every channel of (a), in every bit; the script exits with
status 1 after writing its lines when they do not.  After two warm-ups of each, five alternating repeats of host wall time
around the synchronous calls: median, min and max, M rays/s from the median.  No threshold: the figures are recorded as they
come; a run that was not made is "not measured".

    python scripts/hit_surface_bench.py [--parent-lib LIB] [--from-inf-lib LIB] [--size 1920 1080]
                                        [--scenes dragon fractal_spheres cornell] [--out profiles/hit_surface_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rpt_amd import GpuScene, _abi, scenes  # noqa: E402
from rpt_amd.scene import geometry_snapshot  # noqa: E402
from occlusion_bench import REPEATS, summary  # noqa: E402

WARMUPS = 2
WALK = _abi.RPT_SURFACE_PRIMITIVE | _abi.RPT_SURFACE_BARYCENTRIC


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def open_scene(path, scene):
    """a GpuScene on ANOTHER build of the library (GpuScene's constructor with that build's symbols)"""
    g = GpuScene.__new__(GpuScene)
    g.lib = _abi.load_library(path)
    desc, keep = scene.lower()
    h = C.c_void_p()
    _abi.check(g.lib.rptgpu_scene_create(C.byref(desc), 0, C.byref(h)))
    g.handle, g.device, g._geometry = h, 0, geometry_snapshot(scene)
    return g


def pinhole_rays(camera, width, height):
    """one ray per pixel through its centre: eye, and direction * d + right * x + up * y with d = 1 / tan(fov / 2), x and y
    in [-1, 1] on the longer side (Camera::cast_ray's frame, camera.rs:64-81, without jitter and lens)"""
    eye = np.array([float(c) for c in camera.eye])
    fwd = np.array([float(c) for c in camera.direction])
    up = np.array([float(c) for c in camera.up])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    dist = 1.0 / np.tan(float(camera.fov) / 2.0)
    side = float(max(width, height))
    x = (2.0 * (np.arange(width) + 0.5) - width) / side
    y = (height - 2.0 * (np.arange(height) + 0.5)) / side
    d = fwd[None, None, :] * dist + right[None, None, :] * x[None, :, None] + up[None, None, :] * y[:, None, None]
    o = np.broadcast_to(eye, d.shape)
    return np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))


def bench(name, scene, camera, width, height, parent_lib, from_inf_lib, dev):
    import torch
    g = GpuScene(scene, 0)
    floor = open_scene(parent_lib, scene) if parent_lib else g
    inf = open_scene(from_inf_lib, scene) if from_inf_lib else None
    o, d = pinhole_rays(camera, width, height)
    N = len(o)
    d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.cuda.synchronize(dev)
    answers = {}

    def run(key, f):
        def call():
            answers[key] = f()
        return call

    runs = {"hit_surface_all": run("hit_surface_all", lambda: g.hit_surface(d_o, d_d)),
            "hit_surface_primitive_barycentric": run("hit_surface_primitive_barycentric", lambda: g.hit_surface(d_o, d_d, channels=WALK)),
            "first_hits_t_object": run("first_hits_t_object", lambda: floor.first_hits(d_o, d_d, channels=_abi.RPT_HIT_T | _abi.RPT_HIT_OBJECT))}
    if inf is not None:
        runs["hit_surface_all_from_inf"] = run("hit_surface_all_from_inf", lambda: inf.hit_surface(d_o, d_d))
    for _ in range(WARMUPS):  # code objects, workspace, the walk's columns
        for f in runs.values():
            f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):
        for v, f in runs.items():
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    host = {v: {k: a.cpu().numpy() for k, a in answers[v].items()} for v in runs}
    full = host["hit_surface_all"]
    same = lambda a, b, keys: all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)
    equal = same(full, host["first_hits_t_object"], ("t", "object")) and \
        same(full, host["hit_surface_primitive_barycentric"], ("primitive", "barycentric")) and \
        (inf is None or same(full, host["hit_surface_all_from_inf"], sorted(full)))
    res = dict(bench="hit_surface", scene=name, width=width, height=height, rays=N, repeats=REPEATS, warmups=WARMUPS,
               floor_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               rays_with_a_hit=round(float((full["object"] >= 0).mean()), 4),
               rays_on_a_triangle=round(float((full["primitive"] >= 0).mean()), 4),
               rays_on_a_groups_child=round(float((full["child"] >= 0).mean()), 4),
               runs={v: summary(wall[v], N) for v in runs}, answers_bit_equal=bool(equal),
               bytes_per_ray={"hit_surface_all": {"in": 48, "out": 44}, "hit_surface_primitive_barycentric": {"in": 48, "out": 28},
                              "first_hits_t_object": {"in": 48, "out": 12}})
    floor_s = res["runs"]["first_hits_t_object"]["wall_median_s"]
    for v in ("hit_surface_all", "hit_surface_primitive_barycentric"):
        res[v + "_over_floor"] = round(res["runs"][v]["wall_median_s"] / floor_s, 3)
    if inf is not None:
        res["from_inf_over_cut"] = round(res["runs"]["hit_surface_all_from_inf"]["wall_median_s"] / res["runs"]["hit_surface_all"]["wall_median_s"], 3)
        inf.close()
    else:
        res["from_inf_over_cut"] = "not measured"
    if floor is not g:
        floor.close()
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--from-inf-lib", default=None)
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--scenes", nargs="+", default=["dragon", "fractal_spheres", "cornell"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name in args.scenes:
        scene, camera, _ = getattr(scenes, name)()
        res = bench(name, scene, camera, args.size[0], args.size[1], args.parent_lib, args.from_inf_lib, dev)
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
