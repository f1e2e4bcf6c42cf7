"""Wall time of rptgpu_render_views_aov against what a caller did before it existed: a loop of
rptgpu_render_aov, one call per view.  The baseline runs through another build of the library with --parent-lib (the parent
commit's: a kept copy, or scripts/build_variant.sh on that commit), else through this one.

Workloads: scenes.fractal_spheres and scenes.cornell; 16 and 64 perspective views on a turntable about the point the scene's
camera looks at, 480x270, 4 samples per pixel, all channels; seed_stride 0 and 1 and one run with seeds that are no
arithmetic sequence (rptgpu_render_views_aov_seeded; seed_stride "seeds" in its line), reported separately (the seed
travels with the ray, DESIGN.md §15.1: the launches are shared whatever the seeds).
  (a) render_views_aov          host arrays, one call
  (b) render_views_aov_device   torch tensors on the device, one call
  (c) render_aov per view       host arrays, n calls with the view's seed
  (d) with seed_stride 1: (a) through the --parent-lib build, where every view is a piece of its own (`views_aov_host_parent`)
(a), (b), (c) and (d) must agree in every bit of every channel; the script exits with status 1 after writing its lines when they
do not.  After one warm-up of each, five alternating repeats of host wall time around the synchronous calls: median, min and
max, M primary rays/s from the median.  No threshold: the figures are recorded as they come.

    python scripts/views_aov_bench.py [--parent-lib LIB] [--size 480 270] [--spp 4] [--views 16 64] [--scenes fractal_spheres cornell]
                                      [--out profiles/views_aov_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rpt_amd import Camera, GpuScene, _abi, make_params, scenes  # noqa: E402
from occlusion_bench import REPEATS, SEED, summary  # noqa: E402
from views_bench import scattered_seeds  # noqa: E402

NAMES = ("hits", "depth", "normal", "albedo", "position", "object")


class RawAov:
    """rptgpu_render_aov bound on ANY build of the library (an older one lacks symbols that _abi.load_library insists on)"""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        self.lib.rptgpu_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.rptgpu_render_aov.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib.rptgpu_render_views_aov.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib.rptgpu_scene_destroy.argtypes = [C.c_void_p]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def render_aov(self, cam, params, arrays, v):
        b = _abi.RptAovBuffers()
        b.struct_size, b.channels = C.sizeof(b), _abi.RPT_AOV_ALL
        types = dict(_abi.RptAovBuffers._fields_)
        for k in NAMES:
            setattr(b, k, arrays[k][v].ctypes.data_as(types[k]))
        rc = self.lib.rptgpu_render_aov(self.h, C.byref(cam), C.byref(params), C.byref(b))
        if rc != 0:
            raise RuntimeError("rptgpu_render_aov: %d" % rc)

    def render_views_aov(self, n, views, q, arrays):
        b = _abi.RptAovBuffers()
        b.struct_size, b.channels = C.sizeof(b), _abi.RPT_AOV_ALL
        types = dict(_abi.RptAovBuffers._fields_)
        for k in NAMES:
            setattr(b, k, arrays[k].ctypes.data_as(types[k]))
        rc = self.lib.rptgpu_render_views_aov(self.h, n, views, C.byref(q), C.byref(b))
        if rc != 0:
            raise RuntimeError("rptgpu_render_views_aov: %d" % rc)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def turntable(camera, n):
    """n cameras on a circle about the point the scene's camera looks at, in the plane across its up vector"""
    eye, direction, up = (np.array([float(c) for c in v]) for v in (camera.eye, camera.direction, camera.up))
    L = float(np.linalg.norm(eye)) or 1.0
    target = eye + direction / np.linalg.norm(direction) * L
    up = up / np.linalg.norm(up)
    arm = eye - target
    side = np.cross(up, arm)
    out = []
    for k in range(n):
        a = 2.0 * math.pi * k / n
        e = target + math.cos(a) * arm + math.sin(a) * side
        out.append(Camera.look_at(tuple(e), tuple(target), tuple(up), camera.fov))
    return out


def host_arrays(n, h, w):
    return {"hits": np.zeros((n, h, w), dtype=np.uint32), "depth": np.zeros((n, h, w)), "normal": np.zeros((n, h, w, 3)),
            "albedo": np.zeros((n, h, w, 3)), "position": np.zeros((n, h, w, 3)), "object": np.zeros((n, h, w), dtype=np.int32)}


def bench(name, scene, camera, width, height, spp, n_views, stride, parent_lib, dev):
    """stride: 0, 1, or "seeds" — seeds that are no arithmetic sequence, through the _seeded entry points"""
    import torch
    seeds = scattered_seeds(n_views) if stride == "seeds" else [SEED + v * stride for v in range(n_views)]
    how = dict(seeds=seeds) if stride == "seeds" else dict(seed=SEED, seed_stride=stride)
    g = GpuScene(scene, 0)
    base = RawAov(parent_lib or _abi.LIB_PATH, scene)
    views = turntable(camera, n_views)
    lowered = [v.lower() for v in views]
    loop_out = host_arrays(n_views, height, width)
    dev_out = {k: torch.zeros(a.shape, dtype=torch.float64 if a.dtype == np.float64 else torch.int32, device=dev)
               for k, a in loop_out.items()}
    answers = {}

    host_out = host_arrays(n_views, height, width)  # (as the loop's: made once, outside the timed region)

    def views_aov_host():
        answers["views_aov_host"] = g.render_views_aov(views, width, height, samples=spp, out=host_out, **how)

    def views_aov_device():
        g.render_views_aov(views, width, height, samples=spp, out=dev_out, **how)
        answers["views_aov_device"] = dev_out

    def render_aov_loop():
        for v in range(n_views):
            base.render_aov(lowered[v], make_params(width, height, 0, spp, seed=seeds[v]), loop_out, v)
        answers["render_aov_loop"] = loop_out

    runs = {"views_aov_host": views_aov_host, "views_aov_device": views_aov_device, "render_aov_loop": render_aov_loop}
    if stride == 1:  # the same call on the baseline's build
        parent_out = host_arrays(n_views, height, width)
        arr = GpuScene._lower_views(views, "views_aov_bench")
        q = _abi.RptViewQuery()
        q.struct_size, q.width, q.height, q.iterations = C.sizeof(_abi.RptViewQuery), width, height, spp
        q.seed, q.seed_stride, q.precision_mode = SEED, 1, _abi.RPT_PRECISION_F64_STRICT

        def views_aov_host_parent():
            base.render_views_aov(n_views, arr, q, parent_out)
            answers["views_aov_host_parent"] = parent_out

        runs["views_aov_host_parent"] = views_aov_host_parent
    for f in runs.values():  # warm-up: code objects, workspace, staging arrays
        f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):
        for v, f in runs.items():
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    want = answers["render_aov_loop"]
    got_dev = {k: t.cpu().numpy().view(want[k].dtype) for k, t in answers["views_aov_device"].items()}
    equal = all(answers["views_aov_host"][k].tobytes() == want[k].tobytes() and got_dev[k].tobytes() == want[k].tobytes() for k in NAMES)
    if stride == 1:
        equal = equal and all(answers["views_aov_host_parent"][k].tobytes() == want[k].tobytes() for k in NAMES)
    rays = n_views * width * height * spp
    res = dict(bench="views_aov", scene=name, width=width, height=height, spp=spp, views=n_views, seed_stride=stride, rays=rays,
               repeats=REPEATS, baseline_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               rays_with_a_hit=round(float(want["hits"].sum()) / rays, 4),
               runs={v: summary(wall[v], rays) for v in runs}, answers_bit_equal=bool(equal))
    for v in ("views_aov_host", "views_aov_device"):
        res[v + "_over_render_aov_loop"] = round(res["runs"]["render_aov_loop"]["wall_median_s"] / res["runs"][v]["wall_median_s"], 2)
    if stride == 1:
        res["views_aov_host_over_views_aov_host_parent"] = round(
            res["runs"]["views_aov_host_parent"]["wall_median_s"] / res["runs"]["views_aov_host"]["wall_median_s"], 2)
    base.close()
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", type=int, nargs=2, default=[480, 270])
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--scenes", nargs="+", default=["fractal_spheres", "cornell"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name in args.scenes:
        scene, camera, _ = getattr(scenes, name)()
        for n_views in args.views:
            for stride in (0, 1, "seeds"):
                res = bench(name, scene, camera, args.size[0], args.size[1], args.spp, n_views, stride, args.parent_lib, dev)
                if not res["answers_bit_equal"]:
                    bad.append("%s, %d views, stride %s: the answers differ" % (name, n_views, stride))
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
