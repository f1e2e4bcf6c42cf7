"""Wall time of rptgpu_trace_vertices_device against its floor: rptgpu_trace_rays_device on the same rays —
the same paths with nothing exported — through another build of the library with --parent-lib (the parent commit's: a kept
copy, or scripts/build_variant.sh on that commit), else through this one.

The workload: the C3 mesh (scenes.dragon) and scenes.cornell, a 1920x1080 frame's camera rays through the pixel centres
(scripts/trace_rays_bench.py makes them on the device), streams = the pixel indices, first_draw = 2, 8 bounces, 4 samples per
ray; every array in device memory.
  (a) trace_vertices_device, all channels   152 B per vertex, 9 vertices per path, 4 B per path and 24 B per ray written
  (b) trace_vertices_device, LENGTH | RGB   4 B per path and 24 B per ray: the per-depth kernel stores nothing
  (c) trace_rays_device                     24 B per ray: the floor
The RGB of (a) and (b) must equal (c)'s in every bit, and the numpy fold of (a)'s channels must be that RGB on a sample of
the rays; the script exits with status 1 after writing its lines when they do not.  After one warm-up of each (two of the
first: a handle's first pass measures its record ratio), five alternating repeats of host wall time around the synchronous
calls: median, min and max, M paths/s from the median, the two ratios over the floor and the bytes written per path.  No
threshold: the figures are recorded as they come.

    python scripts/trace_vertices_bench.py [--parent-lib LIB] [--size 1920 1080] [--spp 4] [--bounces 8] [--scenes dragon cornell]
                                           [--out profiles/trace_vertices_bench.json]
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
from trace_rays_bench import pixel_centre_rays  # noqa: E402

SEED = 0x52505447
REPEATS = 5


class RawRays:
    """rptgpu_trace_rays_device bound on ANY build of the library (an older one lacks symbols that _abi.load_library insists on)"""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        self.lib.rptgpu_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.rptgpu_trace_rays_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.POINTER(_abi.RptRayQuery), C.c_void_p, C.c_void_p]
        self.lib.rptgpu_scene_destroy.argtypes = [C.c_void_p]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def trace(self, o, d, ids, bounces, spp, out):
        q = _abi.RptRayQuery()
        q.struct_size, q.max_bounces, q.iterations, q.first_draw, q.seed = C.sizeof(q), bounces, spp, 2, SEED
        rc = self.lib.rptgpu_trace_rays_device(self.h, o.shape[0], o.data_ptr(), d.data_ptr(), ids.data_ptr(), C.byref(q), out.data_ptr(), None)
        if rc != 0:
            raise RuntimeError("rptgpu_trace_rays_device: %d" % rc)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def summary(wall, paths):
    med = float(np.median(wall))
    return dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(med, 5), wall_min_s=round(min(wall), 5),
                wall_max_s=round(max(wall), 5), mpaths_per_s=round(paths / med / 1e6, 1))


def fold_rgb(v, rows, spp):
    """the header's fold over the exported channels of some rays, in numpy"""
    length = v.length[rows].cpu().numpy().view(np.uint32)
    A, f = v.radiance[rows].cpu().numpy(), v.bsdf[rows].cpu().numpy()
    inv_pdf, abs_cos = v.inv_pdf[rows].cpu().numpy(), v.abs_cos[rows].cpu().numpy()
    V = A.shape[2]
    L = np.zeros(A.shape[:2] + (3,))
    with np.errstate(all="ignore"):
        for d in range(V - 1, -1, -1):
            ind = (inv_pdf[:, :, d, None] * (f[:, :, d] * L)) * abs_cos[:, :, d, None]
            inner = (length - 1 > d)[:, :, None]
            last = (length - 1 == d)[:, :, None]
            L = np.where(inner, A[:, :, d] + np.fmin(ind, 100.0), np.where(last, A[:, :, d], L))
        acc = np.zeros((len(rows), 3))
        for s in range(spp):
            acc = acc + L[:, s]
    return acc / spp


def bench(name, scene, camera, W, H, bounces, spp, parent_lib, dev):
    import torch
    g = GpuScene(scene, 0)
    floor = RawRays(parent_lib or _abi.LIB_PATH, scene)
    o, d = pixel_centre_rays(camera, W, H, dev)
    n = o.shape[0]
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    rgb_floor = torch.empty((n, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    answers = {}
    kw = dict(samples=spp, seed=SEED, streams=ids, first_draw=2)

    def vertices_all():
        answers["vertices_all"] = None  # (the last answer's arrays are freed before the next ones are made)
        answers["vertices_all"] = g.trace_vertices(o, d, bounces, **kw)

    def vertices_length_rgb():
        answers["vertices_length_rgb"] = g.trace_vertices(o, d, bounces, channels=_abi.RPT_VERTEX_LENGTH | _abi.RPT_VERTEX_RGB, **kw)

    def trace_rays_floor():
        floor.trace(o, d, ids, bounces, spp, rgb_floor)

    runs = {"vertices_all": vertices_all, "vertices_length_rgb": vertices_length_rgb, "trace_rays_floor": trace_rays_floor}
    vertices_all()
    for f in runs.values():  # warm-up: code objects, workspace, the record ratio of this max_bounces
        f()
        f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    full, two = answers["vertices_all"], answers["vertices_length_rgb"]
    rows = torch.arange(0, n, max(1, n // 4096), device=dev)
    equal = bool(torch.equal(full.rgb, rgb_floor) and torch.equal(two.rgb, rgb_floor) and torch.equal(two.length, full.length))
    folded = bool(np.array_equal(fold_rgb(full, rows, spp), rgb_floor[rows].cpu().numpy()))
    paths = n * spp
    length = full.length.to(torch.float64)
    per_path = {"vertices_all": (bounces + 1) * 152 + 4 + 24.0 / spp, "vertices_length_rgb": 4 + 24.0 / spp, "trace_rays_floor": 24.0 / spp}
    res = dict(bench="trace_vertices", scene=name, width=W, height=H, rays=n, spp=spp, max_bounces=bounces, paths=paths, repeats=REPEATS,
               floor_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               mean_vertices_per_path=round(float(length.mean().item()), 3), runs={v: summary(wall[v], paths) for v in runs},
               rgb_bit_equal=equal, fold_bit_equal=folded, bytes_written_per_path={k: round(b, 1) for k, b in per_path.items()})
    for v in ("vertices_all", "vertices_length_rgb"):
        res[v + "_over_floor"] = round(res["runs"][v]["wall_median_s"] / res["runs"]["trace_rays_floor"]["wall_median_s"], 3)
    floor.close()
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--scenes", nargs="+", default=["dragon", "cornell"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name in args.scenes:
        scene, camera, _ = getattr(scenes, name)()
        res = bench(name, scene, camera, args.size[0], args.size[1], args.bounces, args.spp, args.parent_lib, dev)
        if not (res["rgb_bit_equal"] and res["fold_bit_equal"]):
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
