"""Wall time of rptgpu_trace_vertices_device under RPT_FLAG_VERTICES_PERSISTENT (the call's paths in the
persistent path kernel, rpt_paths_vertices, which writes each vertex where it makes it) beside
  the baseline  the same call without the flag (the wavefront pipeline and its two carry-out kernels) through another build of
                the library with --parent-lib (the parent commit's: a kept copy, or scripts/build_variant.sh on that commit),
                else through this one
  the floor     rptgpu_trace_rays_device under RPT_FLAG_RAYS_PERSISTENT of this build: the same paths in the same kernel
                loop with nothing exported
§19's protocol: scenes.cornell and scenes.glass, a 1920x1080 frame's camera rays through the pixel centres
(scripts/trace_rays_bench.py makes them on the device), streams = the pixel indices, first_draw = 2, 8 bounces, 4 samples per
ray, every array in device memory and allocated once; channel sets: all twelve channels (152 B per vertex, 9 vertices per
path) and LENGTH | RGB.  After two warm-ups of each, five alternating repeats of host wall time around the synchronous
calls: median, min and max.  The RGB of every run must be equal in every bit, the baseline's LENGTH the flagged call's, the
numpy fold of the flagged all-channel call's factors that RGB on 4 096 sampled rays, and the flagged call must have run
rpt_paths: the script exits with status 1 after writing its lines when they do not.  No threshold: the figures are recorded
as they come.

    python scripts/trace_vertices_persistent_bench.py [--parent-lib LIB] [--size 1920 1080] [--spp 4] [--bounces 8]
                                                      [--scenes cornell glass] [--out profiles/trace_vertices_persistent_bench.json]
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
from rpt_amd.device import PathVertices  # noqa: E402
from trace_rays_bench import pixel_centre_rays  # noqa: E402
from trace_vertices_bench import REPEATS, SEED, fold_rgb, summary  # noqa: E402

FLAG = _abi.RPT_FLAG_VERTICES_PERSISTENT
SETS = (("all", _abi.RPT_VERTEX_ALL), ("length_rgb", _abi.RPT_VERTEX_LENGTH | _abi.RPT_VERTEX_RGB))


class RawVertices:
    """rptgpu_trace_vertices_device bound on ANY build of the library (an older one lacks symbols that _abi.load_library insists
    on), writing into arrays that are allocated once"""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        VP = C.c_void_p
        self.lib.rptgpu_scene_create.argtypes = [VP, C.c_int, C.POINTER(VP)]
        self.lib.rptgpu_trace_vertices_device.argtypes = [VP, C.c_uint64, VP, VP, VP, VP, VP, VP]
        self.lib.rptgpu_scene_destroy.argtypes = [VP]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def trace(self, o, d, ids, bounces, spp, channels, flags, arrays):
        q = _abi.RptVertexQuery()
        q.struct_size, q.max_bounces, q.iterations, q.first_draw, q.seed = C.sizeof(q), bounces, spp, 2, SEED
        q.channels, q.flags = channels, flags
        rc = self.lib.rptgpu_trace_vertices_device(self.h, o.shape[0], o.data_ptr(), d.data_ptr(), ids.data_ptr(), C.byref(q),
                                                   C.byref(arrays), None)
        if rc != 0:
            raise RuntimeError("rptgpu_trace_vertices_device: %d" % rc)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def allocate(n, spp, bounces, channels, dev):
    """-> (a PathVertices of new device tensors for the named channels, the RptVertexArrays that points to them)"""
    import torch
    heads = {"path": (n, spp), "vertex": (n, spp, bounces + 1), "ray": (n,)}
    types = dict(_abi.RptVertexArrays._fields_)
    v = PathVertices(channels)
    a = _abi.RptVertexArrays()
    a.struct_size = C.sizeof(a)
    for bit, name, kind, tail, dtype in GpuScene._VERTEX_CHANNELS:
        if channels & bit:
            t = torch.empty(heads[kind] + tail, dtype=torch.float64 if dtype is np.float64 else torch.int32, device=dev)
            setattr(v, name, t)
            setattr(a, name, C.cast(C.c_void_p(t.data_ptr()), types[name]))
    return v, a


def bench(name, scene, camera, W, H, bounces, spp, set_name, channels, parent_lib, dev):
    import torch
    g = GpuScene(scene, 0)
    this = RawVertices(_abi.LIB_PATH, scene)
    base = RawVertices(parent_lib, scene) if parent_lib else this
    o, d = pixel_centre_rays(camera, W, H, dev)
    n = o.shape[0]
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    out = {k: allocate(n, spp, bounces, channels, dev) for k in ("flagged", "baseline_unflagged")}
    rgb_floor = torch.empty((n, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    runs = {"flagged": lambda: this.trace(o, d, ids, bounces, spp, channels, FLAG, out["flagged"][1]),
            "baseline_unflagged": lambda: base.trace(o, d, ids, bounces, spp, channels, 0, out["baseline_unflagged"][1]),
            "floor_flagged_trace_rays": lambda: g.trace_rays(o, d, bounces, samples=spp, seed=SEED, streams=ids, first_draw=2,
                                                             flags=_abi.RPT_FLAG_RAYS_PERSISTENT, out=rgb_floor)}
    # (the route of a flagged call, by the stats of a handle of the package's own)
    g.reset_stats()
    g.trace_vertices(o[:4096], d[:4096], bounces, channels=channels, samples=spp, seed=SEED, streams=ids[:4096], first_draw=2, flags=FLAG)
    st = g.stats()
    on_route = st.kernel_launches[_abi.RPT_K_PATHS] >= 1 and st.kernel_launches[_abi.RPT_K_RAYGEN] == 0
    for f in runs.values():  # warm-up: code objects, workspace, the record ratio of this max_bounces
        f()
        f()
    wall = {k: [] for k in runs}
    for _ in range(REPEATS):  # alternating
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            wall[k].append(time.perf_counter() - t0)
    full, want = out["flagged"][0], out["baseline_unflagged"][0]
    same = lambda x, y: bool(torch.equal(*(t.view(torch.int64) if t.dtype == torch.float64 else t for t in (x, y))))  # raw bits
    equal = same(full.rgb, rgb_floor) and same(want.rgb, rgb_floor) and same(want.length, full.length)
    folded = None
    if channels == _abi.RPT_VERTEX_ALL:
        rows = torch.arange(0, n, max(1, n // 4096), device=dev)
        folded = bool(np.array_equal(fold_rgb(full, rows, spp), rgb_floor[rows].cpu().numpy()))
        equal = equal and all(same(a, getattr(want, k)) for k, a in full.arrays().items())  # every channel, every byte
    paths = n * spp
    res = dict(bench="trace_vertices_persistent", scene=name, channels=set_name, width=W, height=H, rays=n, spp=spp, max_bounces=bounces,
               paths=paths, repeats=REPEATS, baseline_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               mean_vertices_per_path=round(float(full.length.to(torch.float64).mean().item()), 3),
               flagged_ran_rpt_paths=bool(on_route), runs={k: summary(wall[k], paths) for k in runs},
               results_bit_equal=equal, fold_bit_equal=folded, finite=bool(torch.isfinite(rgb_floor).all().item()))
    med = {k: res["runs"][k]["wall_median_s"] for k in runs}
    res["baseline_over_flagged"] = round(med["baseline_unflagged"] / med["flagged"], 3)  # > 1: the flagged route is faster
    res["flagged_over_floor"] = round(med["flagged"] / med["floor_flagged_trace_rays"], 3)
    res["baseline_over_floor"] = round(med["baseline_unflagged"] / med["floor_flagged_trace_rays"], 3)
    if base is not this:
        base.close()
    this.close()
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--scenes", nargs="+", default=["cornell", "glass"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name in args.scenes:
        scene, camera, _ = getattr(scenes, name)()
        for set_name, channels in SETS:
            res = bench(name, scene, camera, args.size[0], args.size[1], args.bounces, args.spp, set_name, channels, args.parent_lib, dev)
            ok = res["results_bit_equal"] and res["fold_bit_equal"] is not False and res["finite"] and res["flagged_ran_rpt_paths"]
            if not ok:
                bad.append("%s, %s: results_bit_equal=%s fold_bit_equal=%s finite=%s flagged_ran_rpt_paths=%s"
                           % (name, set_name, res["results_bit_equal"], res["fold_bit_equal"], res["finite"], res["flagged_ran_rpt_paths"]))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for b in bad:
        print("FAILED: " + b, file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
