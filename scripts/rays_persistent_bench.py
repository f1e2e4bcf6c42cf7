"""Rays and probes per second of rptgpu_trace_rays_device and rptgpu_bake_probes_device under RPT_FLAG_RAYS_PERSISTENT
(the call's paths in the persistent path kernel, rpt_paths_rays) beside the same call without the
flag (the wavefront pipeline) and beside the unflagged call through another build of the library with --parent-lib (the
parent commit's: a kept copy, or scripts/build_variant.sh on that commit), the baseline.  The protocol is
scripts/views_persistent_bench.py's.

Workloads, on scenes.cornell (the fused flat kernel) and scenes.glass (flat under an HDRI: the parked form), arrays in
device memory:
  rays        the camera rays of a 1920x1080 frame (pixel centres, the pixel as stream id, first_draw 2), 8 bounces, 4 samples
  sh9         65 536 SH9 probes x 64 directions, 8 bounces, at positions drawn uniformly inside the scene's box
  irradiance  65 536 irradiance probes x 64 directions there, normals uniform on the sphere
After two warm-up calls of each kind, five alternating repeats of host wall time around the synchronous calls: median, min
and max, and paths per second from the median.  All results of a workload must be bit-equal — flagged, unflagged and the
parent's — and finite, and the flagged call must have run rpt_paths_rays: the script exits with status 1 after writing its
lines when they are not.  No threshold: the figures are recorded as they come.

    python scripts/rays_persistent_bench.py [--parent-lib LIB] [--out profiles/rays_persistent_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rpt_amd import GpuScene, _abi, scenes  # noqa: E402

import views_bench as VB  # noqa: E402

W, H, BOUNCES, SPP, SEED = 1920, 1080, 8, 4, VB.SEED
N_PROBES, PROBE_SAMPLES = 65536, 64
FLAG = _abi.RPT_FLAG_RAYS_PERSISTENT
# where the probes stand: inside the box of each scene (tests/test_gpu_probes.py's)
BOXES = {"cornell": ((20.0, 20.0, 20.0), (536.0, 528.0, 540.0)), "glass": ((-2.5, -1.5, -2.5), (2.5, 1.5, 2.5))}


class RawRays:
    """The two device entry points bound on ANY build of the library (an older one lacks symbols that _abi.load_library
    insists on for the package's own)."""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        VP = C.c_void_p
        self.lib.rptgpu_scene_create.argtypes = [VP, C.c_int, C.POINTER(VP)]
        self.lib.rptgpu_trace_rays_device.argtypes = [VP, C.c_uint64, VP, VP, VP, VP, VP, VP]
        self.lib.rptgpu_bake_probes_device.argtypes = [VP, C.c_uint64, VP, VP, VP, VP, VP, VP]
        self.lib.rptgpu_scene_destroy.argtypes = [VP]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def trace_rays(self, o, d, ids, q, out):
        rc = self.lib.rptgpu_trace_rays_device(self.h, o.shape[0], o.data_ptr(), d.data_ptr(), ids.data_ptr(), C.byref(q),
                                               out.data_ptr(), None)
        if rc != 0:
            raise RuntimeError("rptgpu_trace_rays_device: %d" % rc)

    def bake_probes(self, pos, nrm, q, out):
        rc = self.lib.rptgpu_bake_probes_device(self.h, pos.shape[0], pos.data_ptr(), nrm.data_ptr() if nrm is not None else None,
                                                None, C.byref(q), out.data_ptr(), None)
        if rc != 0:
            raise RuntimeError("rptgpu_bake_probes_device: %d" % rc)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def camera_rays(camera):
    """the rays of the pixel centres of a W x H frame of `camera` (renderer.rs:132-134 and camera.rs:64-81 without the jitter
    and the lens), in numpy: (origins, unit directions, the pixels as stream ids)"""
    eye, direction, up = (np.array([float(c) for c in v]) for v in (camera.eye, camera.direction, camera.up))
    right = np.cross(direction, up)
    right /= np.linalg.norm(right)
    dist = 1.0 / math.tan(camera.fov / 2.0)
    dim = float(max(W, H))
    y, x = np.divmod(np.arange(W * H), W)
    px = ((2 * x + 1) - W) / dim
    py = ((2 * (H - y) - 1) - H) / dim
    d = dist * direction[None, :] + px[:, None] * right[None, :] + py[:, None] * up[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(eye, (W * H, 1)), d, np.arange(W * H, dtype=np.uint32)


def summary(wall, n_paths):
    med = float(np.median(wall))
    return dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(med, 5), wall_min_s=round(min(wall), 5),
                wall_max_s=round(max(wall), 5), mpaths_per_s=round(n_paths / med / 1e6, 2))


def bench(name, scene, camera, workload, parent_lib, dev):
    import torch
    g = GpuScene(scene, 0)
    parent = RawRays(parent_lib, scene) if parent_lib else None
    keys = ["flagged", "unflagged"] + (["parent_unflagged"] if parent else [])
    if workload == "rays":
        o, d, ids = camera_rays(camera)
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        ti = torch.from_numpy(ids.astype(np.int32)).to(dev)
        n, iterations = W * H, SPP
        outs = {k: torch.zeros((n, 3), dtype=torch.float64, device=dev) for k in keys}
        kw = dict(samples=SPP, seed=SEED, streams=ti, first_draw=2)
        q = _abi.RptRayQuery()
        q.struct_size, q.max_bounces, q.iterations, q.first_draw, q.seed = C.sizeof(q), BOUNCES, SPP, 2, SEED
        runs = {"flagged": lambda: g.trace_rays(to, td, BOUNCES, flags=FLAG, out=outs["flagged"], **kw),
                "unflagged": lambda: g.trace_rays(to, td, BOUNCES, out=outs["unflagged"], **kw)}
        if parent:
            runs["parent_unflagged"] = lambda: parent.trace_rays(to, td, ti, q, outs["parent_unflagged"])
    else:
        kind = _abi.RPT_PROBE_SH9 if workload == "sh9" else _abi.RPT_PROBE_IRRADIANCE
        rs = np.random.RandomState(sum(map(ord, name + workload)))
        lo, hi = BOXES[name]
        pos = rs.uniform(lo, hi, (N_PROBES, 3))
        nrm = rs.standard_normal((N_PROBES, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        tp = torch.from_numpy(pos).to(dev)
        tn = torch.from_numpy(nrm).to(dev) if kind == _abi.RPT_PROBE_IRRADIANCE else None
        n, iterations = N_PROBES, PROBE_SAMPLES
        shape = (n, 9, 3) if kind == _abi.RPT_PROBE_SH9 else (n, 3)
        outs = {k: torch.zeros(shape, dtype=torch.float64, device=dev) for k in keys}
        kw = dict(kind=kind, samples=PROBE_SAMPLES, max_bounces=BOUNCES, seed=SEED)
        q = _abi.RptProbeQuery()
        q.struct_size, q.kind, q.samples, q.max_bounces, q.seed = C.sizeof(q), kind, PROBE_SAMPLES, BOUNCES, SEED
        runs = {"flagged": lambda: g.bake_probes(tp, tn, flags=FLAG, out=outs["flagged"], **kw),
                "unflagged": lambda: g.bake_probes(tp, tn, out=outs["unflagged"], **kw)}
        if parent:
            runs["parent_unflagged"] = lambda: parent.bake_probes(tp, tn, q, outs["parent_unflagged"])
    g.reset_stats()
    runs["flagged"]()
    st = g.stats()
    on_route = st.kernel_launches[_abi.RPT_K_PATHS] >= 1 and st.kernel_launches[_abi.RPT_K_RAYGEN] == 0
    wall, _ = VB.alternate(runs)
    equal = all(bool(torch.equal(outs["flagged"], outs[k])) for k in keys[1:])
    res = dict(bench="rays_persistent", scene=name, workload=workload, n=n, iterations=iterations, max_bounces=BOUNCES,
               repeats=VB.REPEATS, baseline_library="parent" if parent else None, gpu=torch.cuda.get_device_name(0),
               flagged_ran_rpt_paths_rays=bool(on_route), runs={k: summary(wall[k], n * iterations) for k in keys},
               results_bit_equal=equal, finite=all(bool(torch.isfinite(f).all().item()) for f in outs.values()))
    med = {k: res["runs"][k]["wall_median_s"] for k in keys}
    res["flagged_over_unflagged"] = round(med["unflagged"] / med["flagged"], 3)  # > 1: the flagged route is faster
    if parent:
        res["flagged_over_parent_unflagged"] = round(med["parent_unflagged"] / med["flagged"], 3)
        res["unflagged_over_parent_unflagged"] = round(med["parent_unflagged"] / med["unflagged"], 3)
        parent.close()
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--workloads", nargs="+", default=["rays", "sh9", "irradiance"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name, make in (("cornell", scenes.cornell), ("glass", scenes.glass)):
        scene, camera, _ = make()
        for workload in args.workloads:
            res = bench(name, scene, camera, workload, args.parent_lib, dev)
            if not (res["results_bit_equal"] and res["finite"] and res["flagged_ran_rpt_paths_rays"]):
                bad.append("%s, %s: results_bit_equal=%s finite=%s flagged_ran_rpt_paths_rays=%s"
                           % (name, workload, res["results_bit_equal"], res["finite"], res["flagged_ran_rpt_paths_rays"]))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:  # the routes must give the same results: a profile of differing ones is not a measurement
        print("rays_persistent_bench: " + "; ".join(bad), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
