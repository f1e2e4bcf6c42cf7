"""Wall time of rptgpu_bake_ao_device and rptgpu_occluded_device against what a caller did before they
existed: the same rays through rptgpu_closest_hit — host arrays, every ray's closest hit with its normal and object — and a
numpy compare of t.  The baseline runs through another build of the library with --parent-lib (the parent commit's: a kept
copy, or scripts/build_variant.sh on that commit), else through this one.

Workloads: the C3 mesh (scenes.dragon), scenes.fractal_spheres and scenes.cornell.  One point per pixel of a 1920x1080
frame: the first hit of sample 0 and its normal from rptgpu_render_aov, lifted off the surface by 1e-6 of the camera's
distance along the normal (the header's advice); a pixel that sees nothing stands at the camera, facing back along its
direction.  S = 16 directions per point, unbounded (max_distance = +inf).
  (a) bake_ao_device  positions and normals in device memory -> the unoccluded fraction per point
  (b) occluded_device the same n x S rays, in device memory, without max_t -> one byte per ray, folded with torch
  (c) closest_hit     the same rays from host memory -> t per ray (and the normal and object nobody asked for), `t > DBL_MAX`
                      and the fold in numpy
The rays of (b) and (c) are made ONCE, outside the timed region, and are exactly (a)'s: direction k of every point is read
back from the library itself — bake_ao with samples = 1, sample_index_base = k and max_distance = -1 (never occluded)
returns bent = d_k / 1.0 — so the three answers must agree in every bit, and the script exits with status 1 after writing its
lines when they do not.  After one warm-up of each, five alternating repeats of host wall time around the synchronous calls:
median, min and max, M rays/s from the median, and the bytes per ray that cross the ABI either way.  No threshold: the
figures are recorded as they come.

    python scripts/occlusion_bench.py [--parent-lib LIB] [--size 1920 1080] [--samples 16] [--scenes dragon fractal_spheres cornell]
                                      [--out profiles/occlusion_bench.json]
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

from rpt_amd import GpuScene, _abi, make_params, scenes  # noqa: E402

SEED = 0x52505447
REPEATS = 5
DBL_MAX = 1.7976931348623157e308
PD = C.POINTER(C.c_double)


class RawScene:
    """rptgpu_closest_hit bound on ANY build of the library (an older one lacks symbols that _abi.load_library insists on)"""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        self.lib.rptgpu_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.rptgpu_closest_hit.argtypes = [C.c_void_p, C.c_uint64, PD, PD, C.c_uint32, PD, PD, C.POINTER(C.c_int32)]
        self.lib.rptgpu_scene_destroy.argtypes = [C.c_void_p]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def closest_hit(self, o, d, t, nrm, obj):
        rc = self.lib.rptgpu_closest_hit(self.h, len(o), o.ctypes.data_as(PD), d.ctypes.data_as(PD), 0, t.ctypes.data_as(PD),
                                         nrm.ctypes.data_as(PD), obj.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            raise RuntimeError("rptgpu_closest_hit: %d" % rc)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def points_of(g, camera, width, height):
    """one point and normal per pixel: sample 0's first hit, lifted off its surface"""
    aov = g.render_aov(camera, make_params(width, height, 0, 1, seed=SEED), _abi.RPT_AOV_POSITION | _abi.RPT_AOV_NORMAL)
    hit = aov["hits"].reshape(-1) > 0
    eye = np.array([float(c) for c in camera.eye])
    back = -np.array([float(c) for c in camera.direction])
    back /= np.linalg.norm(back)
    nrm = np.where(hit[:, None], aov["normal"].reshape(-1, 3), back[None, :])
    pos = np.where(hit[:, None], aov["position"].reshape(-1, 3), eye[None, :])
    pos = pos + nrm * (1e-6 * float(np.linalg.norm(eye)))
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm), float(hit.mean())


def summary(wall, n_rays):
    med = float(np.median(wall))
    return dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(med, 5), wall_min_s=round(min(wall), 5),
                wall_max_s=round(max(wall), 5), mrays_per_s=round(n_rays / med / 1e6, 1))


def bench(name, scene, camera, width, height, S, parent_lib, dev):
    import torch
    g = GpuScene(scene, 0)
    base = RawScene(parent_lib or _abi.LIB_PATH, scene)
    pos, nrm, hit_share = points_of(g, camera, width, height)
    n = len(pos)
    d_pos, d_nrm = torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev)
    # the rays, once: direction k of every point from the library itself (see above), [n][S][3]
    d_dirs = torch.empty((n, S, 3), dtype=torch.float64, device=dev)
    ao1, bent1 = torch.empty(n, dtype=torch.float64, device=dev), torch.empty((n, 3), dtype=torch.float64, device=dev)
    for k in range(S):
        g.bake_ao(d_pos, d_nrm, samples=1, seed=SEED, sample_index_base=k, max_distance=-1.0, bent_normals=True, out=(ao1, bent1))
        d_dirs[:, k] = bent1
    d_o = d_pos[:, None, :].expand(n, S, 3).reshape(-1, 3).contiguous()
    d_d = d_dirs.reshape(-1, 3)
    h_o, h_d = d_o.cpu().numpy(), d_d.cpu().numpy()
    torch.cuda.synchronize(dev)
    out_ao = torch.empty(n, dtype=torch.float64, device=dev)
    out_occ = torch.empty(n * S, dtype=torch.uint8, device=dev)
    t, hn, obj = np.empty(n * S), np.empty((n * S, 3)), np.empty(n * S, dtype=np.int32)
    answers = {}

    def bake_ao_device():
        g.bake_ao(d_pos, d_nrm, samples=S, seed=SEED, out=out_ao)
        answers["bake_ao_device"] = out_ao

    def occluded_device():
        g.occluded(d_o, d_d, out=out_occ)
        answers["occluded_device"] = (1 - out_occ.reshape(n, S).to(torch.int32)).sum(dim=1).to(torch.float64) / float(S)
        torch.cuda.synchronize(dev)

    def closest_hit_host():
        base.closest_hit(h_o, h_d, t, hn, obj)
        answers["closest_hit_host"] = (t > DBL_MAX).reshape(n, S).sum(axis=1).astype(np.float64) / float(S)

    runs = {"bake_ao_device": bake_ao_device, "occluded_device": occluded_device, "closest_hit_host": closest_hit_host}
    for f in runs.values():  # warm-up: code objects, workspace, staging arrays
        f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):
        for v, f in runs.items():
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    a = answers["bake_ao_device"].cpu().numpy()
    equal = bool(a.tobytes() == answers["occluded_device"].cpu().numpy().tobytes() and a.tobytes() == answers["closest_hit_host"].tobytes())
    res = dict(bench="occlusion", scene=name, width=width, height=height, points=n, samples=S, rays=n * S, repeats=REPEATS,
               baseline_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               pixels_with_a_hit=round(hit_share, 4), mean_ao=round(float(a.mean()), 6),
               runs={v: summary(wall[v], n * S) for v in runs}, answers_bit_equal=equal,
               bytes_per_ray={"bake_ao_device": {"in": round(48.0 / S, 3), "out": round(8.0 / S, 3)},
                              "occluded_device": {"in": 48, "out": 1}, "closest_hit_host": {"in": 48, "out": 36}})
    for v in ("bake_ao_device", "occluded_device"):
        res[v + "_over_closest_hit_host"] = round(res["runs"][v]["mrays_per_s"] / res["runs"]["closest_hit_host"]["mrays_per_s"], 2)
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
            bad.append("%s: the three answers differ" % name)
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
