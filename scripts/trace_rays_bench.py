"""Throughput of rptgpu_trace_rays_device on the C3 mesh (scenes.dragon) at its frame size and 16 spp,
held against the render it shares every depth kernel with: rptgpu_render_batch_device of the same frame with
RPT_FLAG_WAVEFRONT — through this library and, with --parent-lib, through another build of it (the parent commit's:
a kept copy, or scripts/build_variant.sh on that commit).

The rays are the frame's camera rays through the pixel centres (one ray per pixel, made on the device with torch; every
one of a ray's 16 samples starts from it, where a render jitters each sample inside the pixel), streams = the pixel
indices, first_draw = 2.  After a warm-up call of each kind, five alternating repeats, each under
RPT_FLAG_PROFILE_KERNELS: host wall time around the synchronous call and the summed kernel_ms of RptStats (raygen,
extend, shade, shadow, resolve — the tree kinds are contained in extend and shadow).  One JSON line:
M ray-samples/s of the new call, both sets of numbers, and whether the new call's median device time lies within the
reference render's own min-max spread over its repeats — the margin is that measured spread and nothing more.
Wall time is recorded without a bound (--host adds the host entry point: 48 B per ray up, 24 B per ray down).

    python scripts/trace_rays_bench.py [--parent-lib LIB] [--spp 16] [--host] [--out profiles/trace_rays_bench.json]
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

from rpt_amd import GpuScene, _abi, make_params, scenes  # noqa: E402

SEED = 0x52505447
REPEATS = 5
DEVICE_KINDS = (_abi.RPT_K_RAYGEN, _abi.RPT_K_EXTEND, _abi.RPT_K_SHADE, _abi.RPT_K_SHADOW, _abi.RPT_K_RESOLVE)


class RawScene:
    """What the reference render needs, bound on ANY build of the library (an older one lacks symbols that
    _abi.load_library insists on)."""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        self.lib.rptgpu_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.rptgpu_render_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self.lib.rptgpu_get_stats.argtypes = [C.c_void_p, C.POINTER(_abi.RptStats)]
        self.lib.rptgpu_reset_stats.argtypes = [C.c_void_p]
        self.lib.rptgpu_scene_destroy.argtypes = [C.c_void_p]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def render_device(self, cam, p, d_ptr):
        rc = self.lib.rptgpu_render_batch_device(self.h, C.byref(cam), C.byref(p), C.c_void_p(d_ptr), 0, None)
        if rc != 0:
            raise RuntimeError("rptgpu_render_batch_device: %d" % rc)

    def device_ms(self):
        s = _abi.RptStats()
        self.lib.rptgpu_get_stats(self.h, C.byref(s))
        self.lib.rptgpu_reset_stats(self.h)
        return sum(s.kernel_ms[k] for k in DEVICE_KINDS)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def pixel_centre_rays(camera, W, H, dev):
    """renderer.rs:132-134 and Camera::cast_ray (camera.rs:64-81) without jitter and lens, as tensors on the device"""
    import torch
    f64 = dict(dtype=torch.float64, device=dev)
    direction, up = torch.tensor(list(camera.direction), **f64), torch.tensor(list(camera.up), **f64)
    right = torch.linalg.cross(direction, up)
    right = right / right.norm()
    dim = float(max(W, H))
    x = torch.arange(W, **f64)
    y = torch.arange(H, **f64)
    xn = ((2.0 * x + 1.0) - W) / dim
    yn = ((2.0 * (H - y) - 1.0) - H) / dim
    d = (1.0 / math.tan(camera.fov / 2.0)) * direction[None, None, :] + xn[None, :, None] * right[None, None, :] \
        + yn[:, None, None] * up[None, None, :]
    d = (d / d.norm(dim=2, keepdim=True)).reshape(-1, 3).contiguous()
    o = torch.tensor(list(camera.eye), **f64).expand(W * H, 3).contiguous()
    return o, d


def summary(wall, dev_ms):
    return dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(float(np.median(wall)), 5),
                device_ms=[round(t, 3) for t in dev_ms], device_median_ms=round(float(np.median(dev_ms)), 3),
                device_min_ms=round(min(dev_ms), 3), device_max_ms=round(max(dev_ms), 3))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--host", action="store_true", help="also time the host entry point (numpy arrays)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    scene, camera, cfg = scenes.dragon()
    W, H, bounces, spp = cfg["width"], cfg["height"], cfg["max_bounces"], args.spp
    dev = torch.device("cuda", 0)
    flags = _abi.RPT_FLAG_WAVEFRONT | _abi.RPT_FLAG_PROFILE_KERNELS
    p = make_params(W, H, bounces, spp, seed=SEED, flags=flags)
    cam = camera.lower()
    frame = torch.empty(W * H * 3, dtype=torch.float64, device=dev)
    o, d = pixel_centre_rays(camera, W, H, dev)
    ids = torch.arange(W * H, dtype=torch.int32, device=dev)
    out = torch.empty((W * H, 3), dtype=torch.float64, device=dev)
    g = GpuScene(scene, 0)
    raw = {"render": RawScene(_abi.LIB_PATH, scene)}
    if args.parent_lib:
        raw["render_parent"] = RawScene(args.parent_lib, scene)

    def trace_device():
        g.reset_stats()
        g.trace_rays(o, d, bounces, samples=spp, seed=SEED, streams=ids, first_draw=2, flags=flags, out=out)
        s = g.stats()
        return sum(s.kernel_ms[k] for k in DEVICE_KINDS)

    runs = {"trace_rays_device": trace_device}
    for name, r in raw.items():
        runs[name] = (lambda r=r: (r.render_device(cam, p, frame.data_ptr()), r.device_ms())[1])
    if args.host:
        ho, hd, hi = o.cpu().numpy(), d.cpu().numpy(), ids.cpu().numpy().astype(np.uint32)

        def trace_host():
            g.reset_stats()
            g.trace_rays(ho, hd, bounces, samples=spp, seed=SEED, streams=hi, first_draw=2, flags=flags)
            s = g.stats()
            return sum(s.kernel_ms[k] for k in DEVICE_KINDS)
        runs["trace_rays_host"] = trace_host
    for r in raw.values():
        r.device_ms()
    for f in runs.values():  # warm-up: code objects, workspace, the record ratio of this max_bounces
        f()
        f()
    wall = {v: [] for v in runs}
    dev_ms = {v: [] for v in runs}
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            t0 = time.perf_counter()
            ms = f()
            wall[v].append(time.perf_counter() - t0)
            dev_ms[v].append(ms)
    res = dict(bench="trace_rays", scene="dragon", width=W, height=H, spp=spp, max_bounces=bounces, rays=W * H, repeats=REPEATS,
               gpu=torch.cuda.get_device_name(0), runs={v: summary(wall[v], dev_ms[v]) for v in runs})
    res["mray_samples_per_s"] = round(W * H * spp / float(np.median(wall["trace_rays_device"])) / 1e6, 1)
    ref = "render_parent" if args.parent_lib else "render"
    lo, hi = min(dev_ms[ref]), max(dev_ms[ref])
    med = float(np.median(dev_ms["trace_rays_device"]))
    res["reference"] = ref
    res["device_ms_within_reference_spread"] = bool(lo <= med <= hi)
    res["finite"] = bool(torch.isfinite(out).all().item())
    for r in raw.values():
        r.close()
    g.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
