"""Views per second of rptgpu_render_views_device against the loop a caller writes without it: one
rptgpu_render_batch_device per view — through another build of the library with --parent-lib (the parent commit's: a kept
copy, or scripts/build_variant.sh on that commit), else through this one.

Workloads: 16 and 64 perspective views (a 4x4 and an 8x8 light field: the scene's camera moved sideways and up in steps
of 2 % of its distance from the origin) of scenes.fractal_spheres and scenes.cornell at 480x270, 8 bounces, 4 spp, every
view with the same seed, frames in device memory — and the same batch with a seed per view: seed_stride = 1 on this build
(`batched_stride`: the seed travels with the path, pieces span views) beside the same call on the --parent-lib build
(`batched_stride_parent`: every view a piece of its own there, nothing shared between views), and seeds that are no
arithmetic sequence through rptgpu_render_views_seeded_device (`batched_seeds`).  The loop is timed on both routes a render
offers: the library's own choice (flags 0: the persistent kernel for the Cornell box) and RPT_FLAG_WAVEFRONT.  After two
warm-up calls of each kind, five alternating repeats of host wall time around the synchronous calls: median, min and max,
and views per second from the median.  All frames must be bit-equal between the variants (the batches with a seed per view:
to the loop with the same seeds), and finite: the script exits with status 1 after writing its lines when they are not.  No
threshold: the figures are recorded as they come.

Then one 2048x1024 panorama of scenes.wine_glass at 16 spp beside rptgpu_trace_rays_device on as many rays made by the
caller (the texel centres' directions, made with torch), both under RPT_FLAG_PROFILE_KERNELS: wall, the summed kernel_ms
of RptStats, and the bytes per pixel that cross the ABI either way.

    python scripts/views_bench.py [--parent-lib LIB] [--views 16 64] [--skip-panorama] [--out profiles/views_bench.json]
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

from rpt_amd import Camera, GpuScene, View, _abi, make_params, scenes  # noqa: E402

SEED = 0x52505447
REPEATS = 5
W, H, BOUNCES, SPP = 480, 270, 8, 4
DEVICE_KINDS = (_abi.RPT_K_RAYGEN, _abi.RPT_K_EXTEND, _abi.RPT_K_SHADE, _abi.RPT_K_SHADOW, _abi.RPT_K_RESOLVE)


class RawScene:
    """What the loop needs, bound on ANY build of the library (an older one lacks symbols that _abi.load_library
    insists on)."""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        self.lib.rptgpu_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.rptgpu_render_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self.lib.rptgpu_render_views_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self.lib.rptgpu_scene_destroy.argtypes = [C.c_void_p]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def render_device(self, cam, p, d_ptr):
        rc = self.lib.rptgpu_render_batch_device(self.h, C.byref(cam), C.byref(p), C.c_void_p(d_ptr), 0, None)
        if rc != 0:
            raise RuntimeError("rptgpu_render_batch_device: %d" % rc)

    def render_views_device(self, n, views, q, d_ptr):
        rc = self.lib.rptgpu_render_views_device(self.h, n, views, C.byref(q), C.c_void_p(d_ptr), 0, None)
        if rc != 0:
            raise RuntimeError("rptgpu_render_views_device: %d" % rc)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def light_field(camera, n):
    """n = k x k cameras: the scene's, moved on a grid across its own image plane"""
    k = int(round(math.sqrt(n)))
    assert k * k == n
    eye, direction, up = (np.array([float(c) for c in v]) for v in (camera.eye, camera.direction, camera.up))
    right = np.cross(direction, up)
    right /= np.linalg.norm(right)
    step = 0.02 * float(np.linalg.norm(eye))
    return [Camera(tuple(eye + (i - 0.5 * (k - 1)) * step * right + (j - 0.5 * (k - 1)) * step * up), camera.direction,
                   camera.up, camera.fov, 0.0, 0.0) for j in range(k) for i in range(k)]


def scattered_seeds(n):
    """n seeds that are no arithmetic sequence: SplitMix64's outputs from SEED on"""
    out, x, mask = [], SEED, (1 << 64) - 1
    for _ in range(n):
        x = (x + 0x9E3779B97F4A7C15) & mask
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        out.append(z ^ (z >> 31))
    return out


def summary(wall, n_views):
    med = float(np.median(wall))
    return dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(med, 5), wall_min_s=round(min(wall), 5),
                wall_max_s=round(max(wall), 5), views_per_s=round(n_views / med, 1))


def alternate(runs):
    for f in runs.values():  # warm-up: code objects, workspace, the record ratio of this max_bounces
        f()
        f()
    wall = {v: [] for v in runs}
    extra = {v: [] for v in runs}
    for _ in range(REPEATS):
        for v, f in runs.items():
            t0 = time.perf_counter()
            x = f()
            wall[v].append(time.perf_counter() - t0)
            extra[v].append(x)
    return wall, extra


def bench_views(name, scene, camera, n_views, parent_lib, dev):
    import torch
    cams = light_field(camera, n_views)
    lowered = [c.lower() for c in cams]
    g = GpuScene(scene, 0)
    loop = RawScene(parent_lib or _abi.LIB_PATH, scene)
    frames = {v: torch.zeros((n_views, H, W, 3), dtype=torch.float64, device=dev) for v in ("batched", "looped", "looped_wavefront")}

    def batched():
        g.render_views(cams, W, H, BOUNCES, samples=SPP, seed=SEED, out=frames["batched"])

    def looped(flags, key):
        p = make_params(W, H, BOUNCES, SPP, seed=SEED, flags=flags)
        out = frames[key]
        for v, cam in enumerate(lowered):
            loop.render_device(cam, p, out[v].data_ptr())

    # every view with a seed of its own: seed_stride = 1 on this build, where the seed travels with the path and the views
    # share their launches, beside the same call on the loop's build (the parent's: each view a piece of its own), and seeds
    # that are no arithmetic sequence — measured beside the others, checked against the loop with the same seeds (rendered
    # once, untimed)
    for v in ("batched_stride", "batched_stride_parent", "batched_seeds"):
        frames[v] = torch.zeros_like(frames["batched"])
    seeds = scattered_seeds(n_views)
    arr = GpuScene._lower_views(cams, "views_bench")
    q = _abi.RptViewQuery()
    q.struct_size, q.width, q.height, q.max_bounces, q.iterations = C.sizeof(_abi.RptViewQuery), W, H, BOUNCES, SPP
    q.seed, q.seed_stride, q.precision_mode = SEED, 1, _abi.RPT_PRECISION_F64_STRICT

    def batched_stride():
        g.render_views(cams, W, H, BOUNCES, samples=SPP, seed=SEED, seed_stride=1, out=frames["batched_stride"])

    def batched_stride_parent():
        loop.render_views_device(n_views, arr, q, frames["batched_stride_parent"].data_ptr())

    def batched_seeds():
        g.render_views(cams, W, H, BOUNCES, samples=SPP, seeds=seeds, out=frames["batched_seeds"])

    runs = {"batched": batched, "batched_stride": batched_stride, "batched_stride_parent": batched_stride_parent,
            "batched_seeds": batched_seeds, "looped": lambda: looped(0, "looped"),
            "looped_wavefront": lambda: looped(_abi.RPT_FLAG_WAVEFRONT, "looped_wavefront")}
    wall, _ = alternate(runs)
    equal = bool(torch.equal(frames["batched"], frames["looped"]) and torch.equal(frames["batched"], frames["looped_wavefront"]))
    want = torch.zeros_like(frames["batched"])
    for v, cam in enumerate(lowered):
        loop.render_device(cam, make_params(W, H, BOUNCES, SPP, seed=SEED + v), want[v].data_ptr())
    equal = equal and bool(torch.equal(frames["batched_stride"], want) and torch.equal(frames["batched_stride_parent"], want))
    for v, cam in enumerate(lowered):
        loop.render_device(cam, make_params(W, H, BOUNCES, SPP, seed=seeds[v]), want[v].data_ptr())
    equal = equal and bool(torch.equal(frames["batched_seeds"], want))
    res = dict(bench="views", scene=name, views=n_views, width=W, height=H, spp=SPP, max_bounces=BOUNCES, repeats=REPEATS,
               loop_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               views_piece=os.environ.get("RPTGPU_VIEWS_PIECE", "default"),
               runs={v: summary(wall[v], n_views) for v in runs}, frames_bit_equal=equal,
               finite=bool(torch.isfinite(frames["batched"]).all().item()))
    for v in ("looped", "looped_wavefront"):
        res["batched_over_" + v] = round(res["runs"]["batched"]["views_per_s"] / res["runs"][v]["views_per_s"], 3)
        res["batched_stride_over_" + v] = round(res["runs"]["batched_stride"]["views_per_s"] / res["runs"][v]["views_per_s"], 3)
    vps = {v: res["runs"][v]["views_per_s"] for v in runs}
    res["batched_stride_over_batched_stride_parent"] = round(vps["batched_stride"] / vps["batched_stride_parent"], 3)
    res["batched_stride_over_batched"] = round(vps["batched_stride"] / vps["batched"], 3)
    res["batched_seeds_over_batched"] = round(vps["batched_seeds"] / vps["batched"], 3)
    loop.close()
    g.close()
    return res


def bench_panorama(dev, pw=2048, ph=1024, spp=16):
    import torch
    scene, camera, cfg = scenes.wine_glass()
    bounces = cfg["max_bounces"]
    g = GpuScene(scene, 0)
    eye = tuple(float(c) for c in camera.eye)
    flags = _abi.RPT_FLAG_PROFILE_KERNELS
    pano = torch.zeros((1, ph, pw, 3), dtype=torch.float64, device=dev)
    # the caller's rays: the texel centres' directions in the panorama's convention
    f64 = dict(dtype=torch.float64, device=dev)
    az = (torch.arange(pw, **f64) / (pw - 1) - 0.5) * (2.0 * math.pi)
    el = (0.5 - torch.arange(ph, **f64) / (ph - 1)) * math.pi
    d = torch.stack([torch.cos(el)[:, None] * torch.cos(az)[None, :], torch.sin(el)[:, None].expand(ph, pw),
                     torch.cos(el)[:, None] * torch.sin(az)[None, :]], dim=2).reshape(-1, 3).contiguous()
    o = torch.tensor(eye, **f64).expand(pw * ph, 3).contiguous()
    ids = torch.arange(pw * ph, dtype=torch.int32, device=dev)
    out = torch.zeros((pw * ph, 3), dtype=torch.float64, device=dev)

    def device_ms():
        s = g.stats()
        return sum(s.kernel_ms[k] for k in DEVICE_KINDS)

    def views():
        g.reset_stats()
        g.render_views([View.panorama(eye)], pw, ph, bounces, samples=spp, seed=SEED, flags=flags, out=pano)
        return device_ms()

    def rays():
        g.reset_stats()
        g.trace_rays(o, d, bounces, samples=spp, seed=SEED, streams=ids, first_draw=2, flags=flags, out=out)
        return device_ms()

    wall, dev_ms = alternate({"render_views_device": views, "trace_rays_device": rays})
    res = dict(bench="views_panorama", scene="wine_glass", width=pw, height=ph, spp=spp, max_bounces=bounces, repeats=REPEATS,
               gpu=torch.cuda.get_device_name(0), finite=bool(torch.isfinite(pano).all().item()),
               bytes_per_pixel=dict(render_views_device={"in": round(C.sizeof(_abi.RptView) / float(pw * ph), 6), "out": 24},
                                    trace_rays_device={"in": 52, "out": 24}),
               runs={})
    for v in wall:
        ms = dev_ms[v]
        res["runs"][v] = dict(wall_median_s=round(float(np.median(wall[v])), 5), wall_min_s=round(min(wall[v]), 5),
                              wall_max_s=round(max(wall[v]), 5), device_ms=[round(t, 3) for t in ms],
                              device_median_ms=round(float(np.median(ms)), 3), device_min_ms=round(min(ms), 3),
                              device_max_ms=round(max(ms), 3))
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--skip-panorama", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name, make in (("fractal_spheres", scenes.fractal_spheres), ("cornell", scenes.cornell)):
        scene, camera, _ = make()
        for n in args.views:
            res = bench_views(name, scene, camera, n, args.parent_lib, dev)
            if not (res["frames_bit_equal"] and res["finite"]):
                bad.append("%s, %d views: frames_bit_equal=%s finite=%s" % (name, n, res["frames_bit_equal"], res["finite"]))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if not args.skip_panorama:
        res = bench_panorama(dev)
        if not res["finite"]:
            bad.append("panorama: finite=False")
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:  # the variants must render the same frames: a profile of differing ones is not a measurement
        print("views_bench: " + "; ".join(bad), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
