"""Views per second of rptgpu_render_views_denoised against the loop a caller writes without it: per view a
device Buffer, four rptgpu_buffer_sample calls, rptgpu_buffer_features and rptgpu_buffer_denoise — through another build of
the library with --parent-lib (the parent commit's: a kept copy, or scripts/build_variant.sh on that commit), else through
this one.

Workloads (§15's protocol): 16 and 64 perspective views (scripts/views_bench.py's light fields) of scenes.fractal_spheres and
scenes.cornell at 480x270, 8 bounces, 4 batches of 4 spp, features from 4 spp, 3 levels, every view with a seed of its own
(seed + v).  The one call is timed in both forms — `device` (rptgpu_render_views_denoised_device into a torch tensor) and
`host` (into a numpy array) —, the loop on both routes a render offers: the library's own choice (flags 0: the persistent
kernel for the Cornell box) and RPT_FLAG_WAVEFRONT.  After two warm-up calls of each kind, five alternating repeats of host
wall time around the synchronous calls: median, min and max, and views per second from the median.  Every denoised frame
must be bit-equal between the variants, and finite: the script exits with status 1 after writing its lines when they are
not.  No threshold: the figures are recorded as they come, with the working set's bytes (rpt_amd/csrc/render_plan.h
views_denoise_plan's figures).

The filter kernels' own time comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o <scene>_<views> --output-format csv -- \\
        python scripts/views_denoised_bench.py --trace fractal_spheres 16
    python scripts/views_denoised_bench.py --merge-stats DIR --out profiles/views_denoised_bench.json

    python scripts/views_denoised_bench.py [--parent-lib LIB] [--views 16 64] [--out profiles/views_denoised_bench.json]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rpt_amd import GpuScene, _abi, make_params, scenes  # noqa: E402
from views_bench import light_field, summary  # noqa: E402

SEED = 0x52505447
REPEATS = 5
W, H, BOUNCES, SPP, BATCHES, FSPP, LEVELS = 480, 270, 8, 4, 4, 4, 3
SCENES = {"fractal_spheres": scenes.fractal_spheres, "cornell": scenes.cornell}
# bytes per (view, pixel) on the device: state, a batch's frame, feature sums, filter columns; a host caller's `denoised`
WORKING_SET = dict(state=60, staging=24, features=84, columns=145, host_denoised=24)


class BufferLoop:
    """The Buffer calls the loop needs, bound on ANY build of the library (an older one lacks symbols that
    _abi.load_library insists on)."""

    def __init__(self, path, scene):
        self.lib = lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        vp = C.c_void_p
        lib.rptgpu_scene_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
        lib.rptgpu_scene_destroy.argtypes = [vp]
        lib.rptgpu_scene_destroy.restype = None
        lib.rptgpu_buffer_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        lib.rptgpu_buffer_destroy.argtypes = [vp]
        lib.rptgpu_buffer_destroy.restype = None
        lib.rptgpu_buffer_sample.argtypes = [vp, vp, vp]
        lib.rptgpu_buffer_features.argtypes = [vp, vp, vp]
        lib.rptgpu_buffer_denoise.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        self.must(lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h)), "rptgpu_scene_create")

    @staticmethod
    def must(rc, what):
        if rc != 0:
            raise RuntimeError("%s: %d" % (what, rc))

    def view(self, cam, seed, flags, out):
        """one view as a caller gets it today -> its denoised frame in out (H, W, 3)"""
        lib, b = self.lib, C.c_void_p()
        self.must(lib.rptgpu_buffer_create(self.h, W, H, 0, C.byref(b)), "rptgpu_buffer_create")
        for k in range(BATCHES):
            p = make_params(W, H, BOUNCES, SPP, seed=seed, sample_index_base=k * SPP, flags=flags)
            self.must(lib.rptgpu_buffer_sample(b, C.byref(cam), C.byref(p)), "rptgpu_buffer_sample")
        p = make_params(W, H, BOUNCES, FSPP, seed=seed, flags=flags)
        self.must(lib.rptgpu_buffer_features(b, C.byref(cam), C.byref(p)), "rptgpu_buffer_features")
        d = _abi.RptDenoise(C.sizeof(_abi.RptDenoise), LEVELS, 2.0, 0.1, 0.01, 0.1)
        self.must(lib.rptgpu_buffer_denoise(b, C.byref(d), out.ctypes.data_as(C.POINTER(C.c_double)), None), "rptgpu_buffer_denoise")
        lib.rptgpu_buffer_destroy(b)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def one_call(g, cams, out):
    return g.render_views_denoised(cams, W, H, BOUNCES, SPP, BATCHES, seed=SEED, seed_stride=1, feature_samples=FSPP, levels=LEVELS,
                                   out={"denoised": out})


def bench(name, n_views, parent_lib, dev):
    import torch
    scene, camera, _ = SCENES[name]()
    cams = light_field(camera, n_views)
    lowered = [c.lower() for c in cams]
    g = GpuScene(scene, 0)
    loop = BufferLoop(parent_lib or _abi.LIB_PATH, scene)
    shape = (n_views, H, W, 3)
    frames = {"device": torch.zeros(shape, dtype=torch.float64, device=dev), "host": np.zeros(shape),
              "looped": np.zeros(shape), "looped_wavefront": np.zeros(shape)}

    def looped(flags, key):
        for v, cam in enumerate(lowered):
            loop.view(cam, SEED + v, flags, frames[key][v])

    runs = {"device": lambda: one_call(g, cams, frames["device"]), "host": lambda: one_call(g, cams, frames["host"]),
            "looped": lambda: looped(0, "looped"), "looped_wavefront": lambda: looped(_abi.RPT_FLAG_WAVEFRONT, "looped_wavefront")}
    for f in runs.values():  # warm-up: code objects, workspace, the record ratio of this max_bounces
        f()
        f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):
        for v, f in runs.items():
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    got = frames["device"].cpu().numpy()
    bits = lambda a: a.view(np.uint64)  # noqa: E731
    equal = all(np.array_equal(bits(got), bits(frames[v])) for v in ("host", "looped", "looped_wavefront"))
    n = n_views * W * H
    res = dict(bench="views_denoised", scene=name, views=n_views, width=W, height=H, spp_per_batch=SPP, batches=BATCHES,
               feature_spp=FSPP, levels=LEVELS, max_bounces=BOUNCES, repeats=REPEATS, loop_library="parent" if parent_lib else "this",
               gpu=torch.cuda.get_device_name(0), runs={v: summary(wall[v], n_views) for v in runs}, frames_bit_equal=bool(equal),
               finite=bool(np.isfinite(got).all()), working_set_bytes_per_pixel=WORKING_SET,
               working_set_bytes=dict(device=n * sum(v for k, v in WORKING_SET.items() if k != "host_denoised"),
                                      host=n * sum(WORKING_SET.values())))
    vps = {v: res["runs"][v]["views_per_s"] for v in runs}
    for v in ("looped", "looped_wavefront"):
        res["device_over_" + v] = round(vps["device"] / vps[v], 3)
        res["host_over_" + v] = round(vps["host"] / vps[v], 3)
    loop.close()
    g.close()
    return res


def trace(name, n_views):
    """what a kernel trace needs to see: one warm-up and one call"""
    import torch
    dev = torch.device("cuda", 0)
    scene, camera, _ = SCENES[name]()
    cams = light_field(camera, n_views)
    g = GpuScene(scene, 0)
    out = torch.zeros((n_views, H, W, 3), dtype=torch.float64, device=dev)
    for _ in range(2):
        one_call(g, cams, out)
    g.close()


def merge_stats(directory, out_path):
    """the filter's kernels (and the accumulation) of every <scene>_<views>_kernel_stats.csv into that workload's line"""
    lines = [json.loads(l) for l in open(out_path)] if os.path.exists(out_path) else []
    by_key = {"%s_%d" % (l["scene"], l["views"]): l for l in lines if l.get("bench") == "views_denoised"}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*_kernel_stats.csv"), recursive=True)):
        key = os.path.basename(path)[:-len("_kernel_stats.csv")]
        if key not in by_key:
            continue
        kernels, total = {}, 0.0
        for r in csv.DictReader(open(path)):
            total += float(r["TotalDurationNs"])
            if "rpt_denoise_views" in r["Name"] or "rpt_buffer_accumulate" in r["Name"]:
                short = r["Name"].split("(")[0].split("::")[-1]
                kernels[short] = dict(calls=int(r["Calls"]), total_ms=round(float(r["TotalDurationNs"]) / 1e6, 4),
                                      mean_ms=round(float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e6, 4))
        by_key[key]["kernel_trace"] = dict(calls_traced=2, kernels=kernels, all_kernels_ms=round(total / 1e6, 3),
                                           filter_share=round(sum(k["total_ms"] for n, k in kernels.items() if "denoise" in n) /
                                                              (total / 1e6), 5) if total else None)
    with open(out_path, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
            print(json.dumps(l))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--trace", nargs=2, metavar=("SCENE", "VIEWS"), default=None)
    ap.add_argument("--merge-stats", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out or os.path.join(ROOT, "profiles", "views_denoised_bench.json"))
        return 0
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    if args.trace:
        trace(args.trace[0], int(args.trace[1]))
        return 0
    lines, bad = [], []
    for name in SCENES:
        for n in args.views:
            res = bench(name, n, args.parent_lib, dev)
            if not (res["frames_bit_equal"] and res["finite"]):
                bad.append("%s, %d views: frames_bit_equal=%s finite=%s" % (name, n, res["frames_bit_equal"], res["finite"]))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:  # the variants must give the same frames: a profile of differing ones is not a measurement
        print("views_denoised_bench: " + "; ".join(bad), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
