"""First-hit feature buffers (rptgpu_render_aov) against the cheapest call that traced the same camera rays
before they existed: rptgpu_render_batch_device with max_bounces = 0 at the same frame, seed and spp (it also evaluates
the lights and the BSDF at the hit, so it does strictly more device work).  C2 (cornell, 1920x1080, 16 spp) and the C5
mesh (wine_glass, 3840x2160, 4 spp), as rpt_amd/scenes.py defines them.

Wall times (the default mode): per scene, after a warm-up call of each shape, three alternating repeats of
  baseline      the 0-bounce render with this library — and, with --parent-lib, the same call through another build of
                the library (the parent commit's: scripts/build_variant.sh or a kept copy), whose frame must be bit-equal;
  aov_all       rptgpu_render_aov with every channel;
  aov_dn        ... with RPT_AOV_DEPTH | RPT_AOV_NORMAL only.
One JSON line per scene with each variant's three host wall times around the synchronous call, their median and their
spread (max - min: the margin of every comparison), and the bytes each channel set returns per pixel.

Kernel times: run ONE variant alone under the profiler, the program after `--`, no counters in that run,
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python scripts/aov_bench.py --scene S --trace V
(a warm-up call and one more call of the same shape), then
    python scripts/aov_bench.py --merge-stats DIR --out profiles/aov_bench.json
adds, per (scene, variant) found in DIR as <scene>_<variant>_kernel_stats.csv, the summed kernel time per call (the
total halved: both calls have the same shape) and the kernels that carry it.

    python scripts/aov_bench.py [--scene cornell|wine_glass] [--parent-lib PATH] [--out profiles/aov_bench.json]
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

from rpt_amd import GpuScene, _abi, _marshal, make_params, scenes  # noqa: E402

CONFIGS = {"cornell": 16, "wine_glass": 4}  # scene: spp
SEED = 0x52505447
REPEATS = 3
CHANNEL_SETS = {"aov_all": _abi.RPT_AOV_ALL, "aov_dn": _abi.RPT_AOV_DEPTH | _abi.RPT_AOV_NORMAL}
CHANNEL_BYTES = {bit: np.dtype(dtype).itemsize * (tail + (1,))[0] for bit, _, tail, dtype in _marshal.AOV_CHANNELS}


def bytes_per_pixel(channels):
    return 4 + sum(b for bit, b in CHANNEL_BYTES.items() if channels & bit)  # hits: always


class RawScene:
    """The three entry points the baseline needs, bound on ANY build of the library (an older one lacks symbols that
    _abi.load_library insists on)."""

    def __init__(self, path, scene):
        self.lib = C.CDLL(path)
        self.desc, self.keep = scene.lower()
        self.h = C.c_void_p()
        self.lib.rptgpu_scene_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.rptgpu_render_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self.lib.rptgpu_scene_destroy.argtypes = [C.c_void_p]
        self.lib.rptgpu_scene_destroy.restype = None
        rc = self.lib.rptgpu_scene_create(C.byref(self.desc), 0, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("rptgpu_scene_create (%s): %d" % (path, rc))

    def render_device(self, cam, p, d_ptr):
        rc = self.lib.rptgpu_render_batch_device(self.h, C.byref(cam), C.byref(p), C.c_void_p(d_ptr), 0, None)
        if rc != 0:
            raise RuntimeError("rptgpu_render_batch_device: %d" % rc)

    def close(self):
        self.lib.rptgpu_scene_destroy(self.h)


def stats(ts):
    return dict(wall_s=[round(t, 5) for t in ts], median_s=round(float(np.median(ts)), 5), spread_s=round(max(ts) - min(ts), 5))


def setup(name):
    import torch
    scene, camera, cfg = getattr(scenes, name)()
    W, H, spp = cfg["width"], cfg["height"], CONFIGS[name]
    frame = torch.empty(W * H * 3, dtype=torch.float64, device="cuda")
    return scene, camera.lower(), camera, W, H, spp, frame


def bench(name, parent_lib):
    scene, cam, camera, W, H, spp, frame = setup(name)
    p0 = make_params(W, H, 0, spp, seed=SEED)
    g = GpuScene(scene, 0)
    runs = {"baseline": lambda: g.render_batch_device(cam, p0, frame.data_ptr())}
    parent = None
    if parent_lib:
        parent = RawScene(parent_lib, scene)
        runs["baseline_parent"] = lambda: parent.render_device(cam, p0, frame.data_ptr())
    for v, ch in CHANNEL_SETS.items():
        runs[v] = (lambda ch=ch: g.render_aov(camera, p0, ch))
    frames = {}
    for v, f in runs.items():  # warm-up: code objects, workspace, host buffers
        f()
        if v.startswith("baseline"):
            frames[v] = frame.cpu().numpy().copy()
    times = {v: [] for v in runs}
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            t0 = time.perf_counter()
            f()
            times[v].append(time.perf_counter() - t0)
    out = dict(scene=name, width=W, height=H, spp=spp, repeats=REPEATS,
               bytes_per_pixel={v: bytes_per_pixel(ch) for v, ch in CHANNEL_SETS.items()},
               wall={v: stats(ts) for v, ts in times.items()})
    if parent:
        out["parent_frame_bit_equal"] = bool(frames["baseline"].tobytes() == frames["baseline_parent"].tobytes())
        parent.close()
    g.close()
    return out


def trace(name, variant):
    """a warm-up call and one more of one variant, for a profiler run"""
    scene, cam, camera, W, H, spp, frame = setup(name)
    p0 = make_params(W, H, 0, spp, seed=SEED)
    g = GpuScene(scene, 0)
    for _ in range(2):
        if variant == "baseline":
            g.render_batch_device(cam, p0, frame.data_ptr())
        else:
            g.render_aov(camera, p0, CHANNEL_SETS[variant])
    g.close()


def merge_stats(directory, out_path):
    lines = [json.loads(l) for l in open(out_path)] if os.path.exists(out_path) else []
    by_scene = {l["scene"]: l for l in lines if "scene" in l}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*_kernel_stats.csv"), recursive=True)):
        base = os.path.basename(path)[:-len("_kernel_stats.csv")]
        scene = next((s for s in CONFIGS if base.startswith(s + "_")), None)
        if scene is None:
            continue
        variant = base[len(scene) + 1:]
        rows = list(csv.DictReader(open(path)))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:6]
        entry = dict(kernel_ms_per_call=round(total / 2 / 1e6, 4), calls_traced=2,
                     top_kernels=[dict(name=r["Name"][:80], calls=int(r["Calls"]), ms_per_call=round(float(r["TotalDurationNs"]) / 2 / 1e6, 4))
                                  for r in top])
        by_scene.setdefault(scene, dict(scene=scene)).setdefault("kernel", {})[variant] = entry
    for l in by_scene.values():
        k = l.get("kernel", {})
        if "baseline" in k:
            spread_ms = 1e3 * l.get("wall", {}).get("baseline", {}).get("spread_s", 0.0)
            for v in CHANNEL_SETS:
                if v in k:
                    k[v]["minus_baseline_ms"] = round(k[v]["kernel_ms_per_call"] - k["baseline"]["kernel_ms_per_call"], 4)
                    k[v]["within_baseline_spread"] = bool(k[v]["minus_baseline_ms"] <= spread_ms)
            l["margin_ms_baseline_wall_spread"] = round(spread_ms, 4)
    with open(out_path, "w") as f:
        for l in by_scene.values():
            f.write(json.dumps(l) + "\n")
            print(json.dumps(l))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--parent-lib", default=None, help="another build of the library for the baseline's second leg")
    ap.add_argument("--trace", choices=["baseline"] + sorted(CHANNEL_SETS), default=None)
    ap.add_argument("--merge-stats", default=None, metavar="DIR")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (--merge-stats: rewrite it)")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out or os.path.join(ROOT, "profiles", "aov_bench.json"))
    names = [args.scene] if args.scene else ["cornell", "wine_glass"]
    if args.trace:
        for name in names:
            trace(name, args.trace)
        return
    for name in names:
        line = json.dumps(bench(name, args.parent_lib))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
