"""Device time of rptgpu_bake_probes_device on the C3 mesh (scenes.dragon), held against what a caller
had to do before it existed: make n x S rays, send them through rptgpu_trace_rays_device and project the radiance with
torch on the device.

n probes stand at random points around the mesh (fixed seed), S directions each.  The baseline's directions come from
torch's generator — uniform on the sphere for SH9, cosine-weighted about the normal for IRRADIANCE — so the two sides
trace equally many, equally distributed rays but not the same ones; both results are checked finite, nothing more.
After a warm-up of each, five alternating repeats, each under RPT_FLAG_PROFILE_KERNELS: host wall time around the
synchronous call, the summed kernel_ms of RptStats (raygen, extend, shade, shadow, resolve) and, for the baseline, the
milliseconds of the torch projection between two events.  One JSON line per kind; no threshold is attached.

    python scripts/probes_bench.py [--probes 65536] [--samples 64] [--kind sh9|irradiance|both] [--out profiles/probes_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpt_amd import GpuScene, _abi, scenes  # noqa: E402

SEED = 0x52505447
REPEATS = 5
DEVICE_KINDS = (_abi.RPT_K_RAYGEN, _abi.RPT_K_EXTEND, _abi.RPT_K_SHADE, _abi.RPT_K_SHADOW, _abi.RPT_K_RESOLVE)
Y = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)


def sh9_basis_torch(d):
    import torch
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return torch.stack([torch.full_like(x, Y[0]), Y[1] * y, Y[1] * z, Y[1] * x, Y[2] * (x * y), Y[2] * (y * z),
                        Y[3] * (3.0 * (z * z) - 1.0), Y[2] * (x * z), Y[4] * (x * x - y * y)], dim=1)


def summary(wall, dev_ms, extra=None):
    s = dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(float(np.median(wall)), 5),
             device_ms=[round(t, 3) for t in dev_ms], device_median_ms=round(float(np.median(dev_ms)), 3),
             device_min_ms=round(min(dev_ms), 3), device_max_ms=round(max(dev_ms), 3))
    if extra is not None:
        s["projection_ms"] = [round(t, 3) for t in extra]
        s["projection_median_ms"] = round(float(np.median(extra)), 3)
    return s


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--kind", default="both", choices=["sh9", "irradiance", "both"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    scene, camera, cfg = scenes.dragon()
    n, S, bounces = args.probes, args.samples, cfg["max_bounces"]
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    lo, hi = torch.tensor([-3.0, -0.9, -3.0], **f64), torch.tensor([3.0, 3.0, 3.0], **f64)
    pos = lo + (hi - lo) * torch.rand((n, 3), generator=gen, **f64)
    nrm = torch.randn((n, 3), generator=gen, **f64)
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    flags = _abi.RPT_FLAG_PROFILE_KERNELS
    g = GpuScene(scene, 0)
    lines = []
    for kind_name in (["sh9", "irradiance"] if args.kind == "both" else [args.kind]):
        kind = _abi.RPT_PROBE_SH9 if kind_name == "sh9" else _abi.RPT_PROBE_IRRADIANCE
        width = 27 if kind == _abi.RPT_PROBE_SH9 else 3
        out = torch.empty((n, 9, 3) if width == 27 else (n, 3), **f64)
        rays_o = pos.repeat_interleave(S, dim=0).contiguous()
        L = torch.empty((n * S, 3), **f64)
        state = {}

        def bake():
            g.reset_stats()
            g.bake_probes(pos, nrm if width == 3 else None, kind=kind, samples=S, max_bounces=bounces, seed=SEED, flags=flags, out=out)
            s = g.stats()
            return sum(s.kernel_ms[k] for k in DEVICE_KINDS), None

        def rays_and_projection():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            v = torch.randn((n * S, 3), generator=gen, **f64)
            v = v / v.norm(dim=1, keepdim=True)
            if width == 3:  # cosine-weighted about the normal: a unit vector plus a uniform one, normalised
                v = v + nrm.repeat_interleave(S, dim=0)
                v = v / v.norm(dim=1, keepdim=True).clamp_min(1e-300)
            e1.record()
            g.reset_stats()
            g.trace_rays(rays_o, v, bounces, samples=1, seed=SEED, flags=flags, out=L)
            s = g.stats()
            e2, e3 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e2.record()
            if width == 27:
                res = torch.einsum("rj,rc->rjc", sh9_basis_torch(v), L).reshape(n, S, 9, 3).sum(dim=1) * (4.0 * np.pi / S)
            else:
                res = L.reshape(n, S, 3).sum(dim=1) * (np.pi / S)
            e3.record()
            torch.cuda.synchronize()
            state["res"] = res
            return sum(s.kernel_ms[k] for k in DEVICE_KINDS), e0.elapsed_time(e1) + e2.elapsed_time(e3)

        runs = {"bake_probes_device": bake, "trace_rays_device_plus_torch": rays_and_projection}
        for f in runs.values():  # warm-up: code objects, workspace, the record ratio of this max_bounces
            f()
            f()
        wall = {v: [] for v in runs}
        dev_ms = {v: [] for v in runs}
        proj = {v: [] for v in runs}
        for _ in range(REPEATS):  # alternating
            for v, f in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ms, extra = f()
                wall[v].append(time.perf_counter() - t0)
                dev_ms[v].append(ms)
                if extra is not None:
                    proj[v].append(extra)
        res = dict(bench="probes", kind=kind_name, scene="dragon", probes=n, samples=S, max_bounces=bounces, repeats=REPEATS,
                   gpu=torch.cuda.get_device_name(0),
                   bytes_in_per_probe=24 * (2 if width == 3 else 1), bytes_out_per_probe=8 * width,
                   baseline_bytes_per_probe=(48 + 24) * S,
                   runs={v: summary(wall[v], dev_ms[v], proj[v] or None) for v in runs})
        res["mpaths_per_s"] = round(n * S / float(np.median(wall["bake_probes_device"])) / 1e6, 1)
        res["finite"] = bool(torch.isfinite(out).all().item() and torch.isfinite(state["res"]).all().item())
        lines.append(json.dumps(res))
        print(lines[-1])
    g.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
