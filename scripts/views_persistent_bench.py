"""Views per second of rptgpu_render_views_device under RPT_FLAG_VIEWS_PERSISTENT (the batch in the
persistent path kernel, rpt_paths_views) beside the same call without the flag (the wavefront pipeline) and beside the loop
a caller of flat scenes writes today: one rptgpu_render_batch_device per view on the library's own route — through another
build of the library with --parent-lib (the parent commit's: a kept copy, or scripts/build_variant.sh on that commit), else
through this one.  The protocol is scripts/views_bench.py's.

Workloads: 16 and 64 perspective views (views_bench.py's light field) of scenes.cornell (the fused flat kernel) and
scenes.glass (flat under an HDRI: the parked form) at 480x270, 8 bounces, 4 spp, frames in device memory; every view with
the same seed (`stride0`), seed_stride = 1 (`stride1`) and seeds that are no arithmetic sequence through
rptgpu_render_views_seeded_device (`seeds`).  After two warm-up calls of each kind, five alternating repeats of host wall
time around the synchronous calls: median, min and max, and views per second from the median.  All frames must be bit-equal
— flagged, unflagged and the loop with the same seeds — and finite: the script exits with status 1 after writing its lines
when they are not.  No threshold: the figures are recorded as they come.

    python scripts/views_persistent_bench.py [--parent-lib LIB] [--views 16 64] [--out profiles/views_persistent_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from rpt_amd import GpuScene, _abi, make_params, scenes  # noqa: E402

import views_bench as VB  # noqa: E402

W, H, BOUNCES, SPP, SEED = VB.W, VB.H, VB.BOUNCES, VB.SPP, VB.SEED
FLAG = _abi.RPT_FLAG_VIEWS_PERSISTENT


def bench(name, scene, camera, n_views, parent_lib, dev):
    import torch
    cams = VB.light_field(camera, n_views)
    lowered = [c.lower() for c in cams]
    g = GpuScene(scene, 0)
    loop = VB.RawScene(parent_lib or _abi.LIB_PATH, scene)
    seedings = {"stride0": dict(seed_stride=0), "stride1": dict(seed_stride=1), "seeds": dict(seeds=VB.scattered_seeds(n_views))}
    view_seeds = {"stride0": [SEED] * n_views, "stride1": [SEED + v for v in range(n_views)], "seeds": seedings["seeds"]["seeds"]}
    frames, runs = {}, {}

    def batched(key, flags, kw):
        def run():
            g.render_views(cams, W, H, BOUNCES, samples=SPP, seed=SEED, flags=flags, out=frames[key], **kw)
        return run

    def looped(key, seeds):
        def run():
            for v, cam in enumerate(lowered):
                loop.render_device(cam, make_params(W, H, BOUNCES, SPP, seed=seeds[v]), frames[key][v].data_ptr())
        return run

    for s, kw in seedings.items():
        for route, flags in (("persistent", FLAG), ("wavefront", 0)):
            key = "%s_%s" % (route, s)
            frames[key] = torch.zeros((n_views, H, W, 3), dtype=torch.float64, device=dev)
            runs[key] = batched(key, flags, kw)
        frames["looped_" + s] = torch.zeros((n_views, H, W, 3), dtype=torch.float64, device=dev)
        runs["looped_" + s] = looped("looped_" + s, view_seeds[s])
    g.reset_stats()
    runs["persistent_stride0"]()
    st = g.stats()
    on_route = st.kernel_launches[_abi.RPT_K_PATHS] >= 1 and st.kernel_launches[_abi.RPT_K_RAYGEN] == 0
    wall, _ = VB.alternate(runs)
    equal = all(bool(torch.equal(frames["persistent_" + s], frames["looped_" + s]) and
                     torch.equal(frames["wavefront_" + s], frames["looped_" + s])) for s in seedings)
    res = dict(bench="views_persistent", scene=name, views=n_views, width=W, height=H, spp=SPP, max_bounces=BOUNCES,
               repeats=VB.REPEATS, loop_library="parent" if parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               flagged_ran_rpt_paths_views=bool(on_route), runs={v: VB.summary(wall[v], n_views) for v in runs},
               frames_bit_equal=equal, finite=all(bool(torch.isfinite(f).all().item()) for f in frames.values()))
    vps = {v: res["runs"][v]["views_per_s"] for v in runs}
    for s in seedings:
        res["persistent_over_looped_" + s] = round(vps["persistent_" + s] / vps["looped_" + s], 3)
        res["persistent_over_wavefront_" + s] = round(vps["persistent_" + s] / vps["wavefront_" + s], 3)
        res["wavefront_over_looped_" + s] = round(vps["wavefront_" + s] / vps["looped_" + s], 3)
    loop.close()
    g.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)  # (the device is opened by torch first)
    lines, bad = [], []
    for name, make in (("cornell", scenes.cornell), ("glass", scenes.glass)):
        scene, camera, _ = make()
        for n in args.views:
            res = bench(name, scene, camera, n, args.parent_lib, dev)
            if not (res["frames_bit_equal"] and res["finite"] and res["flagged_ran_rpt_paths_views"]):
                bad.append("%s, %d views: frames_bit_equal=%s finite=%s flagged_ran_rpt_paths_views=%s"
                           % (name, n, res["frames_bit_equal"], res["finite"], res["flagged_ran_rpt_paths_views"]))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:  # the variants must render the same frames: a profile of differing ones is not a measurement
        print("views_persistent_bench: " + "; ".join(bad), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
