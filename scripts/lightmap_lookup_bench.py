"""Wall time of rptgpu_lookup_lightmap_device against what a caller writes today — hit_surface_device and the
same rule as torch operations on the device — and against its floor, hit_surface_device alone, both in the parent commit's
build (--parent-lib; else this one's, and the line says so).

The workload: the 1920x1080 pinhole rays of the camera of the C3 mesh (scenes.dragon) and of scenes.cornell, through pixel
centres, in device memory (2.07 M rays), and a --size^2 map of 3 components with random texels and every texel valid, bound
to the mesh under lightmap_bench's synthetic atlas, and to cornell's back wall (the 16:9 frame does not see the floor) under one
two-triangle chart over the whole map.
  (a) lookup_lightmap_device, VALUE | COVERED, bilinear
  (b) hit_surface_device (OBJECT | PRIMITIVE | BARYCENTRIC) + the bilinear rule as torch operations   --parent-lib's build
  (c) hit_surface_device (OBJECT | PRIMITIVE | BARYCENTRIC) alone, the floor                           --parent-lib's build
The sides run in one process, alternating: after two warm-ups of each, five repeats of host wall time around the synchronous
calls: median, min and max.  (b) multiplies and adds in the header's order, but torch may contract: the line reports the
largest difference to (a) over the covered rays and does not gate on it.  The one gate: the call on a crop — every 506th ray, 4 099 rays
spread evenly over the frame — must equal tests/lightmap_lookup_model.py over the call's own hit_surface output in every bit;
the script exits with status 1 after writing its lines when it does not.  No threshold otherwise: the figures are recorded as they come.

The second measurement, per scene: --views views (16) of 480x270 at 4 spp — the scene's camera moved sideways a step per view —
through render_views_lightmapped_device with the same binding, beside render_views_device at 8 bounces in --parent-lib's
build: what a bake buys at view time, as a ratio; the same protocol, no gate of its own.  The torch side of the first
measurement leaves the valid mask out (every texel of the bench's map is valid), which favours it if anything.

    python scripts/lightmap_lookup_bench.py [--parent-lib LIB] [--size 2048] [--frame 1920 1080] [--scenes dragon cornell]
                                            [--out profiles/lightmap_lookup_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rpt_amd import GpuScene, _abi, lightmap, scenes  # noqa: E402
from hit_surface_bench import open_scene, pinhole_rays  # noqa: E402
from lightmap_bench import atlas, summary  # noqa: E402

REPEATS, WARMUPS = 5, 2
SURFACE = _abi.RPT_SURFACE_OBJECT | _abi.RPT_SURFACE_PRIMITIVE | _abi.RPT_SURFACE_BARYCENTRIC
CROP = 4096


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def torch_lookup(torch, surf, obj, uvs, tex):
    """the header's bilinear rule for one binding whose texels are all valid, as torch operations -> (covered, value)"""
    H, W = tex.shape[0], tex.shape[1]
    prim, bary = surf["primitive"], surf["barycentric"]
    bound = (surf["object"] == obj) & (prim >= 0)
    t = uvs[prim.clamp(min=0).long()]                                   # (n, 3, 2)
    uv = (bary[:, 0, None] * t[:, 0] + bary[:, 1, None] * t[:, 1]) + bary[:, 2, None] * t[:, 2]

    def axis(c, size):
        s = torch.clamp(c * float(size) - 0.5, -1.0, float(size))
        f0 = torch.floor(s)
        f = s - f0
        i0 = f0.long()
        return i0.clamp(0, size - 1), (i0 + 1).clamp(0, size - 1), f, 1.0 - f

    x0, x1, fx, gx = axis(uv[:, 0], W)
    y0, y1, fy, gy = axis(uv[:, 1], H)
    w00, w10, w01, w11 = gx * gy, fx * gy, gx * fy, fx * fy
    ws = ((w00 + w10) + w01) + w11
    value = (((w00[:, None] * tex[y0, x0] + w10[:, None] * tex[y0, x1]) + w01[:, None] * tex[y1, x0]) + w11[:, None] * tex[y1, x1]) / ws[:, None]
    covered = bound & torch.isfinite(uv).all(dim=1) & (ws > 0.0)
    return covered, torch.where(covered[:, None], value, torch.zeros_like(value))


def workload(name, size):
    rs = np.random.RandomState(size)
    if name == "dragon":
        scene, camera, _ = scenes.dragon()
        obj = 0
        uvs, _ = atlas(len(scene.objects[obj].shape.shape.triangles), size)
    else:
        scene, camera, _ = scenes.cornell()
        obj = 2   # the back wall
        uvs = np.array([[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]])
    return scene, camera, obj, np.ascontiguousarray(uvs, dtype=np.float64), rs.uniform(0.0, 4.0, (size, size, 3))


def bench(name, args, dev):
    import torch
    import lightmap_lookup_model as model
    width, height = args.frame
    scene, camera, obj, uvs, tex = workload(name, args.size)
    g = GpuScene(scene, 0)
    before = open_scene(args.parent_lib, scene) if args.parent_lib else g
    o, d = pinhole_rays(camera, width, height)
    N = len(o)
    d_o, d_d, d_uvs, d_tex = (torch.from_numpy(a).to(dev) for a in (o, d, uvs, tex))
    binding = [lightmap.Binding(obj, d_uvs, d_tex)]
    torch.cuda.synchronize(dev)
    state = {}

    def this():
        state["this"] = g.lookup_lightmap(d_o, d_d, binding, channels=_abi.RPT_LOOKUP_VALUE | _abi.RPT_LOOKUP_COVERED)

    def torch_ops():
        state["torch"] = torch_lookup(torch, before.hit_surface(d_o, d_d, channels=SURFACE), obj, d_uvs, d_tex)
        torch.cuda.synchronize(dev)

    def floor():
        state["floor"] = before.hit_surface(d_o, d_d, channels=SURFACE)

    runs = {"lookup_lightmap_device": this, "hit_surface_device_plus_torch_ops": torch_ops, "hit_surface_device": floor}
    for f in runs.values():
        for _ in range(WARMUPS):
            f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            wall[v].append(time.perf_counter() - t0)
    covered = state["this"]["covered"].cpu().numpy() != 0
    a, b = state["this"]["value"].cpu().numpy(), state["torch"][1].cpu().numpy()
    same_cover = bool(np.array_equal(covered, state["torch"][0].cpu().numpy()))
    diff = float(np.abs(a[covered] - b[covered]).max()) if covered.any() else 0.0
    # the gate: a crop of the rays through the host call, against the numpy model over the call's own hit_surface output
    stride = max(1, N // CROP)
    oc, dc = np.ascontiguousarray(o[::stride]), np.ascontiguousarray(d[::stride])
    k = len(oc)
    host = [lightmap.Binding(obj, uvs, tex)]
    got = g.lookup_lightmap(oc, dc, host)
    surf = g.hit_surface(oc, dc)
    want = model.lookup(surf["object"], surf["primitive"], surf["barycentric"], host, model.BILINEAR)
    equal = all(np.array_equal(bits(got[c]), bits(want[c])) for c in ("binding", "covered", "uv", "value"))
    res = dict(bench="lightmap_lookup", scene=name, width=width, height=height, rays=N, map=[args.size, args.size], components=3,
               filter="bilinear", channels="VALUE|COVERED", repeats=REPEATS, warmups=WARMUPS,
               before_library="parent" if args.parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               rays_covered=round(float(covered.mean()), 4), runs={v: summary(wall[v]) for v in runs},
               covered_equal_to_torch=same_cover, max_difference_to_torch=diff, crop_rays=k, crop_bit_equal_to_model=bool(equal),
               torch_side_reads_valid_mask=False)
    med = {v: res["runs"][v]["wall_median_s"] for v in runs}
    res["speedup_over_torch_ops"] = round(med["hit_surface_device_plus_torch_ops"] / med["lookup_lightmap_device"], 2)
    res["lookup_over_floor"] = round(med["lookup_lightmap_device"] / med["hit_surface_device"], 3)
    res["mrays_per_s"] = round(N / med["lookup_lightmap_device"] / 1e6, 1)
    if before is not g:
        before.close()
    g.close()
    return res


def bench_views(name, args, dev):
    import torch
    from rpt_amd import Camera
    width, height, spp, bounces = 480, 270, 4, 8
    scene, camera, obj, uvs, tex = workload(name, args.size)
    g = GpuScene(scene, 0)
    before = open_scene(args.parent_lib, scene) if args.parent_lib else g
    eye, fwd, up = (np.array([float(c) for c in v]) for v in (camera.eye, camera.direction, camera.up))
    right = np.cross(fwd, up)
    step = 0.01 * float(np.linalg.norm(eye))
    views = [Camera(tuple(eye + (k - args.views / 2.0) * step * right), camera.direction, camera.up, camera.fov, 0.0, 0.0)
             for k in range(args.views)]
    binding = [lightmap.Binding(obj, torch.from_numpy(uvs).to(dev), torch.from_numpy(tex).to(dev))]
    frames = torch.empty((args.views, height, width, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)

    def this():
        g.render_views_lightmapped(views, width, height, binding, samples=spp, seed=7, seed_stride=1)

    def path_traced():
        before.render_views(views, width, height, bounces, samples=spp, seed=7, seed_stride=1, out=frames)

    runs = {"render_views_lightmapped_device": this, "render_views_device_8_bounces": path_traced}
    for f in runs.values():
        for _ in range(WARMUPS):
            f()
    wall = {v: [] for v in runs}
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            wall[v].append(time.perf_counter() - t0)
    res = dict(bench="lightmap_lookup_views", scene=name, views=args.views, width=width, height=height, spp=spp, map=[args.size, args.size],
               filter="bilinear", path_traced_max_bounces=bounces, repeats=REPEATS, warmups=WARMUPS,
               before_library="parent" if args.parent_lib else "this", gpu=torch.cuda.get_device_name(0),
               runs={v: summary(wall[v]) for v in runs})
    med = {v: res["runs"][v]["wall_median_s"] for v in runs}
    res["path_traced_over_lightmapped"] = round(med["render_views_device_8_bounces"] / med["render_views_lightmapped_device"], 2)
    res["views_per_s"] = round(args.views / med["render_views_lightmapped_device"], 1)
    if before is not g:
        before.close()
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--frame", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--scenes", nargs="+", default=["dragon", "cornell"], choices=["dragon", "cornell"])
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    lines, ok = [], True
    for name in args.scenes:
        res = bench(name, args, dev)
        ok = ok and res["crop_bit_equal_to_model"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        lines.append(json.dumps(bench_views(name, args, dev)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
