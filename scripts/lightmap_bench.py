"""Wall time of rptgpu_bake_lightmap_device against what a caller had to do before it existed, through the
parent commit's build (--parent-lib; else this one's, and the line says so): rasterise the uv charts in numpy (the header's
rule, restricted to each triangle's box of texels — the whole map for a sliver), interpolate a gather point and a normal per owned texel, upload them,
rptgpu_bake_probes_device, scatter the results into an image and fill the gutters in numpy.

Workloads, both IRRADIANCE | OWNER at --samples and --bounces with --dilate rounds over a --size^2 map:
  atlas   the C3 mesh (scenes.dragon's knot, in world space) under a synthetic atlas made here: triangle j has its own cell
          of a square grid, its corners at three fixed points of the cell
  quad    one two-triangle chart over the whole map, on scenes.cornell's floor
Every array of the two sides must be equal in every bit; the script exits with status 1 after writing its lines when they are
not.  After two warm-ups of each side, five alternating repeats of host wall time around the synchronous calls: median, min
and max.  The baseline's time is split into its numpy half (raster, interpolation, scatter, dilation) and its device half (the
upload and the probe call).  No threshold: the figures are recorded as they come; a run that was not made is "not measured".

    python scripts/lightmap_bench.py [--parent-lib LIB] [--size 2048] [--samples 64] [--bounces 8] [--dilate 2]
                                     [--workloads atlas quad] [--out profiles/lightmap_bench.json]

--trace: two calls of this build's side per workload and nothing else — the process to profile for the rasteriser's and the
dilation's share of kernel time, in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python scripts/lightmap_bench.py --trace
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

from rpt_amd import GpuScene, _abi, scenes  # noqa: E402
from hit_surface_bench import open_scene  # noqa: E402

SEED = 0x52505447
REPEATS, WARMUPS = 5, 2
CHANNELS = _abi.RPT_LIGHTMAP_IRRADIANCE | _abi.RPT_LIGHTMAP_OWNER


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def edge(px, py, qx, qy, cx, cy):
    return (qx - px) * (cy - py) - (qy - py) * (cx - px)


def raster(uvs, width, height):
    """include/rpt_gpu_lightmap.h's owner rule and barycentrics in numpy -> (owner (H, W) int32, bary (H, W, 3)).  Triangles
    whose box of texels is at most 16 x 16 are tested together, padded to the largest of them; the others one by one."""
    n = len(uvs)
    ax, ay = uvs[:, :, 0] * float(width), uvs[:, :, 1] * float(height)
    with np.errstate(all="ignore"):
        area = edge(ax[:, 0], ay[:, 0], ax[:, 1], ay[:, 1], ax[:, 2], ay[:, 2])
        ok = np.isfinite(ax).all(axis=1) & np.isfinite(ay).all(axis=1) & np.isfinite(area) & (area != 0.0)
        x0 = np.clip(np.floor(np.where(ok, ax.min(axis=1), 0.0)) - 1.0, 0, width).astype(np.int64)
        x1 = np.clip(np.ceil(np.where(ok, ax.max(axis=1), 0.0)) + 1.0, 0, width).astype(np.int64)
        y0 = np.clip(np.floor(np.where(ok, ay.min(axis=1), 0.0)) - 1.0, 0, height).astype(np.int64)
        y1 = np.clip(np.ceil(np.where(ok, ay.max(axis=1), 0.0)) + 1.0, 0, height).astype(np.int64)
        # a sliver's rounded edge tests also pass along its line beyond its vertices: the whole map (lightmap_plan.h sliver)
        ex, ey = ax.max(axis=1) - ax.min(axis=1), ay.max(axis=1) - ay.min(axis=1)
        m = np.maximum(float(max(width, height)), np.maximum(np.abs(ax).max(axis=1), np.abs(ay).max(axis=1)))
        thin = ok & ~(np.abs(area) > 2.0 ** -46 * ((2.0 * m) * (ex + ey) * np.maximum(ex, ey) + ex * ey) + 2.0 ** -1000 * np.maximum(1.0, np.maximum(ex, ey)))
        x0, y0 = np.where(thin, 0, x0), np.where(thin, 0, y0)
        x1, y1 = np.where(thin, width, x1), np.where(thin, height, y1)
    owner = np.full(width * height, n, dtype=np.int64)
    small = ok & (x1 - x0 <= 16) & (y1 - y0 <= 16) & (x1 > x0) & (y1 > y0)

    def covered(j, xs, ys):
        cx, cy = xs + 0.5, ys + 0.5
        a = area[j]
        e1 = edge(ax[j, 1], ay[j, 1], ax[j, 2], ay[j, 2], cx, cy)
        e2 = edge(ax[j, 2], ay[j, 2], ax[j, 0], ay[j, 0], cx, cy)
        e3 = edge(ax[j, 0], ay[j, 0], ax[j, 1], ay[j, 1], cx, cy)
        return np.where(a > 0.0, (e1 >= 0.0) & (e2 >= 0.0) & (e3 >= 0.0), (e1 <= 0.0) & (e2 <= 0.0) & (e3 <= 0.0))

    js = np.flatnonzero(small)
    if len(js):
        bw, bh = int((x1 - x0)[js].max()), int((y1 - y0)[js].max())
        xs = (x0[js, None, None] + np.arange(bw)[None, None, :]).astype(np.float64)
        ys = (y0[js, None, None] + np.arange(bh)[None, :, None]).astype(np.float64)
        jj = js[:, None, None]
        inside = (xs < x1[jj]) & (ys < y1[jj])
        with np.errstate(all="ignore"):
            cov = covered(jj, xs, ys) & inside
        idx = (ys.astype(np.int64) * width + xs.astype(np.int64))
        idx, who = np.broadcast_to(idx, cov.shape)[cov], np.broadcast_to(jj, cov.shape)[cov]
        np.minimum.at(owner, idx, who)
    for j in np.flatnonzero(ok & ~small & (x1 > x0) & (y1 > y0)):
        xs = np.arange(x0[j], x1[j], dtype=np.float64)[None, :]
        ys = np.arange(y0[j], y1[j], dtype=np.float64)[:, None]
        with np.errstate(all="ignore"):
            cov = covered(j, xs, ys)
        view = owner.reshape(height, width)[y0[j]:y1[j], x0[j]:x1[j]]
        view[cov & (view > j)] = j
    owner = owner.reshape(height, width)
    owned = owner < n
    o = owner[owned]
    ys, xs = np.nonzero(owned)
    cx, cy = xs + 0.5, ys + 0.5
    bary = np.zeros((height, width, 3))
    with np.errstate(all="ignore"):
        bary[owned, 0] = edge(ax[o, 1], ay[o, 1], ax[o, 2], ay[o, 2], cx, cy) / area[o]
        bary[owned, 1] = edge(ax[o, 2], ay[o, 2], ax[o, 0], ay[o, 0], cx, cy) / area[o]
        bary[owned, 2] = edge(ax[o, 0], ay[o, 0], ax[o, 1], ay[o, 1], cx, cy) / area[o]
    return np.where(owned, owner, -1).astype(np.int32), bary


def gather_points(owner, bary, positions, offset):
    """-> (G (k, 3), n (k, 3)) of the owned texels in row-major order, flat normals (Triangle::from_vertices')"""
    owned = owner >= 0
    p = positions[owner[owned]]
    b1, b2, b3 = (bary[owned][:, k, None] for k in range(3))
    pos = (b1 * p[:, 0] + b2 * p[:, 1]) + b3 * p[:, 2]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    m = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    with np.errstate(all="ignore"):
        unit = m / np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])[:, None]
    return pos + offset * unit, unit


def dilate(values, filled, rounds):
    """the header's rounds over (H, W, 3) values"""
    h, w = filled.shape
    for _ in range(rounds):
        acc = np.zeros_like(values)
        count = np.zeros((h, w), dtype=np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nf = np.zeros((h, w), dtype=bool)
                nv = np.zeros_like(values)
                ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
                xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
                nf[yd, xd] = filled[ys, xs]
                nv[yd, xd] = values[ys, xs]
                acc = np.where(nf[:, :, None], acc + nv, acc)
                count += nf
        take = ~filled & (count > 0)
        with np.errstate(all="ignore"):
            values = np.where(take[:, :, None], acc / count.astype(np.float64)[:, :, None], values)
        filled = filled | take
    return values


def atlas(n, size):
    """triangle j in cell j of a square grid over the map: uvs (n, 3, 2), and the texels a cell is wide"""
    cells = int(np.ceil(np.sqrt(n)))
    cell = size // cells
    if cell < 2:
        raise SystemExit("lightmap_bench: a %d^2 map has no room for %d cells" % (size, n))
    j = np.arange(n)
    cx, cy = (j % cells) * cell, (j // cells) * cell
    corners = np.array([[0.25, 0.25], [cell - 0.25, 0.5], [0.5, cell - 0.25]])   # inside the cell, a texel's fraction off its border
    tex = np.stack([cx, cy], axis=1)[:, None, :] + corners[None, :, :]
    return tex / float(size), cell


def world_triangles(shape):
    """a placed Mesh's triangle positions in world space, (n, 3, 3)"""
    rows, m = shape.shape.triangles, np.asarray(shape.transform_m, dtype=np.float64).reshape(4, 4).T
    p = rows[:, :9].reshape(-1, 3)
    return np.ascontiguousarray((p @ m[:3, :3].T + m[:3, 3]).reshape(-1, 3, 3))


def summary(wall):
    med = float(np.median(wall))
    return dict(wall_s=[round(t, 5) for t in wall], wall_median_s=round(med, 5), wall_min_s=round(min(wall), 5),
                wall_max_s=round(max(wall), 5))


def bench(name, scene, positions, uvs, args, dev):
    import torch
    size, S, B, rounds = args.size, args.samples, args.bounces, args.dilate
    offset = 1e-4 * float(np.abs(positions).max())
    g = GpuScene(scene, 0)
    gp = open_scene(args.parent_lib, scene) if args.parent_lib else g
    t_pos, t_uvs = torch.from_numpy(positions).to(dev), torch.from_numpy(uvs).to(dev)
    state = {}

    def this():
        out = g.bake_lightmap(t_pos, t_uvs, size, size, samples=S, max_bounces=B, seed=SEED, offset=offset, dilate=rounds,
                              channels=CHANNELS)
        state["this"] = {k: v.cpu().numpy() for k, v in out.items()}
        return None

    def before():
        t0 = time.perf_counter()
        owner, bary = raster(uvs, size, size)
        pts, nrm = gather_points(owner, bary, positions, offset)
        owned = owner >= 0
        ids = np.flatnonzero(owned.ravel()).astype(np.uint32)
        t1 = time.perf_counter()
        res = gp.bake_probes(torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev), kind=_abi.RPT_PROBE_IRRADIANCE,
                             samples=S, max_bounces=B, seed=SEED, streams=torch.from_numpy(ids.astype(np.int64)).to(dev)).cpu().numpy()
        t2 = time.perf_counter()
        image = np.zeros((size, size, 3))
        image[owned] = res
        image = dilate(image, owned, rounds)
        t3 = time.perf_counter()
        state["before"] = {"irradiance": image, "owner": owner}
        return (t1 - t0) + (t3 - t2), t2 - t1

    if args.trace:
        this()
        this()
        g.close()
        return None
    runs = {"bake_lightmap_device": this, "numpy_raster_plus_bake_probes_device": before}
    for f in runs.values():
        for _ in range(WARMUPS):
            f()
    wall = {v: [] for v in runs}
    host_s, device_s = [], []
    for _ in range(REPEATS):  # alternating
        for v, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts = f()
            wall[v].append(time.perf_counter() - t0)
            if parts:
                host_s.append(parts[0])
                device_s.append(parts[1])
    a, b = state["this"], state["before"]
    equal = all(a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])) for k in ("irradiance", "owner"))
    owned = int((a["owner"] >= 0).sum())
    res = dict(bench="lightmap", workload=name, map=[size, size], triangles=int(len(uvs)), owned_texels=owned, samples=S, max_bounces=B,
               dilate=rounds, repeats=REPEATS, warmups=WARMUPS, gpu=torch.cuda.get_device_name(0),
               parent_lib=os.path.basename(args.parent_lib) if args.parent_lib else "not measured (the baseline ran on this build)",
               runs={v: summary(wall[v]) for v in runs}, baseline_numpy_median_s=round(float(np.median(host_s)), 5),
               baseline_upload_and_probes_median_s=round(float(np.median(device_s)), 5), bit_equal=bool(equal))
    res["speedup"] = round(res["runs"]["numpy_raster_plus_bake_probes_device"]["wall_median_s"] /
                           res["runs"]["bake_lightmap_device"]["wall_median_s"], 2)
    res["mpaths_per_s"] = round(owned * S / res["runs"]["bake_lightmap_device"]["wall_median_s"] / 1e6, 1)
    g.close()
    if gp is not g:
        gp.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["atlas", "quad"], choices=["atlas", "quad"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines, ok = [], True
    for name in args.workloads:
        if name == "atlas":
            scene = scenes.dragon()[0]
            positions = world_triangles(scene.objects[0].shape)
            uvs, _ = atlas(len(positions), args.size)
        else:
            scene = scenes.cornell()[0]
            positions = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 559.2], [556.0, 0.0, 559.2]],
                                  [[0.0, 0.0, 0.0], [556.0, 0.0, 559.2], [556.0, 0.0, 0.0]]])
            uvs = np.array([[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]])
        res = bench(name, scene, positions, np.ascontiguousarray(uvs, dtype=np.float64), args, dev)
        if res is None:
            continue
        ok = ok and res["bit_equal"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
