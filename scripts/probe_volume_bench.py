"""Wall time of rptgpu_lookup_probe_volume_device against what a caller writes today — first_hits_device and the
same rule as torch operations on the device — and against its floor, first_hits_device alone, both in the parent commit's
build (--parent-lib; else this one's, and the line says so).

The workload: the 1920x1080 pinhole rays of the camera of the C3 mesh (scenes.dragon) and of scenes.cornell, through pixel
centres, in device memory (2.07 M rays), and a --grid^3 volume (32) of random coefficients over the hits' bounding box, every
probe valid.
  (a) lookup_probe_volume_device, VALUE | COVERED
  (b) first_hits_device (OBJECT | NORMAL | POSITION) + the rule as torch operations   --parent-lib's build
  (c) first_hits_device (OBJECT | NORMAL | POSITION) alone, the floor                 --parent-lib's build
The sides run in one process, alternating: after two warm-ups of each, five repeats of host wall time around the synchronous
calls: median, min and max.  (b) multiplies and adds in the header's order, but torch may contract: the line reports the
largest difference to (a) over the covered rays and does not gate on it.  The one gate: the call on a crop — every 506th ray —
must equal tests/probe_volume_model.py over first_hits' own output in every bit; the script exits with status 1 after writing
its lines when it does not.  No threshold otherwise: the figures are recorded as they come.  bytes_lower_bound is what a ray
must move at the least — 48 B of ray, 52 B of hit record read, 25 B written, and for a covered ray 8 x 216 B of coefficients —
over the kernel's share of the call ((a) minus (c)), against the 8 TB/s HBM peak: a lower bound on the achieved rate, the
coefficients mostly coming from cache.

The second measurement, per scene: --views views (16) of 480x270 at 4 spp — the scene's camera moved sideways a step per view —
through render_views_probe_lit_device with the volume and one lightmap binding, beside render_views_lightmapped_device of
--parent-lib's build with the same binding: what the volume's term costs a view; the same protocol, and a crop gate of its own:
4 096 pixels of view 0 spread over the frame equal, in every bit, tests/views_model.py's rays through first_hits, hit_surface,
tests/lightmap_lookup_model.py and tests/probe_volume_model.py, folded by hand.

The lookup kernel's share of the call by the profiler is a run of its own, never combined with counters:
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/probe_volume_bench.py --scenes cornell --profile-run
(--profile-run: ten calls of (a) on one scene and nothing else; the share is rpt_probe_volume_lookup's time over the sum of the
call's kernels in OUT's kernel stats).

    python scripts/probe_volume_bench.py [--parent-lib LIB] [--grid 32] [--frame 1920 1080] [--scenes dragon cornell]
                                         [--out profiles/probe_volume_bench.json]
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

from rpt_amd import GpuScene, ProbeVolume, _abi, lightmap, scenes  # noqa: E402
from hit_surface_bench import open_scene, pinhole_rays  # noqa: E402
from lightmap_bench import summary  # noqa: E402
from lightmap_lookup_bench import workload as lightmap_workload  # noqa: E402

REPEATS, WARMUPS = 5, 2
HIT = _abi.RPT_HIT_OBJECT | _abi.RPT_HIT_NORMAL | _abi.RPT_HIT_POSITION
CROP = 4096
HBM_PEAK = 8.0e12
A = (3.141592653589793,) + (2.0943951023931953,) * 3 + (0.7853981633974483,) * 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def torch_rule(torch, hits, dirs, vol, coeffs, bias):
    """the header's rule for a volume whose probes are all valid, as torch operations -> (covered, value)"""
    n, P, obj = hits["normal"], hits["position"], hits["object"]
    dot = (n[:, 0] * dirs[:, 0] + n[:, 1] * dirs[:, 1]) + n[:, 2] * dirs[:, 2]
    N = torch.where((dot > 0.0)[:, None], -n, n)
    Q = P + bias * N
    nx, ny, nz = vol.counts
    C = coeffs.reshape(nx * ny * nz, 27)

    def cell(q, o, h, count):
        s = torch.clamp((q - o) / h, 0.0, float(count - 1))
        f0 = torch.floor(s)
        i0 = f0.long()
        return s - f0, i0, (i0 + 1).clamp(max=count - 1)

    fx, i0, i1 = cell(Q[:, 0], vol.origin[0], vol.spacing[0], nx)
    fy, j0, j1 = cell(Q[:, 1], vol.origin[1], vol.spacing[1], ny)
    fz, k0, k1 = cell(Q[:, 2], vol.origin[2], vol.spacing[2], nz)
    X, Y, Z, I, J, K = (1.0 - fx, fx), (1.0 - fy, fy), (1.0 - fz, fz), (i0, i1), (j0, j1), (k0, k1)
    S, ws = None, None
    for t in range(8):
        a, b, c = t & 1, (t >> 1) & 1, t >> 2
        w = (X[a] * Y[b]) * Z[c]
        term = w[:, None] * C[(K[c] * ny + J[b]) * nx + I[a]]
        S, ws = (term, w) if t == 0 else (S + term, ws + w)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    Yn = (torch.full_like(x, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
          1.0925484305920792 * (x * y), 1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0),
          1.0925484305920792 * (x * z), 0.5462742152960396 * (x * x - y * y))
    S = S.reshape(-1, 9, 3)
    M = None
    for j in range(9):
        term = (A[j] * Yn[j])[:, None] * S[:, j]
        M = term if j == 0 else M + term
    covered = (obj >= 0) & torch.isfinite(Q).all(dim=1) & torch.isfinite(N).all(dim=1) & (ws > 0.0)
    return covered, torch.where(covered[:, None], M / ws[:, None], torch.zeros_like(M))


def volume_for(g, o, d, grid):
    """a grid^3 volume of random coefficients over the bounding box of the rays' hits"""
    hits = g.first_hits(np.ascontiguousarray(o[::101]), np.ascontiguousarray(d[::101]), channels=HIT)
    P = hits["position"][hits["object"] >= 0]
    lo, hi = P.min(axis=0), P.max(axis=0)
    rs = np.random.RandomState(grid)
    coeffs = rs.uniform(-1.0, 1.0, (grid, grid, grid, 9, 3))
    coeffs[..., 0, :] += 4.0
    return ProbeVolume(lo, np.maximum(hi - lo, 1e-9) / (grid - 1), (grid, grid, grid), coeffs), 0.001 * float(np.linalg.norm(hi - lo))


def profile_run(name, args, dev):
    import torch
    scene, camera = scene_of(name)
    g = GpuScene(scene, 0)
    o, d = pinhole_rays(camera, *args.frame)
    vol, bias = volume_for(g, o, d, args.grid)
    d_o, d_d, d_c = (torch.from_numpy(a).to(dev) for a in (o, d, vol.coeffs))
    dvol = ProbeVolume(vol.origin, vol.spacing, vol.counts, d_c)
    for _ in range(10):
        g.lookup_probe_volume(d_o, d_d, dvol, normal_bias=bias, channels=_abi.RPT_VOLUME_VALUE | _abi.RPT_VOLUME_COVERED)
    g.close()


def scene_of(name):
    return scenes.dragon()[:2] if name == "dragon" else scenes.cornell()[:2]


def bench(name, args, dev):
    import torch
    import probe_volume_model as model
    width, height = args.frame
    scene, camera = scene_of(name)
    g = GpuScene(scene, 0)
    before = open_scene(args.parent_lib, scene) if args.parent_lib else g
    o, d = pinhole_rays(camera, width, height)
    N = len(o)
    vol, bias = volume_for(g, o, d, args.grid)
    d_o, d_d, d_c = (torch.from_numpy(a).to(dev) for a in (o, d, vol.coeffs))
    dvol = ProbeVolume(vol.origin, vol.spacing, vol.counts, d_c)
    torch.cuda.synchronize(dev)
    state = {}

    def this():
        state["this"] = g.lookup_probe_volume(d_o, d_d, dvol, normal_bias=bias, channels=_abi.RPT_VOLUME_VALUE | _abi.RPT_VOLUME_COVERED)

    def torch_ops():
        state["torch"] = torch_rule(torch, before.first_hits(d_o, d_d, channels=HIT), d_d, vol, d_c, bias)
        torch.cuda.synchronize(dev)

    def floor():
        state["floor"] = before.first_hits(d_o, d_d, channels=HIT)

    runs = {"lookup_probe_volume_device": this, "first_hits_device_plus_torch_ops": torch_ops, "first_hits_device": floor}
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
    # the gate: a crop of the rays through the host call, against the numpy model over first_hits' own output
    stride = max(1, N // CROP)
    oc, dc = np.ascontiguousarray(o[::stride]), np.ascontiguousarray(d[::stride])
    got = g.lookup_probe_volume(oc, dc, vol, normal_bias=bias)
    want = model.lookup(vol, dc, g.first_hits(oc, dc, channels=HIT | _abi.RPT_HIT_T), bias)
    equal = all(np.array_equal(bits(got[c]), bits(want[c])) for c in ("t", "object", "position", "normal", "value", "covered", "inside"))
    res = dict(bench="probe_volume", scene=name, width=width, height=height, rays=N, grid=[args.grid] * 3, channels="VALUE|COVERED",
               repeats=REPEATS, warmups=WARMUPS, before_library="parent" if args.parent_lib else "this",
               gpu=torch.cuda.get_device_name(0), rays_covered=round(float(covered.mean()), 4), runs={v: summary(wall[v]) for v in runs},
               covered_equal_to_torch=same_cover, max_difference_to_torch=diff, crop_rays=len(oc), crop_bit_equal_to_model=bool(equal))
    med = {v: res["runs"][v]["wall_median_s"] for v in runs}
    res["speedup_over_torch_ops"] = round(med["first_hits_device_plus_torch_ops"] / med["lookup_probe_volume_device"], 2)
    res["lookup_over_floor"] = round(med["lookup_probe_volume_device"] / med["first_hits_device"], 3)
    res["mrays_per_s"] = round(N / med["lookup_probe_volume_device"] / 1e6, 1)
    kernel_s = med["lookup_probe_volume_device"] - med["first_hits_device"]
    moved = N * (48 + 52 + 25) + int(covered.sum()) * 8 * 216
    res["kernel_share_s"] = round(kernel_s, 6)
    if kernel_s > 0:
        res["bytes_lower_bound_per_s"] = round(moved / kernel_s, 0)
        res["fraction_of_hbm_peak_lower_bound"] = round(moved / kernel_s / HBM_PEAK, 4)
    if before is not g:
        before.close()
    g.close()
    return res


def views_crop_equals_models(g, scene, camera, frame, binds, vol, bias, width, height, spp):
    """the views gate: view 0 (seed 7) restated by tests/views_model.py's rays, first_hits, hit_surface, tests/lightmap_lookup_model.py
    and tests/probe_volume_model.py, folded by hand; CROP pixels spread evenly over the frame must equal `frame`'s in every bit (a
    NaN equals a NaN)"""
    import lightmap_lookup_model as L
    import probe_volume_model as model
    import views_model
    from oracle import oracle_ffi
    oracle_ffi.lib()
    emit = np.array([ob._material.emittance for ob in scene.objects])
    pick = np.arange(0, width * height, max(1, width * height // CROP))
    samples = []
    for s in range(spp):
        o, d = (np.ascontiguousarray(a[pick]) for a in views_model.perspective_rays(oracle_ffi, camera, 7, width, height, s))
        hits = g.first_hits(o, d)
        surf = g.hit_surface(o, d)
        look = L.lookup(surf["object"], surf["primitive"], surf["barycentric"], binds, L.BILINEAR)
        pv = model.lookup(vol, d, hits, bias)
        covered, value, _ = model.irradiance(look["covered"], look["value"], pv["covered"], pv["value"])
        hit = hits["object"] >= 0
        env = np.zeros((len(pick), 3))
        if (~hit).any():
            env[~hit] = g.trace_rays(np.ascontiguousarray(o[~hit]), np.ascontiguousarray(d[~hit]), 0, samples=1, seed=1)
        samples.append(L.shade(hit, env, hits["albedo"], emit[np.maximum(hits["object"], 0)], covered, value, (0.0, 0.0, 0.0)))
    want, got = L.fold(samples, 0.0), frame.reshape(-1, 3)[pick]
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def bench_views(name, args, dev):
    import torch
    from rpt_amd import Camera
    width, height, spp = 480, 270, 4
    scene, camera, obj, uvs, tex = lightmap_workload(name, 2048)
    g = GpuScene(scene, 0)
    before = open_scene(args.parent_lib, scene) if args.parent_lib else g
    o, d = pinhole_rays(camera, 192, 108)
    vol, bias = volume_for(g, o, d, args.grid)
    eye, fwd, up = (np.array([float(c) for c in v]) for v in (camera.eye, camera.direction, camera.up))
    right = np.cross(fwd, up)
    step = 0.01 * float(np.linalg.norm(eye))
    views = [Camera(tuple(eye + (k - args.views / 2.0) * step * right), camera.direction, camera.up, camera.fov, 0.0, 0.0)
             for k in range(args.views)]
    binding = [lightmap.Binding(obj, torch.from_numpy(uvs).to(dev), torch.from_numpy(tex).to(dev))]
    dvol = ProbeVolume(vol.origin, vol.spacing, vol.counts, torch.from_numpy(vol.coeffs).to(dev))
    torch.cuda.synchronize(dev)
    state = {}

    def this():
        state["this"] = g.render_views_probe_lit(views, width, height, binding, dvol, samples=spp, seed=7, seed_stride=1, normal_bias=bias)

    def lightmapped():
        before.render_views_lightmapped(views, width, height, binding, samples=spp, seed=7, seed_stride=1)

    runs = {"render_views_probe_lit_device": this, "render_views_lightmapped_device": lightmapped}
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
    equal = views_crop_equals_models(g, scene, views[0], state["this"][0].cpu().numpy(), [lightmap.Binding(obj, uvs, tex)], vol, bias,
                                     width, height, spp)
    res = dict(bench="probe_volume_views", scene=name, views=args.views, width=width, height=height, spp=spp, grid=[args.grid] * 3,
               repeats=REPEATS, warmups=WARMUPS, before_library="parent" if args.parent_lib else "this",
               gpu=torch.cuda.get_device_name(0), runs={v: summary(wall[v]) for v in runs}, crop_pixels=CROP, crop_bit_equal_to_models=equal)
    med = {v: res["runs"][v]["wall_median_s"] for v in runs}
    res["probe_lit_over_lightmapped"] = round(med["render_views_probe_lit_device"] / med["render_views_lightmapped_device"], 3)
    res["views_per_s"] = round(args.views / med["render_views_probe_lit_device"], 1)
    if before is not g:
        before.close()
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--frame", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--scenes", nargs="+", default=["dragon", "cornell"], choices=["dragon", "cornell"])
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-run", action="store_true", help="ten calls of lookup_probe_volume_device on the first scene, for rocprofv3")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    if args.profile_run:
        profile_run(args.scenes[0], args, dev)
        return 0
    lines, ok = [], True
    for name in args.scenes:
        res = bench(name, args, dev)
        ok = ok and res["crop_bit_equal_to_model"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        res = bench_views(name, args, dev)
        ok = ok and res["crop_bit_equal_to_models"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
