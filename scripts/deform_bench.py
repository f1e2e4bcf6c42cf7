"""A deforming mesh through one scene handle: frames/s and the per-frame hand-off of GpuScene.set_mesh — from a numpy
array and from a torch tensor on the device — against a new GpuScene per frame, in one process on device 0.  Every
frame of the three loops must be bit-equal.  Prints one JSON line and writes it to --out.

Workload: the C3 scene with its knot stand-in (100 352 triangles), its vertices displaced by a sine that moves with the
frame, 20 frames, 480x270, 8 bounces, 4 spp.  What is timed per frame: the hand-off (set_mesh, or GpuScene() of the
frame's scene and the close of the last one) and the render with the frame in host memory.  The deformation itself (numpy,
and the copy of the frame's triangles to the device for the torch loop) is not timed: it stands for the caller's producer.

The hand-off's split (triangle records, boxes to the host, kd build, copies, leaf records, tree and object records) comes
from a child process that runs three updates with RPTGPU_PRINT_UPDATE=1 — the library then synchronises after every step
and prints its time — and reports the last one.

Usage: python scripts/deform_bench.py [--frames 20] [--out profiles/deform_bench.json]
"""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpt_amd import GpuScene, Mesh, make_params, scenes  # noqa: E402

SIZE = (480, 270, 8, 4)


def deformed(knot, frame):
    out = knot.copy()
    v = knot[:, :9].reshape(-1, 3).copy()
    v[:, 1] += 0.02 * np.sin(25.0 * v[:, 0] + 0.4 * frame) * np.cos(19.0 * v[:, 2])
    out[:, :9] = v.reshape(-1, 9)
    return out


def scene_of(tris):
    shape = Mesh(tris).scale((3.4, 3.4, 3.4)).rotate_y(math.pi / 2.0)
    scene, cam, _ = scenes.dragon(shape=shape)
    return scene, cam


def run(frames, how):
    """how: 'new' | 'numpy' | 'torch' -> (hand-off ms per frame, render ms per frame, total s, images)"""
    W, H, B, spp = SIZE
    p = make_params(W, H, B, spp, seed=0x4445)
    hand, render, images = [], [], []
    g, t_all = None, 0.0
    if how == "torch":
        import torch
    for tris in frames:
        scene, cam = scene_of(tris)
        src = tris
        if how == "torch" and g is not None:
            src = torch.from_numpy(tris).to("cuda:0")
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        if how != "new" and g is not None:
            g.set_mesh(0, src)
        else:
            if g is not None:
                g.close()
            g = GpuScene(scene, 0)
        t1 = time.perf_counter()
        img = g.render_batch(cam, p)
        t2 = time.perf_counter()
        hand.append((t1 - t0) * 1e3)
        render.append((t2 - t1) * 1e3)
        t_all += t2 - t0
        images.append(img)
    g.close()
    return hand, render, t_all, images


def median(v):
    return sorted(v)[len(v) // 2]


def split_child():
    knot = scenes.knot_mesh(784, 64)
    scene, _ = scene_of(knot)
    g = GpuScene(scene, 0)
    for f in range(1, 4):
        sys.stderr.write("update %d\n" % f)
        sys.stderr.flush()
        g.set_mesh(0, deformed(knot, f))
    g.close()


def handoff_split():
    env = dict(os.environ, RPTGPU_PRINT_UPDATE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-child"], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        return {"error": r.stderr[-500:]}
    last = r.stderr.split("update 3\n")[-1]
    return {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"scene_set_mesh (.+?)\s+([0-9.]+) ms", last)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_bench.json"))
    ap.add_argument("--split-child", action="store_true")
    a = ap.parse_args()
    if a.split_child:
        return split_child()
    # the first handle of a process pays HIP / module initialisation
    warm, cam, _ = scenes.simple_video(0)
    GpuScene(warm, 0).render_batch(cam, make_params(64, 48, 1, 1))
    knot = scenes.knot_mesh(784, 64)
    frames = [deformed(knot, f) for f in range(a.frames)]
    res = {how: run(frames, how) for how in ("new", "numpy", "torch")}
    equal = all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(res["new"][3], res["numpy"][3], res["torch"][3]))
    line = {"workload": "deform", "frames": a.frames, "frames_bit_equal": equal,
            "config": "C3 knot stand-in (%d triangles), sine displacement per frame: %dx%d, %d bounces, %d spp" % ((len(knot),) + SIZE)}
    for how, key in (("new", "new_handle"), ("numpy", "set_mesh_numpy"), ("torch", "set_mesh_torch")):
        hand, render, t_all, _ = res[how]
        # the first frame of every loop creates the handle: the hand-off of the others is what differs
        line["handoff_ms_median_" + key] = median(hand[1:])
        line["render_ms_median_" + key] = median(render[1:])
        line["frames_per_s_" + key] = a.frames / t_all
    line["handoff_ms_first"] = res["new"][0][0]
    line["handoff_split_ms"] = handoff_split()
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    if not equal:
        sys.exit("deform_bench: a frame through GpuScene.set_mesh differs from the new handle's")
    if not line["handoff_ms_median_set_mesh_numpy"] < line["handoff_ms_median_new_handle"]:
        sys.exit("deform_bench: the update hand-off is not below the new handle's")


if __name__ == "__main__":
    main()
