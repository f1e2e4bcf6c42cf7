"""A group whose children move through one scene handle: frames/s and the per-frame hand-off of GpuScene.set_group — from
Python shapes and from a torch tensor of RptTransform records on the device — against a new GpuScene per frame, in one
process on device 0.  Every frame of the three loops must be bit-equal.  Prints one JSON line and writes it to --out.

Workload: fractal_spheres with its level-4 group (750 spheres) orbiting the centre sphere, 20 frames, 480x270, 8 bounces,
4 spp.  What is timed per frame: the hand-off (set_group — with the lowering of the shapes in the first loop — or
GpuScene() of the frame's scene and the close of the last one) and the render with the frame in host memory.  Making the
frame's shapes and records (and the copy of the records to the device for the torch loop) is not timed: it stands for the
caller's producer.

The hand-off's split (child records, boxes to the host, kd build, copies, leaf boxes, tree and object records) comes from
a child process that runs three updates with RPTGPU_PRINT_UPDATE=1 — the library then synchronises after every step and
prints its time — and reports the last one.

Usage: python scripts/group_update_bench.py [--frames 20] [--out profiles/group_update_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpt_amd import GpuScene, KdTree, Object, make_params, scenes, transform_records  # noqa: E402

SIZE = (480, 270, 8, 4)
GROUP = 4  # the object whose children move: the 750 spheres of the fractal's last level


def children_of(frame):
    """the level-4 spheres turned about the y axis through the centre sphere by 0.05 rad per frame"""
    scene, _, _ = scenes.fractal_spheres()
    kids = scene.objects[GROUP].shape.objects
    return kids if frame == 0 else [k.rotate_y(0.05 * frame) for k in kids]


def scene_of(children):
    scene, cam, _ = scenes.fractal_spheres()
    scene.objects[GROUP] = Object(KdTree(children)).material(scene.objects[GROUP]._material)
    return scene, cam


def run(frames, how):
    """how: 'new' | 'shapes' | 'torch' -> (hand-off ms per frame, render ms per frame, total s, images)"""
    W, H, B, spp = SIZE
    p = make_params(W, H, B, spp, seed=0x4752)
    hand, render, images = [], [], []
    g, t_all = None, 0.0
    if how == "torch":
        import torch
    for children in frames:
        scene, cam = scene_of(children)
        src = children
        if how == "torch" and g is not None:
            src = torch.from_numpy(transform_records(children)).to("cuda:0")
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        if how != "new" and g is not None:
            g.set_group(GROUP, src)
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
    scene, _ = scene_of(children_of(0))
    g = GpuScene(scene, 0)
    for f in range(1, 4):
        kids = children_of(f)
        sys.stderr.write("update %d\n" % f)
        sys.stderr.flush()
        g.set_group(GROUP, kids)
    g.close()


def handoff_split():
    env = dict(os.environ, RPTGPU_PRINT_UPDATE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-child"], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        return {"error": r.stderr[-500:]}
    last = r.stderr.split("update 3\n")[-1]
    return {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"scene_set_group (.+?)\s+([0-9.]+) ms", last)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_update_bench.json"))
    ap.add_argument("--split-child", action="store_true")
    a = ap.parse_args()
    if a.split_child:
        return split_child()
    # torch's device initialisation comes first: started after the library's first handle it has been seen to find no device
    import torch
    torch.cuda.init()
    # the first handle of a process pays HIP / module initialisation
    warm, cam, _ = scenes.simple_video(0)
    GpuScene(warm, 0).render_batch(cam, make_params(64, 48, 1, 1))
    frames = [children_of(f) for f in range(a.frames)]
    res = {how: run(frames, how) for how in ("new", "shapes", "torch")}
    equal = all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(res["new"][3], res["shapes"][3], res["torch"][3]))
    line = {"workload": "group_update", "frames": a.frames, "frames_bit_equal": equal,
            "config": "fractal_spheres, its level-4 group (%d spheres) orbiting: %dx%d, %d bounces, %d spp" % ((len(frames[0]),) + SIZE)}
    for how, key in (("new", "new_handle"), ("shapes", "set_group_shapes"), ("torch", "set_group_torch")):
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
        sys.exit("group_update_bench: a frame through GpuScene.set_group differs from the new handle's")


if __name__ == "__main__":
    main()
