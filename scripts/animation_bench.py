"""Animation through one scene handle: frames/s and the per-frame hand-off (GpuScene.update against a new GpuScene) for
three frame loops, each run both ways on device 0.  Every frame of the update loop is checked bit-equal to the frame
of the rebuild loop.  Prints one JSON line per workload and writes them to --out.

  * simple_video: examples/simple_video.rs's 60 frames (800x600, 1 bounce, 100 spp: the cube slides away);
  * marbles: examples/marbles.rs's TEST branch (200x150, 7 bounces, 1 spp), the state integrated 1/16 s per frame on
    the GPU between frames (outside the timed loop);
  * dragon: the C3 scene with its knot stand-in (100 352 triangles) rotated about y per frame, at a reduced size.

What is timed per frame: the hand-off (GpuScene.update, or GpuScene() of the frame's scene and the close of the last
one) and the render with the frame in host memory.  The Python scene build is not timed.

Usage: python scripts/animation_bench.py [--only simple_video|marbles|dragon] [--out profiles/animation_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpt_amd import GpuScene, Mesh, make_params, scenes  # noqa: E402
from rpt_amd.ode import MarblesSystem  # noqa: E402


def frames_simple_video():
    for f in range(60):
        scene, cam, _ = scenes.simple_video(f)
        yield scene, cam


def frames_marbles(n=30):
    state = scenes.marbles_start()
    system = MarblesSystem(scenes.MARBLES_R)
    for _ in range(n):
        scene, cam, _ = scenes.marbles(state, test=True)
        yield scene, cam
        system.rk4_integrate(state, 1.0 / 16.0, 1.0 / 10000.0)


def frames_dragon(n=20):
    knot = scenes.knot_mesh(784, 64)  # one triangle array for every frame: the geometry is the same object
    for f in range(n):
        shape = Mesh(knot).scale((3.4, 3.4, 3.4)).rotate_y(math.pi / 2.0 + 0.05 * f)
        scene, cam, _ = scenes.dragon(shape=shape)
        yield scene, cam


WORKLOADS = {
    "simple_video": (frames_simple_video, (800, 600, 1, 100), "examples/simple_video.rs, 60 frames"),
    "marbles": (frames_marbles, (200, 150, 7, 1), "examples/marbles.rs TEST branch, 30 frames"),
    "dragon": (frames_dragon, (480, 270, 8, 4), "C3 knot stand-in rotated per frame, 20 frames"),
}


def run(frames, size, update):
    """-> (frames, per-frame hand-off ms, per-frame render ms, total s, images)"""
    W, H, B, spp = size
    hand, render, images = [], [], []
    g = None
    t_all = 0.0
    for scene, cam in frames():
        p = make_params(W, H, B, spp, seed=0x414E)
        t0 = time.perf_counter()
        if update and g is not None:
            g.update(scene)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "animation_bench.json"))
    a = ap.parse_args()
    # the first handle of a process pays HIP / module initialisation
    warm, cam, _ = scenes.simple_video(0)
    GpuScene(warm, 0).render_batch(cam, make_params(64, 48, 1, 1))
    lines = []
    for name in ([a.only] if a.only else sorted(WORKLOADS)):
        frames, size, what = WORKLOADS[name]
        h_new, r_new, t_new, img_new = run(frames, size, update=False)
        h_upd, r_upd, t_upd, img_upd = run(frames, size, update=True)
        equal = all(x.tobytes() == y.tobytes() for x, y in zip(img_new, img_upd))
        n = len(img_new)
        line = {"workload": name, "config": "%s: %dx%d, %d bounces, %d spp" % ((what,) + size), "frames": n,
                "frames_per_s_update": n / t_upd, "frames_per_s_new_handle": n / t_new,
                # the first frame of both loops creates the handle: the hand-off of the others is what differs
                "handoff_ms_median_update": median(h_upd[1:]), "handoff_ms_median_new_handle": median(h_new[1:]),
                "handoff_ms_first": h_new[0], "render_ms_median_update": median(r_upd[1:]),
                "render_ms_median_new_handle": median(r_new[1:]), "frames_bit_equal": equal}
        print(json.dumps(line), flush=True)
        lines.append(line)
        if not equal:
            sys.exit("animation_bench: %s: a frame through GpuScene.update differs from the new handle's" % name)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
