"""examples/marbles.rs: 25 marbles fall into a glass.  Each frame builds the scene from the particle state, renders
it on the GPU and writes video/image_<frame>.png, then MarblesSystem integrates 1/16 s (625 RK4 steps) on the GPU.
One scene handle serves the whole run: each frame moves its marbles with GpuScene.update (the same pixels as a new
handle per frame); --rebuild creates a new handle per frame, as the example does.

Usage: python scripts/marbles.py [--frames 180] [--test] [--width W --height H --spp S --bounces B] [--out video]
       [--rebuild]
--test is the example's TEST = true branch (200 x 150, 7 bounces, 1 spp, an ambient light).  Stand-ins (scenes.marbles):
the analytic monomial_surface(2, 4) for monomial.obj unless $RPT_ASSETS has it, synthetic_hdri for ballroom_8k.hdr.
"""
import argparse
import os
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpt_amd import GpuScene, Renderer, scenes  # noqa: E402
from rpt_amd.ode import MarblesSystem  # noqa: E402


def save_png(img, path):
    """(H, W, 3) uint8 -> an 8-bit RGB PNG (no filter), with the standard library only"""
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=180)
    ap.add_argument("--test", action="store_true")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--spp", type=int)
    ap.add_argument("--bounces", type=int)
    ap.add_argument("--out", default="video")
    ap.add_argument("--rebuild", action="store_true", help="a new scene handle per frame instead of GpuScene.update")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    state = scenes.marbles_start()
    system = MarblesSystem(scenes.MARBLES_R)
    gpu = None
    for frame in range(a.frames):
        t0 = time.perf_counter()
        scene, camera, cfg = scenes.marbles(state, test=a.test)
        r = (Renderer(scene, camera).width(a.width or cfg["width"]).height(a.height or cfg["height"])
             .max_bounces(a.bounces or cfg["max_bounces"]).num_samples(a.spp or cfg["num_samples"]))
        if not a.rebuild:
            if gpu is None:
                gpu = GpuScene(scene, 0)
            else:
                gpu.update(scene)
            r.with_gpu_scene(gpu)
        save_png(r.render(), os.path.join(a.out, "image_%d.png" % frame))
        t1 = time.perf_counter()
        system.rk4_integrate(state, 1.0 / 16.0, 1.0 / 10000.0)
        t2 = time.perf_counter()
        print("Frame %d finished (render %.2f s, integrate %.2f ms)" % (frame, t1 - t0, 1e3 * (t2 - t1)))


if __name__ == "__main__":
    main()
