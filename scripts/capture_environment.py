"""A panorama of one scene becomes the Hdri of another (rptgpu_render_views).

RPT_VIEW_PANORAMA renders 360 degrees around a point in exactly Hdri::get_color's convention (environment.rs:25-52:
column <-> atan2(z, x) + pi over width-1, row <-> acos(y) over height-1), so the frame IS an Hdri's texel array: no
resampling, no flip.  This script captures the Cornell box from its middle, makes that capture the environment of a
scene that holds one mirror sphere and nothing else — no lights: everything it shows comes from the capture —, renders
the sphere, and writes both images as binary PPM.

    python scripts/capture_environment.py [--size 512 256] [--spp 64] [--out-dir .]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rpt_amd import (Camera, Environment, GpuScene, Hdri, Material, Object, Scene, View, color_bytes, make_params,  # noqa: E402
                     scenes, sphere)


def write_ppm(path, rgb):
    """linear f64 (H, W, 3) through the reference's colour bytes (color.rs) into a P6 file"""
    h, w, _ = rgb.shape
    data = bytes(b for px in rgb.reshape(-1, 3) for b in color_bytes(px))
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[512, 256], metavar=("W", "H"))
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--out-dir", default=".")
    args = ap.parse_args()
    w, h = args.size
    # 1. the capture: one panoramic view from the middle of the box
    room, _, cfg = scenes.cornell()
    g = GpuScene(room, 0)
    pano = g.render_views([View.panorama((278.0, 273.0, 280.0))], w, h, cfg["max_bounces"], samples=args.spp, seed=1)[0]
    g.close()
    # 2. the capture as another scene's environment, as it is
    scene = Scene()
    scene.environment = Environment.Hdri(Hdri(w, h, pano))
    scene.add(Object(sphere()).material(Material.metallic_((1.0, 1.0, 1.0), 0.02)))
    camera = Camera.look_at((0.0, 0.5, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.6)
    g = GpuScene(scene, 0)
    p = make_params(480, 360, 4, args.spp, seed=2)
    ball = g.render_batch(camera, p).reshape(p.height, p.width, 3)
    g.close()
    os.makedirs(args.out_dir, exist_ok=True)
    write_ppm(os.path.join(args.out_dir, "captured_environment.ppm"), pano)
    write_ppm(os.path.join(args.out_dir, "mirror_sphere.ppm"), ball)
    # a ray that misses everything looks up the texel it was captured into: straight up is the room's ceiling light's row
    print("panorama %dx%d at %d spp: mean %.4f, top row mean %.4f, bottom row mean %.4f; sphere frame mean %.4f"
          % (w, h, args.spp, pano.mean(), pano[0].mean(), pano[-1].mean(), ball.mean()))
    assert np.isfinite(pano).all() and np.isfinite(ball).all()
    return 0


if __name__ == "__main__":
    sys.exit(main())
