"""The rays of rptgpu_render_views restated in numpy from include/rpt_gpu.h alone: for one view and one sample index, the
origin and direction of every pixel's ray, expression for expression (IEEE f64 — numpy never contracts).  The draws are
the oracle's (oracle.rng_sample on the pixel's stream from draw 0 on); sine and cosine are the caller's `sincos`, a
function x -> (sin x, cos x) over arrays: include/rpt_math.h built for the host (host_sincos) or evaluated on the device
(device_sincos), whose bits a device comparison needs."""
import numpy as np

TWO_PI, PI = 6.283185307179586, 3.141592653589793


def host_sincos(oracle):
    return lambda x: (oracle.math_eval(3, x), oracle.math_eval(4, x))


def device_sincos(g):
    return lambda x: (g.eval_math(3, x), g.eval_math(4, x))


def jitter(oracle, seed, npix, sample, lo, hi):
    """the two gen_range(lo, hi) every pixel's stream (seed, pixel, sample) starts with -> (npix, 2); two draws each"""
    out = np.empty((npix, 2))
    for p in range(npix):
        a, n = oracle.rng_sample(1, lo, hi, seed=seed, pixel=p, sample=sample, draw=0)
        b, n = oracle.rng_sample(1, lo, hi, seed=seed, pixel=p, sample=sample, draw=n)
        assert n == 2
        out[p] = a[0], b[0]
    return out


def _xy(width, height):
    p = np.arange(width * height)
    return (p % width).astype(np.float64), (p // width).astype(np.float64), p % width, p // width


def _normalize(a):
    return a / np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])[..., None]


def _v(x):
    return np.array([float(c) for c in x])


def film(oracle, seed, width, height, sample):
    """px, py of renderer.rs:132-138 for every pixel"""
    _, _, x, y = _xy(width, height)
    dim = float(max(width, height))
    xn = ((2 * x + 1).astype(np.float64) - float(width)) / dim
    yn = ((2 * (height - y) - 1).astype(np.float64) - float(height)) / dim
    j = jitter(oracle, seed, width * height, sample, -1.0 / dim, 1.0 / dim)
    return xn + j[:, 0], yn + j[:, 1]


def camera_frame(camera):
    direction, up = _v(camera.direction), _v(camera.up)
    cr = np.array([direction[1] * up[2] - direction[2] * up[1], direction[2] * up[0] - direction[0] * up[2],
                   direction[0] * up[1] - direction[1] * up[0]])
    return _v(camera.eye), direction, up, _normalize(cr)


def perspective_rays(oracle, camera, seed, width, height, sample):
    """RPT_VIEW_PERSPECTIVE without a lens (camera.rs:64-81 with aperture 0)"""
    assert camera.aperture == 0.0
    eye, direction, up, right = camera_frame(camera)
    px, py = film(oracle, seed, width, height, sample)
    d = 1.0 / np.tan(camera.fov / 2.0)
    new_dir = (d * direction + px[:, None] * right) + py[:, None] * up
    return np.tile(eye, (len(px), 1)), _normalize(new_dir)


def orthographic_rays(oracle, camera, ortho_scale, seed, width, height, sample):
    """RPT_VIEW_ORTHOGRAPHIC: origin = eye + (px*right + py*up) * ortho_scale, dir = normalize(direction)"""
    eye, direction, up, right = camera_frame(camera)
    px, py = film(oracle, seed, width, height, sample)
    origin = eye + (px[:, None] * right + py[:, None] * up) * float(ortho_scale)
    return origin, np.tile(_normalize(direction), (len(px), 1))


def panorama_texels(oracle, seed, width, height, sample):
    """(cx, cy): where in the panorama's texel grid every pixel's ray of this sample points"""
    xf, yf, _, _ = _xy(width, height)
    j = jitter(oracle, seed, width * height, sample, -0.5, 0.5)
    wm, hm = float(width - 1), float(height - 1)
    cx = xf + j[:, 0]
    cx = np.where(cx < 0.0, cx + wm, np.where(cx > wm, cx - wm, cx))
    cy = np.minimum(np.maximum(yf + j[:, 1], 0.0), hm)
    return cx, cy


def panorama_rays(oracle, eye, seed, width, height, sample, sincos):
    """RPT_VIEW_PANORAMA -> origins, dirs, cx, cy"""
    cx, cy = panorama_texels(oracle, seed, width, height, sample)
    wm, hm = float(width - 1), float(height - 1)
    psi = cx / wm - 0.5
    back = np.abs(psi) > 0.25
    s, c = sincos(TWO_PI * np.where(back, psi - np.copysign(0.5, psi), psi))
    s, c = np.where(back, -s, s), np.where(back, -c, c)
    se, ce = sincos((0.5 - cy / hm) * PI)
    dirs = np.stack([ce * c, se, ce * s], axis=1)
    return np.tile(_v(eye), (len(cx), 1)), dirs, cx, cy
