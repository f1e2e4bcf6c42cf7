"""`Color` helpers (reference src/color.rs:10-24).  Host-side, off the timed path."""
import math

import numpy as np

SRGB_GAMMA = 2.2


def hex_color(x):  # color.rs:10-15
    r = ((x >> 16) & 0xFF) / 255.0
    g = ((x >> 8) & 0xFF) / 255.0
    b = (x & 0xFF) / 255.0
    return (r ** SRGB_GAMMA, g ** SRGB_GAMMA, b ** SRGB_GAMMA)


def color_byte(v):
    """color.rs:18-24 for one value, with the C library's pow as Rust's f64::powf: clamp, gamma, `as u8` (truncating,
    NaN -> 0, saturating)"""
    v = 0.0 if math.isnan(v) else min(max(v, 0.0), 1.0)
    t = math.pow(v, 1.0 / SRGB_GAMMA) * 255.0
    return 0 if not t > 0.0 else (255 if t >= 255.0 else int(t))


_THRESHOLDS = None


def byte_thresholds():
    """thr[k], k = 1..255: the smallest double v in [0, 1] with color_byte(v) >= k, by bisection over the bit patterns
    (non-negative doubles order like their bits); thr[0] = 0.  color_byte is this staircase: a value's byte is the
    largest k with thr[k] <= v."""
    global _THRESHOLDS
    if _THRESHOLDS is None:
        one = int(np.float64(1.0).view(np.uint64))
        thr = np.zeros(256)
        for k in range(1, 256):
            lo, hi = 0, one
            while lo < hi:
                mid = (lo + hi) // 2
                if color_byte(float(np.uint64(mid).view(np.float64))) >= k:
                    hi = mid
                else:
                    lo = mid + 1
            thr[k] = np.uint64(lo).view(np.float64)
        _THRESHOLDS = thr
    return _THRESHOLDS


def color_bytes(color):  # color.rs:18-24 — clamp, gamma, `as u8` (truncating, NaN -> 0)
    # through the thresholds of the C library's pow, not np.power: numpy's vectorised pow differs from it by an ulp on
    # some inputs and machines, which moves some thresholds by an ulp (the device's rpt_buffer_image uses the same
    # staircase, built from the same pow)
    c = np.asarray(color, dtype=np.float64)
    t = np.minimum(np.maximum(c, 0.0), 1.0)
    t = np.where(np.isnan(t), 0.0, t)
    return (np.searchsorted(byte_thresholds(), t, side="right") - 1).astype(np.uint8)
