"""numpy restatement of the pixel filter (pt_set_pixel_filter), independent of the C++.

With supersample = s, output pixel (x, y) at frame F takes the path of pixel (s x + sx, s y + sy) of
the s-fold image at frame F, so a frame of the feature is a subsampling of a one-frame image that the
oracle and the plain kernels already produce at the higher resolution.  From such images
frame(F) -> (sH, sW, 3) float32 (row 0 = bottom) this module restates the cells, the taps (fp64,
normalised, then fp32), the tap loop in fp32 in the stated order and the frame-order sum.
"""
from __future__ import annotations

import math

import numpy as np

KINDS = ("box", "tent", "gaussian", "mitchell")
DEFAULT_RADIUS = {"box": 0.5, "tent": 1.0, "gaussian": 1.5, "mitchell": 2.0}
DEFAULT_PARAM = {"box": 0.0, "tent": 0.0, "gaussian": 0.5, "mitchell": 1.0 / 3.0}

# The shapes of test_gpu_pixel_filter.py: 19x17 is more than one 16x16 tile both ways with ragged
# edges; 18 frames from 3 wrap F mod 16, and batches of 5 are ragged.
BASE = dict(w=19, h=17, depth=4, first=3, frames=18, batch=5)
LAMBERT, DIELECTRIC, DEFAULT = 1, 3, 0  # PT_MAT_*


def radical_inverse(c: int) -> int:
    """The 32-bit radical inverse of c: its bits reversed."""
    return int(f"{c & 0xFFFFFFFF:032b}"[::-1], 2)


def sobol2(c: int) -> int:
    """The second Sobol' dimension of c: the xor of the direction numbers v0 = 2^31,
    v(k+1) = v(k) ^ (v(k) >> 1) over the set bits k of c."""
    v, out = 1 << 31, 0
    for k in range(32):
        if c >> k & 1:
            out ^= v
        v ^= v >> 1
    return out


def cell(s: int, frame: int) -> tuple[int, int]:
    """(sx, sy) of frame id `frame` (uint32) under supersample s."""
    b = s.bit_length() - 1
    assert s in (1, 2, 4, 8)
    c = (frame & 0xFFFFFFFF) % (s * s)
    if b == 0:
        return 0, 0
    return radical_inverse(c) >> (32 - b), sobol2(c) >> (32 - b)


def cells(s: int) -> np.ndarray:
    return np.array([cell(s, c) for c in range(s * s)], np.int32)


def resolve(kind: str, radius: float = 0.0, param: float = 0.0) -> tuple[float, float]:
    """radius and param as the library holds them: fp32 values, 0 = the kind's default."""
    r = float(np.float32(radius)) or float(np.float32(DEFAULT_RADIUS[kind]))
    p = float(np.float32(param)) or float(np.float32(DEFAULT_PARAM[kind]))
    return r, p


def tap_radius(kind: str, radius: float = 0.0) -> int:
    return math.ceil(resolve(kind, radius)[0] - 0.5)


def profile(kind: str, t: float, r: float, param: float) -> float:
    a = abs(t)
    if kind == "box":
        return 1.0 if a <= r else 0.0
    if kind == "tent":
        return max(0.0, 1.0 - a / r)
    if kind == "gaussian":
        s2 = 2.0 * param * param
        return max(0.0, math.exp(-(t * t) / s2) - math.exp(-(r * r) / s2))
    B = param
    C = (1.0 - B) / 2.0
    x = 2.0 * a / r
    if x < 1.0:
        return ((12.0 - 9.0 * B - 6.0 * C) * x * x * x + (-18.0 + 12.0 * B + 6.0 * C) * x * x + (6.0 - 2.0 * B)) / 6.0
    if x < 2.0:
        return ((-B - 6.0 * C) * x * x * x + (6.0 * B + 30.0 * C) * x * x + (-12.0 * B - 48.0 * C) * x + (8.0 * B + 24.0 * C)) / 6.0
    return 0.0


def tap_row64(s: int, coord: int, kind: str, radius: float = 0.0, param: float = 0.0) -> np.ndarray:
    """One axis of one cell in fp64: f(i + o) for i = -R..R with o = (coord + 1/2) / s - 1/2, normalised."""
    r, p = resolve(kind, radius, param)
    R = math.ceil(r - 0.5)
    o = (coord + 0.5) / s - 0.5
    v = [profile(kind, i + o, r, p) for i in range(-R, R + 1)]
    total = 0.0
    for x in v:
        total += x
    assert math.isfinite(total) and total > 0.0
    return np.array([x / total for x in v], np.float64)


def taps(s: int, frame: int, kind: str, radius: float = 0.0, param: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
    """(wx, wy) of the frame's cell, fp32."""
    sx, sy = cell(s, frame)
    return (tap_row64(s, sx, kind, radius, param).astype(np.float32),
            tap_row64(s, sy, kind, radius, param).astype(np.float32))


def subsample(frame_img: np.ndarray, s: int, frame: int) -> np.ndarray:
    """The (H, W, 3) image of frame id `frame` from the (sH, sW, 3) one-frame image of that frame id."""
    sx, sy = cell(s, frame)
    return np.ascontiguousarray(np.asarray(frame_img, np.float32)[sy::s, sx::s])


def filter_frame(img: np.ndarray, wx: np.ndarray, wy: np.ndarray) -> np.ndarray:
    """g = 0; for j: for i: g = g + (wy[j] * wx[i]) * L(clamp(X + i), clamp(Y + j)), all in fp32; every tap
    is evaluated, zero weights too."""
    img = np.asarray(img, np.float32)
    h, w, _ = img.shape
    R = (len(wx) - 1) // 2
    assert len(wx) == len(wy) == 2 * R + 1 and wx.dtype == wy.dtype == np.float32
    ys, xs = np.arange(h), np.arange(w)
    g = np.zeros_like(img)
    with np.errstate(all="ignore"):
        for j in range(-R, R + 1):
            rows = np.clip(ys + j, 0, h - 1)
            for i in range(-R, R + 1):
                cols = np.clip(xs + i, 0, w - 1)
                wgt = np.float32(wy[j + R] * wx[i + R])
                g = g + wgt * img[rows][:, cols]
    assert g.dtype == np.float32
    return g


def frame_image(frame, s: int, f: int, kind: str = "box", radius: float = 0.0, param: float = 0.0) -> np.ndarray:
    """One frame's image as the library adds it: the subsampled frame, through the taps when R > 0."""
    img = subsample(frame(f), s, f)
    if tap_radius(kind, radius) == 0:
        return img
    return filter_frame(img, *taps(s, f, kind, radius, param))


def accumulate(frame, s: int, first: int, n: int, kind: str = "box", radius: float = 0.0, param: float = 0.0,
               fp64: bool = False, start=None) -> np.ndarray:
    """The sum buffer after frames first .. first + n - 1, added in frame order in fp32 (fp64: summed
    in fp64, the fp32 rounding returned)."""
    acc = None if start is None else np.array(start, np.float64 if fp64 else np.float32)
    with np.errstate(all="ignore"):
        for f in range(first, first + n):
            g = frame_image(frame, s, f, kind, radius, param)
            if acc is None:
                acc = np.zeros(g.shape, np.float64 if fp64 else np.float32)
            acc = acc + (g.astype(np.float64) if fp64 else g)
    return acc.astype(np.float32)


def single_frame(frame, s: int, f: int, kind: str = "box", radius: float = 0.0, param: float = 0.0) -> np.ndarray:
    """What Render() returns for frame f: 0.0f + the frame's image."""
    with np.errstate(all="ignore"):
        return np.float32(0.0) + frame_image(frame, s, f, kind, radius, param)
