"""numpy restatement of pt_render_adaptive, independent of the C++.

adaptive_reference(frame, w, h, first, ...) drives the rounds from one-frame images
frame(f) -> (H, W, 3) float32 (row 0 = bottom) and returns every piece of state the library
shows: fp32 sums added in frame order, fp64 luminance moments, the per-pixel error, the tile
error by the explicit six-level pairwise tree, the per-tile rounds, the mean, and the pixel list
of every round.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

TILE = 8

# The base case of test_adaptive_ref.py and test_gpu_adaptive.py: tiny scene, Lambert, 52x36 (7x5
# tiles, partial on the right and on top), depth 4, frames from 1.  The threshold was chosen on the
# CPU: this case's tile errors run from 0.12-0.28 after 8 frames to 0.05-0.11 after 64, and 0.07 stops
# 21 of the 35 tiles before max_samples, in rounds 4, 5, 6 and 7 of 8
# (test_adaptive_ref.py::test_threshold_gives_a_mixed_schedule holds it to that).
BASE = dict(w=52, h=36, depth=4, first=1)
OPTIONS = dict(threshold=0.07, min_samples=8, max_samples=64, round_frames=8, luminance_floor=0.01)
LAMBERT, DIELECTRIC, DEFAULT = 1, 3, 0  # PT_MAT_*
PULLED_BACK = (8.0, 0.0, 1.0)  # camera position from which the box no longer fills the view


def luminance(rgb: np.ndarray) -> np.ndarray:
    """fp32 (0.2126 r + 0.7152 g) + 0.0722 b, each operation rounded to fp32."""
    rgb = np.asarray(rgb, np.float32)
    return (np.float32(0.2126) * rgb[..., 0] + np.float32(0.7152) * rgb[..., 1]) + np.float32(0.0722) * rgb[..., 2]


def max_keep_nan(a, b):
    """a < b ? b : a -- a NaN in a stays."""
    return np.where(a < b, b, a)


def pixel_error(n, s1, s2, floor):
    """e of §12 in fp64 from counts and moments (arrays of one shape)."""
    with np.errstate(all="ignore"):
        dn = n.astype(np.float64)
        m = s1 / dn
        v = max_keep_nan(s2 / dn - m * m, np.float64(0.0)) / dn
        return np.sqrt(v) / max_keep_nan(m, np.float64(np.float32(floor)))


def tree_sum64(slots: np.ndarray) -> np.float64:
    """The sum of 64 fp64 slots by the fixed tree: level k = 0..5 adds the elements whose index
    differs in bit k (a butterfly: every element ends with the same total)."""
    v = np.array(slots, np.float64)
    assert v.shape == (64,)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for k in range(6):
            v = v + v[idx ^ (1 << k)]
    assert np.array_equal(v.view(np.uint64), np.full(64, v[:1].view(np.uint64)[0])) or np.isnan(v).all()
    return v[0]


def tile_slots(e: np.ndarray, tx: int, ty: int) -> tuple[np.ndarray, int]:
    """The tile's 64 slots in tile-raster order (slot = 8 * row + column), 0 outside the image, and
    the number of in-image pixels."""
    h, w = e.shape
    slots = np.zeros((TILE, TILE), np.float64)
    y0, x0 = ty * TILE, tx * TILE
    th, tw = min(TILE, h - y0), min(TILE, w - x0)
    slots[:th, :tw] = e[y0:y0 + th, x0:x0 + tw]
    return slots.reshape(64), th * tw


def round_up(v: int, to: int) -> int:
    return (v + to - 1) // to * to


def adaptive_reference(frame, w: int, h: int, first: int = 1, threshold: float = 0.05, min_samples: int = 16,
                       max_samples: int = 1024, round_frames: int = 16, luminance_floor: float = 0.01):
    R = int(round_frames)
    min_n, max_n = round_up(int(min_samples), R), round_up(int(max_samples), R)
    thr = np.float64(np.float32(threshold))
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    n = np.zeros((h, w), np.uint32)
    acc = np.zeros((h, w, 3), np.float32)
    s1 = np.zeros((h, w), np.float64)
    s2 = np.zeros((h, w), np.float64)
    err = np.zeros((h, w), np.float32)
    tile_err = np.zeros((tiles_y, tiles_x), np.float32)
    tile_err64 = np.zeros((tiles_y, tiles_x), np.float64)
    tile_rounds = np.zeros((tiles_y, tiles_x), np.int32)
    active = np.ones((tiles_y, tiles_x), bool)
    stopped = np.zeros((tiles_y, tiles_x), bool)  # by the threshold
    stop_round = np.full((tiles_y, tiles_x), -1, np.int32)
    round_pixels = []
    done = 0
    while done < max_n and active.any():
        # the round's pixels: tile index ascending, raster order inside the tile
        px = []
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                if not active[ty, tx]:
                    continue
                for y in range(ty * TILE, min(h, ty * TILE + TILE)):
                    px.extend(range(y * w + tx * TILE, y * w + min(w, tx * TILE + TILE)))
        px = np.asarray(px, np.int64)
        round_pixels.append(px)
        mask = np.zeros(h * w, bool)
        mask[px] = True
        mask = mask.reshape(h, w)
        with np.errstate(all="ignore"):
            for f in range(first + done, first + done + R):  # frames in order
                img = np.asarray(frame(f), np.float32)
                assert img.shape == (h, w, 3)
                acc[mask] = acc[mask] + img[mask]
                y = luminance(img).astype(np.float64)
                s1[mask] = s1[mask] + y[mask]
                s2[mask] = s2[mask] + y[mask] * y[mask]
        n[mask] += np.uint32(R)
        done += R
        e = pixel_error(np.maximum(n, 1), s1, s2, luminance_floor)
        err[mask] = e[mask].astype(np.float32)
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                if not active[ty, tx]:
                    continue
                slots, cnt = tile_slots(e, tx, ty)
                with np.errstate(all="ignore"):
                    te = tree_sum64(slots) / np.float64(cnt)
                tile_err64[ty, tx] = te
                tile_err[ty, tx] = np.float32(te)
                tile_rounds[ty, tx] += 1
                tn = int(n[ty * TILE, tx * TILE])
                if te <= thr and tn >= min_n:
                    active[ty, tx] = False
                    stopped[ty, tx] = True
                    stop_round[ty, tx] = tile_rounds[ty, tx]
                elif tn >= max_n:
                    active[ty, tx] = False
    with np.errstate(all="ignore"):
        mean = acc / n.astype(np.float32)[..., None]
    return SimpleNamespace(n=n, sum=acc, moments=np.stack([s1, s2], axis=-1), error=err, tile_error=tile_err,
                           tile_error64=tile_err64, tile_rounds=tile_rounds, stopped=stopped, stop_round=stop_round,
                           mean=mean, round_pixels=round_pixels, rounds=len(round_pixels), samples=int(n.sum(dtype=np.uint64)),
                           min_n=min_n, max_n=max_n, round_frames=R)
