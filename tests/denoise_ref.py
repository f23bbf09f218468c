"""What the feature-buffer and denoiser tests compare against: the first-hit G-buffer from the CPU
oracle's debug records, and a numpy float32 restatement of the a-trous filter,
operation for operation, with the shared exp polynomial from oracle.math_eval."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

F32 = np.float32
B3 = [F32(1 / 16), F32(1 / 4), F32(3 / 8), F32(1 / 4), F32(1 / 16)]
AOVS = ["albedo", "normal", "geom_normal", "position", "depth", "prim", "rough_metal"]


def scene_by_name(name: str):
    from optixpathtracer_amd import scenes

    if name.startswith("tiny:"):
        return scenes.tiny_scene(name[5:])
    if name.startswith("textured:"):
        return scenes.textured_scene(name[9:])
    return scenes.make_scene(name)


def oracle_gbuffer_of(scene, w: int, h: int) -> dict:
    """The seven AOVs of `scene` from its own camera at w x h: per pixel, record 0 of the oracle's
    debug path (any frame: the camera ray has no jitter), and the depth from the oracle's trace of
    the oracle's camera ray over [0, 100].  A pixel without a record is a miss: prim -1, zeros."""
    from oracle.oracle import OracleScene, fp, load

    o = OracleScene(scene)
    lp = o.launch(w, h, 1)
    g = {"albedo": np.zeros((h, w, 3), F32), "normal": np.zeros((h, w, 3), F32), "geom_normal": np.zeros((h, w, 3), F32),
         "position": np.zeros((h, w, 3), F32), "depth": np.zeros((h, w), F32), "prim": np.full((h, w), -1, np.int32),
         "rough_metal": np.zeros((h, w, 2), F32)}
    rays = np.zeros((h, w, 8), F32)
    rays[..., 7] = 100.0
    ro, rd = np.zeros(3, F32), np.zeros(3, F32)
    for y in range(h):
        for x in range(w):
            load().orc_camera_ray(C.byref(lp), x, y, fp(ro), fp(rd))
            rays[y, x, 0:3], rays[y, x, 3:6] = ro, rd
            rec, _ = o.sample_path_debug(lp, x, y, 1, max_bounces=1)
            if len(rec) == 0:
                continue
            r = rec[0]
            g["prim"][y, x] = r[1:2].view(np.int32)[0]
            g["position"][y, x], g["albedo"][y, x] = r[2:5], r[5:8]
            g["normal"][y, x], g["geom_normal"][y, x] = r[8:11], r[11:14]
            g["rough_metal"][y, x] = r[14:16]
    prim, t, _, _, _ = o.trace(rays.reshape(-1, 8))
    g["depth"][...] = np.where(prim >= 0, t, F32(0)).reshape(h, w)
    g["trace_prim"] = prim.reshape(h, w)
    o.close()
    for a in g.values():
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def oracle_gbuffer(name: str, w: int, h: int) -> dict:
    """oracle_gbuffer_of a named scene, computed once per session and read-only."""
    return oracle_gbuffer_of(scene_by_name(name), w, h)


def _d2(u):
    return (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]


def atrous_ref(image, g, scale=1.0, iterations=5, demodulate=1, sigma_color=1.0, sigma_normal=0.3, sigma_position=1.0,
               albedo_floor=1e-3) -> np.ndarray:
    """The filter of DESIGN.md §10 on `image` (H, W, 3) with the guides g (albedo, normal, position,
    prim), every operation a separate float32 numpy operation in the kernel's order.  A skipped tap
    leaves the sums as they are (np.where), it does not add a zero."""
    from oracle.oracle import math_eval

    with np.errstate(all="ignore"):
        x = np.asarray(image, F32)
        if F32(scale) != F32(1):
            x = x * F32(scale)
        h, w, _ = x.shape
        valid = g["prim"] >= 0
        v3 = valid[..., None]
        floor = F32(albedo_floor)
        a_p = np.where(g["albedo"] < floor, floor, g["albedo"])
        demod = bool(demodulate)
        c = np.where(v3 & demod, x / a_p, x)
        n, pos = g["normal"], g["position"]
        inv_n = F32(1) / (F32(sigma_normal) * F32(sigma_normal))
        inv_p = F32(1) / (F32(sigma_position) * F32(sigma_position))
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        for i in range(iterations):
            s = 1 << i
            sc = F32(sigma_color) * F32(2.0 ** -i)
            inv_c = F32(1) / (sc * sc)
            acc = np.zeros((h, w, 3), F32)
            wsum = np.zeros((h, w), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * s, xs + dx * s
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    cq = c[qy, qx]
                    a = (_d2(cq - c) * inv_c + _d2(n[qy, qx] - n) * inv_n) + _d2(pos[qy, qx] - pos) * inv_p
                    if dx == 0 and dy == 0:
                        a = np.zeros((h, w), F32)
                    take = inside & valid[qy, qx] & ~np.isnan(a)
                    wt = (B3[dy + 2] * B3[dx + 2]) * math_eval("exp", -a)
                    acc = np.where(take[..., None], acc + cq * wt[..., None], acc)
                    wsum = np.where(take, wsum + wt, wsum)
            c = np.where(v3, acc / wsum[..., None], c)
        out = np.where(v3 & demod, c * a_p, c)
    assert out.dtype == F32
    return out


def same_bits(a, b) -> bool:
    """Equal bit for bit, except that any NaN equals any NaN: the same places hold NaNs."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())
