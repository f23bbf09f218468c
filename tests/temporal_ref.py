"""What the temporal-filter tests compare against: a numpy float32 restatement of DESIGN.md §11
(reprojection and blend, spatial variance, variance-guided a-trous), operation for operation, with
an explicit state dict carried from call to call; and a second reading of the reprojection decision
alone in float64.  Guides come from denoise_ref.oracle_gbuffer_of (the CPU oracle), `exp` from
oracle.math_eval; sqrt, floor and / are numpy's float32 ones (correctly rounded)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
from denoise_ref import B3, F32, _d2, oracle_gbuffer_of, scene_by_name

G3 = [F32(0.25), F32(0.5), F32(0.25)]
TEMPORAL_DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, max_history=32, normal_cos=0.9, plane_distance=0.02,
                         sigma_luminance=4.0, variance_history=4)
DENOISE_DEFAULTS = dict(iterations=5, demodulate=1, sigma_normal=0.3, sigma_position=1.0, albedo_floor=1e-3)
FAULTS = ("no_inverse", "row0_top", "wrong_pixel_normal")


def camera_of(scene, w, h):
    """(position, inv_view, inv_proj) of the scene's own camera at w x h, as the renderer sets it."""
    from optixpathtracer_amd.renderer import camera_from_blender

    return camera_from_blender(scene.camera_blender_pos, scene.camera_blender_rot, scene.fov_deg, w, h)


def with_camera(scene, pos, rot):
    return dataclasses.replace(scene, camera_blender_pos=tuple(pos), camera_blender_rot=tuple(rot))


@functools.lru_cache(maxsize=None)
def oracle_view(name: str, pos: tuple, rot: tuple, w: int, h: int):
    """(guides, camera) of a named scene seen from a Blender-style camera, computed once per session."""
    sc = with_camera(scene_by_name(name), pos, rot)
    return oracle_gbuffer_of(sc, w, h), camera_of(sc, w, h)


def mat4_inverse(m):
    """glm::inverse (compute_inverse<4,4>) in float32 scalars, the order of pt::mat4_inverse."""
    m = [F32(v) for v in np.asarray(m, F32).reshape(16)]

    def M(c, r):
        return m[c * 4 + r]

    C00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3); C02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3)
    C03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3); C04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3)
    C06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3); C07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3)
    C08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2); C10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2)
    C11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2); C12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3)
    C14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3); C15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3)
    C16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2); C18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2)
    C19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2); C20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1)
    C22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1); C23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1)
    F0, F1, F2 = [C00, C00, C02, C03], [C04, C04, C06, C07], [C08, C08, C10, C11]
    F3, F4, F5 = [C12, C12, C14, C15], [C16, C16, C18, C19], [C20, C20, C22, C23]
    V0, V1 = [M(1, 0), M(0, 0), M(0, 0), M(0, 0)], [M(1, 1), M(0, 1), M(0, 1), M(0, 1)]
    V2, V3 = [M(1, 2), M(0, 2), M(0, 2), M(0, 2)], [M(1, 3), M(0, 3), M(0, 3), M(0, 3)]
    SA, SB = [F32(1), F32(-1), F32(1), F32(-1)], [F32(-1), F32(1), F32(-1), F32(1)]
    I0 = [(V1[i] * F0[i] - V2[i] * F1[i] + V3[i] * F2[i]) * SA[i] for i in range(4)]
    I1 = [(V0[i] * F0[i] - V2[i] * F3[i] + V3[i] * F4[i]) * SB[i] for i in range(4)]
    I2 = [(V0[i] * F1[i] - V1[i] * F3[i] + V3[i] * F5[i]) * SA[i] for i in range(4)]
    I3 = [(V0[i] * F2[i] - V1[i] * F4[i] + V2[i] * F5[i]) * SB[i] for i in range(4)]
    d0, d1, d2, d3 = M(0, 0) * I0[0], M(0, 1) * I1[0], M(0, 2) * I2[0], M(0, 3) * I3[0]
    one = F32(1) / ((d0 + d1) + (d2 + d3))
    out = np.array([v * one for v in I0 + I1 + I2 + I3], F32)
    assert out.dtype == F32
    return out


def _mul(m, v):
    """mat4_mul_vec4: column-major m (16), v a list of four (H, W) arrays."""
    return [(m[r] * v[0] + m[4 + r] * v[1]) + (m[8 + r] * v[2] + m[12 + r] * v[3]) for r in range(4)]


def _lum(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def temporal_ref(state, image, g, cam, scale=1.0, fault=None, **options):
    """One pt_denoise_temporal call.  state: None (no history) or what the previous call returned;
    g: the present view's guides; cam: (position, inv_view, inv_proj) of the present view.
    Returns (out, state'): state' holds normal, position, valid, inv_view, inv_proj for the next
    call's reprojection, and length, moments, variance (what entered iteration 0), color (iteration
    0's result), color_variance, reprojected, reset.  fault: one of FAULTS, a seeded mistake."""
    from oracle.oracle import math_eval

    T = dict(TEMPORAL_DEFAULTS)
    D = dict(DENOISE_DEFAULTS)
    for k, v in options.items():
        if k in T:
            T[k] = v
        elif k in D:
            D[k] = v
        elif k != "sigma_color":
            raise KeyError(k)
    assert fault is None or fault in FAULTS
    with np.errstate(all="ignore"):
        x = np.asarray(image, F32)
        if F32(scale) != F32(1):
            x = x * F32(scale)
        h, w, _ = x.shape
        valid = g["prim"] >= 0
        v3 = valid[..., None]
        floor = F32(D["albedo_floor"])
        a_p = np.where(g["albedo"] < floor, floor, g["albedo"])
        demod = bool(D["demodulate"])
        c = np.where(v3 & demod, x / a_p, x)  # step 0: the pack pass
        n, pos, depth = g["normal"], g["position"], g["depth"]
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]

        # ---- step 1: reproject and blend
        l = _lum(c)
        accepted = np.zeros((h, w), bool)
        hcol, h1, h2, hlen = np.zeros((h, w, 3), F32), np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
        if state is not None:
            Vp = mat4_inverse(state["inv_view"]) if fault != "no_inverse" else np.asarray(state["inv_view"], F32)
            Pp = mat4_inverse(state["inv_proj"])
            P = [pos[..., 0], pos[..., 1], pos[..., 2], np.ones((h, w), F32)]
            clip = _mul(Pp, _mul(Vp, P))
            fx = ((clip[0] / clip[3]) * F32(0.5) + F32(0.5)) * F32(w) - F32(0.5)
            fy = ((clip[1] / clip[3]) * F32(0.5) + F32(0.5)) * F32(h) - F32(0.5)
            if fault == "row0_top":
                fy = F32(h - 1) - fy
            have = valid & (clip[3] > 0) & (fx >= F32(-1)) & (fx < F32(w)) & (fy >= F32(-1)) & (fy < F32(h))
            ffx, ffy = np.floor(np.where(have, fx, F32(0))), np.floor(np.where(have, fy, F32(0)))
            ix, iy = ffx.astype(np.int64), ffy.astype(np.int64)
            tx, ty = fx - ffx, fy - ffy
            lim = F32(T["plane_distance"]) * depth
            ws = np.zeros((h, w), F32)
            for j in range(2):
                for i in range(2):
                    qx, qy = ix + i, iy + j
                    ok = have & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    nq = state["normal"][(qy + h // 2) % h, qx]  # the fault "wrong_pixel_normal" reads this one, half an image away
                    ok &= state["valid"][qy, qx]
                    ok &= _dot(state["normal"][qy, qx], n) >= F32(T["normal_cos"])
                    d = pos - state["position"][qy, qx]
                    ok &= np.abs(_dot(d, n if fault != "wrong_pixel_normal" else nq)) <= lim
                    hc, hm, hl = state["color"][qy, qx], state["moments"][qy, qx], state["length"][qy, qx]
                    ok &= np.isfinite(hc).all(-1) & np.isfinite(hm).all(-1) & np.isfinite(hl)
                    wgt = (tx if i else F32(1) - tx) * (ty if j else F32(1) - ty)
                    ws = np.where(ok, ws + wgt, ws)
                    hcol = np.where(ok[..., None], hcol + hc * wgt[..., None], hcol)
                    h1 = np.where(ok, h1 + hm[..., 0] * wgt, h1)
                    h2 = np.where(ok, h2 + hm[..., 1] * wgt, h2)
                    hlen = np.where(ok, hlen + hl * wgt, hlen)
            accepted = have & (ws >= F32(0.01))
            hcol, h1, h2, hlen = hcol / ws[..., None], h1 / ws, h2 / ws, hlen / ws
        N = hlen + F32(1)
        N = np.where(N < F32(T["max_history"]), N, F32(T["max_history"]))
        N = np.where(accepted, N, F32(1))
        r = F32(1) / N
        a = np.where(F32(T["alpha"]) < r, r, F32(T["alpha"]))
        am = np.where(F32(T["alpha_moments"]) < r, r, F32(T["alpha_moments"]))
        t = np.where(accepted[..., None], hcol + (c - hcol) * a[..., None], c)
        m1 = np.where(accepted, h1 + (l - h1) * am, l)
        m2 = np.where(accepted, h2 + (l * l - h2) * am, l * l)
        dv = m2 - m1 * m1
        var = np.where(dv > 0, dv, F32(0))
        # a miss passes its colour through with length 0, moments 0, variance 0
        t = np.where(v3, t, c)
        m1, m2, N, var = (np.where(valid, u, F32(0)) for u in (m1, m2, N, var))
        reprojected, reset = int((valid & accepted).sum()), int((valid & ~accepted).sum())

        # ---- step 2: spatial variance where the history is short
        inv_n = F32(1) / (F32(D["sigma_normal"]) * F32(D["sigma_normal"]))
        inv_p = F32(1) / (F32(D["sigma_position"]) * F32(D["sigma_position"]))
        vh = F32(T["variance_history"])
        if T["variance_history"] > 1:
            sw, s1, s2 = np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    qy, qx = ys + dy, xs + dx
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    take = inside & valid[qy, qx]
                    wgt = math_eval("exp", -(_d2(n[qy, qx] - n) * inv_n + _d2(pos[qy, qx] - pos) * inv_p))
                    if dx == 0 and dy == 0:
                        wgt = np.ones((h, w), F32)
                    sw = np.where(take, sw + wgt, sw)
                    s1 = np.where(take, s1 + m1[qy, qx] * wgt, s1)
                    s2 = np.where(take, s2 + m2[qy, qx] * wgt, s2)
            mu1, mu2 = s1 / sw, s2 / sw
            dv = mu2 - mu1 * mu1
            var = np.where(valid & (N < vh), np.where(dv > 0, dv, F32(0)) * (vh / N), var)
        new = {"normal": n, "position": pos, "valid": valid, "inv_view": np.asarray(cam[1], F32).copy(),
               "inv_proj": np.asarray(cam[2], F32).copy(), "length": N, "moments": np.stack([m1, m2], -1),
               "variance": var, "reprojected": reprojected, "reset": reset}

        # ---- step 3: the variance-guided iterations over colour | variance
        c, v = t, var
        sl = F32(T["sigma_luminance"])
        for it in range(D["iterations"]):
            s = 1 << it
            gsum, ks = np.zeros((h, w), F32), np.zeros((h, w), F32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx = ys + dy, xs + dx
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    take = inside & valid[qy, qx]
                    k = G3[dy + 1] * G3[dx + 1]
                    gsum = np.where(take, gsum + v[qy, qx] * k, gsum)
                    ks = np.where(take, ks + k, ks)
            den = sl * np.sqrt(gsum / ks) + F32(1e-8)
            lp = _lum(c)
            acc, vacc, wsum = np.zeros((h, w, 3), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * s, xs + dx * s
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    cq = c[qy, qx]
                    aa = (np.abs(_lum(cq) - lp) / den + _d2(n[qy, qx] - n) * inv_n) + _d2(pos[qy, qx] - pos) * inv_p
                    if dx == 0 and dy == 0:
                        aa = np.zeros((h, w), F32)
                    take = inside & valid[qy, qx] & ~np.isnan(aa)
                    wt = (B3[dy + 2] * B3[dx + 2]) * math_eval("exp", -aa)
                    acc = np.where(take[..., None], acc + cq * wt[..., None], acc)
                    vacc = np.where(take, vacc + v[qy, qx] * (wt * wt), vacc)
                    wsum = np.where(take, wsum + wt, wsum)
            c = np.where(v3, acc / wsum[..., None], c)
            v = np.where(valid, vacc / (wsum * wsum), v)
            if it == 0:
                new["color"], new["color_variance"] = c, v
        out = np.where(v3 & demod, c * a_p, c)  # step 4
    for k in ("length", "moments", "variance", "color", "color_variance"):
        assert new[k].dtype == F32, k
    assert out.dtype == F32
    return out, new


def reprojection_f64(prev, g, options=None):
    """The reprojection decision alone, read a second time in float64: float64 inverses of the
    previous camera's matrices (numpy.linalg.inv), the same thresholds, all previous history taken
    as finite.  prev: a state of temporal_ref (guides and camera are read).  Returns (accept, near):
    per pixel, whether a hit pixel takes up history, and whether any value tested lies within 1e-4
    relative of its threshold or a reprojected coordinate within 1e-3 of a pixel boundary."""
    T = dict(TEMPORAL_DEFAULTS)
    T.update(options or {})
    f8 = np.float64
    h, w = g["prim"].shape
    valid = g["prim"] >= 0
    V = np.linalg.inv(np.asarray(prev["inv_view"], f8).reshape(4, 4).T)  # column-major storage -> matrix
    Pm = np.linalg.inv(np.asarray(prev["inv_proj"], f8).reshape(4, 4).T)
    pos, n = g["position"].astype(f8), g["normal"].astype(f8)
    P = np.concatenate([pos, np.ones((h, w, 1))], -1)
    clip = P @ (Pm @ V).T
    with np.errstate(all="ignore"):
        fx = (clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * w - 0.5
        fy = (clip[..., 1] / clip[..., 3] * 0.5 + 0.5) * h - 0.5
    front = clip[..., 3] > 0
    ok_range = front & (fx >= -1) & (fx < w) & (fy >= -1) & (fy < h)
    fxs, fys = np.where(ok_range, fx, 0.0), np.where(ok_range, fy, 0.0)
    ix, iy = np.floor(fxs).astype(np.int64), np.floor(fys).astype(np.int64)
    tx, ty = fxs - ix, fys - iy
    near = np.abs(clip[..., 3]) < 1e-4
    near |= ok_range & ((np.abs(fxs - np.round(fxs)) < 1e-3) | (np.abs(fys - np.round(fys)) < 1e-3))
    with np.errstate(all="ignore"):  # the edge of the range in which any tap is inside
        near |= front & ((np.abs(fx + 1) < 1e-3) | (np.abs(fx - w) < 1e-3) | (np.abs(fy + 1) < 1e-3) | (np.abs(fy - h) < 1e-3))

    def close(value, threshold):
        return np.abs(value - threshold) <= 1e-4 * np.maximum(np.abs(threshold), 1e-30)

    lim = T["plane_distance"] * g["depth"].astype(f8)
    ws = np.zeros((h, w))
    for j in range(2):
        for i in range(2):
            qx, qy = ix + i, iy + j
            inside = ok_range & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            inside &= prev["valid"][qy, qx]
            dn = (prev["normal"][qy, qx].astype(f8) * n).sum(-1)
            pd = np.abs(((pos - prev["position"][qy, qx].astype(f8)) * n).sum(-1))
            near |= inside & (close(dn, T["normal_cos"]) | close(pd, lim))
            ok = inside & (dn >= T["normal_cos"]) & (pd <= lim)
            ws += np.where(ok, (tx if i else 1 - tx) * (ty if j else 1 - ty), 0.0)
    near |= ok_range & close(ws, 0.01)
    return valid & ok_range & (ws >= 0.01), valid & near
