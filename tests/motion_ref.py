"""What the motion-vector tests compare against: DESIGN.md §11 restated in numpy float32 with an
optional previous-position array (temporal_ref.temporal_ref's steps, operation for operation, with
pp in the two places of step 1 that the motion kernel uses it in), the world-space triangles of a
scene as the bake computes them, and a hit's previous position from its barycentrics.  That the
restatement is temporal_ref's when nothing moved is a test of its own (test_motion_ref.py)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
from denoise_ref import B3, F32, _d2, oracle_gbuffer_of
from temporal_ref import DENOISE_DEFAULTS, G3, TEMPORAL_DEFAULTS, _dot, _lum, _mul, mat4_inverse


def translation(x, y, z) -> np.ndarray:
    m = np.eye(4, dtype=F32)
    m[:3, 3] = [x, y, z]
    return m


def wall_matrix() -> np.ndarray:
    """A 5 degree rotation about engine z, then a translation of (0.02, 0, 0)."""
    a = np.deg2rad(5.0)
    r = np.eye(4, dtype=F32)
    r[0, 0], r[0, 1], r[1, 0], r[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return translation(0.02, 0.0, 0.0) @ r


def with_mesh(scene, mesh: int, **changes):
    """`scene` with fields of one mesh replaced."""
    meshes = list(scene.meshes)
    meshes[mesh] = dataclasses.replace(meshes[mesh], **changes)
    return dataclasses.replace(scene, meshes=meshes)


def left_multiplied(scene, mesh: int, m4):
    """`scene` with the 4 x 4 matrix m4 left-multiplied onto one mesh's (column-major) model matrix."""
    model = (np.asarray(m4, F32) @ np.asarray(scene.meshes[mesh].model, F32).reshape(4, 4).T).T.reshape(16).copy()
    assert model.dtype == F32
    return with_mesh(scene, mesh, model=model)


def inflated(scene, mesh: int, by: float):
    """`scene` with every vertex of one mesh displaced along its normal."""
    me = scene.meshes[mesh]
    v = np.asarray(me.vertices, F32) + F32(by) * np.asarray(me.normals, F32)
    return with_mesh(scene, mesh, vertices=v.astype(F32))


def world_triangles(scene) -> np.ndarray:
    """(T, 3, 3) float32: per global triangle (meshes concatenated in order) its three vertices
    through the mesh's model matrix in mat4_mul_vec4's order, as the bake and k_rebake compute them."""
    out = []
    for m in scene.meshes:
        v = np.asarray(m.vertices, F32).reshape(-1, 3)
        M = np.asarray(m.model, F32).reshape(16)
        wv = np.stack(_mul(M, [v[:, 0], v[:, 1], v[:, 2], np.ones(len(v), F32)])[:3], -1)
        assert wv.dtype == F32
        out.append(wv[np.asarray(m.indices, np.int64).reshape(-1, 3)])
    return np.concatenate(out, 0)


def mesh_of_triangle(scene) -> np.ndarray:
    """The mesh index of every global triangle."""
    return np.concatenate([np.full(len(np.asarray(m.indices).reshape(-1, 3)), k, np.int32) for k, m in enumerate(scene.meshes)])


def prev_position(world_tris, prim, u, v) -> np.ndarray:
    """reconstruct's expression for s.pos over world_tris: (w v0 + u v1) + v v2 with w = (1 - u) - v
    per component, at the pixels with prim >= 0; zeros at the others."""
    prim = np.asarray(prim)
    u, v = np.asarray(u, F32)[..., None], np.asarray(v, F32)[..., None]
    t = world_tris[np.clip(prim, 0, len(world_tris) - 1)]
    w = (F32(1) - u) - v
    pp = (w * t[..., 0, :] + u * t[..., 1, :]) + v * t[..., 2, :]
    assert pp.dtype == F32
    return np.where((prim >= 0)[..., None], pp, F32(0))


def oracle_barycentrics(scene, w: int, h: int):
    """(prim, u, v), each (h, w): the oracle's closest-hit trace of the oracle's camera rays over [0, 100]."""
    from oracle.oracle import OracleScene, fp, load

    o = OracleScene(scene)
    lp = o.launch(w, h, 1)
    rays = np.zeros((h, w, 8), F32)
    rays[..., 7] = 100.0
    ro, rd = np.zeros(3, F32), np.zeros(3, F32)
    for y in range(h):
        for x in range(w):
            load().orc_camera_ray(C.byref(lp), x, y, fp(ro), fp(rd))
            rays[y, x, 0:3], rays[y, x, 3:6] = ro, rd
    prim, _, u, v, _ = o.trace(rays.reshape(-1, 8))
    o.close()
    hit = prim >= 0
    return prim.reshape(h, w), np.where(hit, u, F32(0)).reshape(h, w), np.where(hit, v, F32(0)).reshape(h, w)


def oracle_guides(scene, w: int, h: int) -> dict:
    """oracle_gbuffer_of with the barycentrics of the first hit besides ("u", "v")."""
    g = dict(oracle_gbuffer_of(scene, w, h))
    prim, u, v = oracle_barycentrics(scene, w, h)
    assert (prim == g["prim"]).all()
    g["u"], g["v"] = u, v
    for a in (u, v):
        a.setflags(write=False)
    return g


def motion_ref(state, image, g, cam, prev_pos=None, scale=1.0, **options):
    """One pt_denoise_temporal call as temporal_ref.temporal_ref restates it, with prev_pos (H, W, 3;
    None = the present positions) as the point that goes through the previous camera and into the
    plane test.  The state it returns is temporal_ref's, and besides: prev_position (pp at the hit
    pixels, 0 at a miss), screen ((fx - x, fy - y, 1) where a hit pixel had a history and clip.w > 0,
    else zeros), moved (hit pixels where pp differs from the position) and accepted (H, W)."""
    from oracle.oracle import math_eval

    T = dict(TEMPORAL_DEFAULTS)
    D = dict(DENOISE_DEFAULTS)
    for k, v in options.items():
        if k in T:
            T[k] = v
        elif k in D:
            D[k] = v
        elif k not in ("sigma_color", "motion_vectors"):
            raise KeyError(k)
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
        pp = pos if prev_pos is None else np.where(v3, np.asarray(prev_pos, F32), F32(0))
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]

        # ---- step 1: reproject pp and blend
        l = _lum(c)
        accepted = np.zeros((h, w), bool)
        screen = np.zeros((h, w, 3), F32)
        hcol, h1, h2, hlen = np.zeros((h, w, 3), F32), np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
        if state is not None:
            Vp = mat4_inverse(state["inv_view"])
            Pp = mat4_inverse(state["inv_proj"])
            P = [pp[..., 0], pp[..., 1], pp[..., 2], np.ones((h, w), F32)]
            clip = _mul(Pp, _mul(Vp, P))
            fx = ((clip[0] / clip[3]) * F32(0.5) + F32(0.5)) * F32(w) - F32(0.5)
            fy = ((clip[1] / clip[3]) * F32(0.5) + F32(0.5)) * F32(h) - F32(0.5)
            front = valid & (clip[3] > 0)
            sx, sy = fx - xs.astype(F32), fy - ys.astype(F32)
            screen = np.where(front[..., None], np.stack([sx, sy, np.ones((h, w), F32)], -1), F32(0))
            have = front & (fx >= F32(-1)) & (fx < F32(w)) & (fy >= F32(-1)) & (fy < F32(h))
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
                    ok &= state["valid"][qy, qx]
                    ok &= _dot(state["normal"][qy, qx], n) >= F32(T["normal_cos"])
                    d = pp - state["position"][qy, qx]
                    ok &= np.abs(_dot(d, n)) <= lim
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
        t = np.where(v3, t, c)
        m1, m2, N, var = (np.where(valid, q, F32(0)) for q in (m1, m2, N, var))
        reprojected, reset = int((valid & accepted).sum()), int((valid & ~accepted).sum())
        moved = int((valid & (pp != pos).any(-1)).sum())

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
               "variance": var, "reprojected": reprojected, "reset": reset, "moved": moved,
               "prev_position": np.where(v3, pp, F32(0)), "screen": screen, "accepted": valid & accepted}

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
    for k in ("length", "moments", "variance", "color", "color_variance", "prev_position", "screen"):
        assert new[k].dtype == F32, k
    assert out.dtype == F32
    return out, new
