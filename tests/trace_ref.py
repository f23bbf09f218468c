"""A float64 reference for traced hits, and the contract a traced result is held to.

Pure numpy: no GPU and no oracle import.  The oracle and the kernels share one hit rule by design
(fp32 Moller-Trumbore, then tri_accept: t brought into the slab interval of the triangle's own padded box),
so comparing one with the other says nothing about whether the rule finds the triangle the ray
actually hits.  This module asks that question of either of them.

Reference
    exact_hits(tris, rays): Moller-Trumbore in float64 over every (ray, triangle) pair, on the fp32
    vertices and rays as given (widened, nothing re-derived from float64 scene data):

        e1 = v1 - v0,  e2 = v2 - v0,  tv = o - v0,  p = d x e2,  q = tv x e1,  det = e1 . p
        u = (tv . p) / det,  v = (d . q) / det,  t = (e2 . q) / det,  m = min(u, v, 1 - u - v)

    m is the inside-margin: the ray hits the triangle iff m >= 0.

Bound
    bound_x = C * 2^-24 * cond_x for x in (u, v, m, t): a forward-error bound of the fp32 evaluation
    of the expressions above (pt_oracle.c tri_hit, pt_device.h tri_test; no contraction assumed, a
    fused multiply-add only removes a rounding).  With U = 2^-24 and |a| (x) |b| the cross product of
    the absolute values with every term added (P_x = |d_y e2_z| + |d_z e2_y|, ...):

        P = |d| (x) |e2|        Q = |tv| (x) |e1|        D = |e1| . P
        cond_u = (|tv| . P) / |det| + |u| (D / |det| + 1)
        cond_v = (|d|  . Q) / |det| + |v| (D / |det| + 1)
        cond_m = cond_u + cond_v + |u + v|
        cond_t = ((|e2| . Q) / |det| + |t| (D / |det| + 1)) / |t|        (relative to |t|)

    The inputs are fp32 numbers, so every subtraction of two of them (e1, e2, tv) carries ONE
    relative rounding and no term in |o| or |v0|: the bound does not grow when the scene moves away
    from the origin, only the acceptance pad does.  The roundings, per chain:

        p  = d x e2      e2 (1), product (1), difference (1)                            3 U P
        q  = tv x e1     tv (1), e1 (1), product (1), difference (1)                    4 U Q
        det = e1 . p     e1 (1), p (3), product (1), two sums (2)                       7 U D
        tv . p           tv (1), p (3), product (1), two sums (2)                       7 U |tv| . P
        d . q            q (4), product (1), two sums (2)                               7 U |d| . Q
        e2 . q           e2 (1), q (4), product (1), two sums (2)                       8 U |e2| . Q
        x = num * (1 / det)   reciprocal (1), product (1), det's own error (7 U D / |det|)
        u + v <= 1       one more sum (1 U |u + v|)

    No chain has more than eight, so C = 8.  It comes from this count and is not tuned.  The
    first-order term D / |det| is taken exactly, as eps / (1 - eps) with eps = C U D / |det|: where
    eps >= 1 fp32 cannot tell the sign of det (the ray lies in the triangle's plane to rounding), the
    bound is infinite and nothing is asked of that pair.  det = 0 with D = 0 (an axis-parallel ray in
    an axis-aligned wall's plane) is a certain miss in fp32 too and is treated as one, and so is every
    triangle without area (the exact cross product of its edges is zero), which must never come back.

    Measured worst ratios error / (2^-24 cond), i.e. the C each clause would need, over every
    committed ray set of every variant below (tests/test_trace_geometry.py prints them with -s):

        oracle:   u 1.70   v 2.18   t 1.61   returned triangle outside by 0.96
                  nearer real triangle skipped while inside by 0.50

    So C is 3.7 times the worst measured error.  Before tri_accept clamped t instead of rejecting it the
    `slivers` variant skipped a triangle while inside by 101.8 (test_trace_geometry.py).  The kernels
    return the oracle's bits on the same sets on all four builders (tests/test_gpu_trace_geometry.py),
    so their ratios are the same numbers.

Contract, per ray, for a result (prim g, t, u, v, backface)
    1. Nothing real is skipped: no triangle j with m_j > bound_m_j and t_j certainly inside
       [tmin, tmax] has t_j nearer than the returned t by more than the two t bounds.  A miss counts
       as t = +inf.
    2. The returned triangle is real: m_g >= -bound_m_g, |t - t_g| <= bound_t_g |t_g|, u and v within
       bound_u_g / bound_v_g of the float64 u, v, backface == (det_g < 0), tmin <= t <= tmax.  A
       triangle without area is never returned.
    3. Ties go to the lowest index: of coplanar duplicates (bit-equal vertices) the lowest global
       index is the one returned.
    4. Any-hit says hit when some triangle has m > bound_m certainly in range, and miss when none
       has m >= -bound_m possibly in range.

    A ray is left out of a clause when the clause cannot be decided for it: the pair it hinges on has
    an infinite bound (|det| under its own rounding) or a t within its bound of tmin or tmax.
    Float64's own rounding, 2^-40 cond, is added to every bound and leaves no ray out.  check_* report
    the share left out per clause and the callers assert it is at most MAX_UNDECIDED.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -24
C = 8.0
F64_FLOOR = 2.0 ** -40   # in units of cond: below it float64's own rounding decides
MAX_UNDECIDED = 0.01
CLAUSES = ("skipped", "returned", "ties", "any_hit", "any_miss")


# -- the float64 reference --------------------------------------------------------------------------
def _abs_cross(a, b):
    """|a| (x) |b| with every term added."""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _exact_chunk(tris, rays):
    o = rays[:, None, 0:3]
    d = rays[:, None, 3:6]
    v0 = tris[None, :, 0]
    e1 = (tris[:, 1] - tris[:, 0])[None]
    e2 = (tris[:, 2] - tris[:, 0])[None]
    tv = o - v0
    p = np.cross(d, e2)
    q = np.cross(tv, e1)
    det = _dot(e1, p)
    P = _abs_cross(d, e2)
    Q = _abs_cross(tv, e1)
    D = _dot(np.abs(e1), P)
    with np.errstate(all="ignore"):
        u = _dot(tv, p) / det
        v = _dot(d, q) / det
        t = _dot(e2, q) / det
        ad = np.abs(det)
        eps = C * U * D / ad
        # the det term: first order D/|det|, taken exactly as eps / (1 - eps) / (C U)
        dterm = np.where(eps < 1.0, D / ad / (1.0 - eps), np.inf)
        cu = _dot(np.abs(tv), P) / ad + np.abs(u) * (dterm + 1.0)
        cv = _dot(np.abs(d), Q) / ad + np.abs(v) * (dterm + 1.0)
        cm = cu + cv + np.abs(u + v)
        cta = _dot(np.abs(e2), Q) / ad + np.abs(t) * (dterm + 1.0)  # absolute: cond_t |t|, finite at t = 0
        ct = cta / np.abs(t)
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
    # det == 0 with D == 0: every fp32 product is an exact zero too, a certain miss on both sides
    flat = (D == 0.0) | no_area(tris)[None]
    m = np.where(flat, -np.inf, m)
    t = np.where(flat, np.inf, t)
    for c in (cu, cv, cm, ct, cta):
        c[flat] = 0.0
        c[np.isnan(c)] = np.inf
    m = np.where(np.isnan(m), -np.inf, m)  # 0/0 with D > 0: bound infinite, nothing asked
    return dict(t=t, u=u, v=v, det=det, m=m, cond_u=cu, cond_v=cv, cond_m=cm, cond_t=ct, cond_t_abs=cta)


def exact_hits(tris_f32, rays_f32, chunk=256):
    """Every (ray, triangle) pair in float64.

    tris_f32 (T, 3, 3): v0, v1, v2 as the tracer holds them (fp32 values; float64 arrays of widened
    values are taken as they are).  rays_f32 (R, 8): origin, direction, tmin, tmax.  Returns a dict
    of (R, T) float64 arrays: t, u, v, det, m and cond_u, cond_v, cond_m, cond_t, cond_t_abs = cond_t |t| (module
    docstring; bound_x = C * 2^-24 * cond_x)."""
    tris = np.asarray(tris_f32, np.float64).reshape(-1, 3, 3)
    rays = np.asarray(rays_f32, np.float64).reshape(-1, 8)
    parts = [_exact_chunk(tris, rays[i:i + chunk]) for i in range(0, len(rays), chunk)]
    if not parts:
        return {k: np.zeros((0, len(tris))) for k in ("t", "u", "v", "det", "m", "cond_u", "cond_v", "cond_m", "cond_t", "cond_t_abs")}
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def bound(cond):
    """C 2^-24 cond, plus float64's own rounding of the reference (2^-40 cond) on the lenient side."""
    return (C * U + F64_FLOOR) * cond


def no_area(tris):
    """(T,) bool: the exact cross product of the edges is zero (zero-area and collinear triangles)."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return ~n.any(axis=1)


def duplicate_leader(tris_f32):
    """(T,) int: the lowest index among the triangles whose nine fp32 vertex words equal this one's."""
    t = np.ascontiguousarray(np.asarray(tris_f32, np.float32).reshape(-1, 9))
    first = {}
    out = np.empty(len(t), np.int64)
    for i, row in enumerate(t):
        out[i] = first.setdefault(row.tobytes(), i)
    return out


# -- the contract -----------------------------------------------------------------------------------
@dataclass
class Report:
    """What one check found: violations per clause (ray indices with a sentence each), the share of
    rays left out per clause, and the worst error / (2^-24 cond) ratios seen."""
    n: int = 0
    violations: dict = field(default_factory=lambda: {c: [] for c in CLAUSES})
    left_out: dict = field(default_factory=lambda: {c: 0 for c in CLAUSES})
    ratios: dict = field(default_factory=lambda: dict(skipped_inside=0.0, returned_outside=0.0, t=0.0, u=0.0, v=0.0))
    passed_between: int = 0  # rays whose float64 nearest hit was not the one returned (within bounds)

    def share(self, clause):
        return self.left_out[clause] / max(1, self.n)

    def merge(self, other, offset=0):
        self.n += other.n
        for c in CLAUSES:
            self.violations[c] += [(i + offset, s) for i, s in other.violations[c]]
            self.left_out[c] += other.left_out[c]
        for k, x in other.ratios.items():
            self.ratios[k] = max(self.ratios[k], x)
        self.passed_between += other.passed_between

    def ok(self):
        return not any(self.violations.values())

    def describe(self, limit=5):
        out = []
        for c in CLAUSES:
            v = self.violations[c]
            if v:
                out.append(f"clause '{c}': {len(v)} of {self.n} rays, e.g. " + "; ".join(f"ray {i}: {s}" for i, s in v[:limit]))
        return "\n".join(out) or "no violations"


def _in_range(E, rays):
    """(certainly, possibly) inside [tmin, tmax], per pair, by the pair's own t bound."""
    tmin, tmax = rays[:, 6:7].astype(np.float64), rays[:, 7:8].astype(np.float64)
    with np.errstate(all="ignore"):
        bt = bound(E["cond_t_abs"])
        sure = (E["t"] - bt > tmin) & (E["t"] + bt < tmax)
        maybe = (E["t"] + bt >= tmin) & (E["t"] - bt <= tmax)
    return sure, maybe, bt


CULL_ABOVE = 2048  # triangles: scenes up to this size are always checked exhaustively


def _candidates(tris, rays, keep=(), cull=True):
    """Indices of the triangles whose bounding sphere (radius x 1.5) the line of some ray of the chunk
    passes, plus `keep`.  The others are certain misses in float64 (m < 0), so no clause can ask for
    them; leaving them out only makes 'any_miss' stricter.  Used above CULL_ABOVE triangles only (the
    250k-triangle scene of test_gpu_determinism); test_trace_geometry holds it to the un-culled pass."""
    if not cull or len(tris) <= CULL_ABOVE:
        return np.arange(len(tris))
    c = tris.mean(axis=1)
    r2 = 2.25 * ((tris - c[:, None]) ** 2).sum(axis=2).max(axis=1)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    wd = c @ d.T - (o * d).sum(axis=1)                                        # (T, R): (c - o) . d
    w2 = (c * c).sum(axis=1)[:, None] - 2.0 * (c @ o.T) + (o * o).sum(axis=1)  # |c - o|^2
    near = (w2 - wd * wd <= r2[:, None] + 1e-9 * w2).any(axis=1)
    near[np.asarray(keep, np.int64)] = True
    return np.nonzero(near)[0]


def check_closest(tris, rays, result, chunk=32, cull=True):
    """Clauses 1-3 for a closest-hit result (prim, t, u, v, backface) -> Report."""
    tris64 = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    flat = no_area(tris64)
    leader = duplicate_leader(tris)
    prim, t, u, v, back = (np.asarray(x) for x in result)
    rep = Report()
    for i0 in range(0, len(rays), chunk):
        sl = slice(i0, i0 + chunk)
        ids = _candidates(tris64, rays[sl], prim[sl][prim[sl] >= 0], cull)
        local = np.where(prim[sl] >= 0, np.searchsorted(ids, np.maximum(prim[sl], 0)), -1)
        rep.merge(_check_closest_chunk(tris64[ids], flat[ids], ids, rays[sl], local, t[sl], u[sl], v[sl], back[sl]), i0)
    # clause 3: of bit-equal duplicates the lowest index comes back
    for i in np.nonzero(prim >= 0)[0]:
        j = int(prim[i])
        if leader[j] != j:
            rep.violations["ties"].append((int(i), f"triangle {j} returned, its bit-equal duplicate {int(leader[j])} has the lower index"))
    return rep


def _check_closest_chunk(tris, flat, ids, rays, prim, t, u, v, back):
    E = _exact_chunk(tris, rays.astype(np.float64))
    n = len(rays)
    rep = Report(n=n)
    ar = np.arange(n)
    hit = prim >= 0
    g = np.where(hit, prim, 0)
    sure, maybe, bt = _in_range(E, rays)
    bm = bound(E["cond_m"])
    tret = np.where(hit, t.astype(np.float64), np.inf)
    btg = np.where(hit, bt[ar, g], 0.0)

    # clause 2: the returned triangle is real
    for i in np.nonzero(hit)[0]:
        j = int(g[i])
        if flat[j]:
            rep.violations["returned"].append((int(i), f"triangle {int(ids[j])} has no area"))
            continue
        if not np.isfinite(bm[i, j]) or not np.isfinite(bt[i, j]):
            rep.left_out["returned"] += 1
            continue
        why = []
        cm, ctj = E["cond_m"][i, j], E["cond_t_abs"][i, j]
        if not rays[i, 6] <= t[i] <= rays[i, 7]:
            why.append(f"t {t[i]!r} outside [{rays[i, 6]!r}, {rays[i, 7]!r}]")
        if E["m"][i, j] < -bm[i, j]:
            why.append(f"triangle {int(ids[j])} is missed in float64: m {E['m'][i, j]:.3e} < -bound {bm[i, j]:.3e}")
        et = abs(float(t[i]) - E["t"][i, j])
        if et > bt[i, j]:
            why.append(f"t {t[i]!r} vs float64 {E['t'][i, j]!r}: off by {et:.3e} > bound {bt[i, j]:.3e}")
        eu, ev = abs(float(u[i]) - E["u"][i, j]), abs(float(v[i]) - E["v"][i, j])
        bu, bv = bound(E["cond_u"][i, j]), bound(E["cond_v"][i, j])
        if eu > bu or ev > bv:
            why.append(f"(u, v) off by ({eu:.3e}, {ev:.3e}) > bounds ({bu:.3e}, {bv:.3e})")
        if bool(back[i]) != bool(E["det"][i, j] < 0):
            why.append(f"backface {int(back[i])} but float64 det {E['det'][i, j]:.3e}")
        if why:
            rep.violations["returned"].append((int(i), "; ".join(why)))
        with np.errstate(all="ignore"):
            rep.ratios["returned_outside"] = max(rep.ratios["returned_outside"], -E["m"][i, j] / (U * cm))
            rep.ratios["t"] = max(rep.ratios["t"], et / (U * ctj))
            rep.ratios["u"] = max(rep.ratios["u"], eu / (U * E["cond_u"][i, j]))
            rep.ratios["v"] = max(rep.ratios["v"], ev / (U * E["cond_v"][i, j]))

    # clause 1: nothing real is skipped
    with np.errstate(all="ignore"):
        nearer = E["t"] + bt + btg[:, None] < tret[:, None]
        bad = (E["m"] > bm) & sure & nearer
        # left out: a triangle that is real by its bound and nearer, but within its t bound of tmin / tmax
        vague = (E["m"] > bm) & maybe & ~sure & nearer
    inf_ret = hit & ~np.isfinite(btg)
    for i in range(n):
        if inf_ret[i] or (vague[i].any() and not bad[i].any()):
            rep.left_out["skipped"] += 1
            continue
        js = np.nonzero(bad[i])[0]
        if len(js):
            j = int(js[np.argmin(E["t"][i, js])])
            got = f"triangle {int(ids[prim[i]])} at t {t[i]!r}" if hit[i] else "a miss"
            rep.violations["skipped"].append(
                (i, f"triangle {int(ids[j])} is hit in float64 at t {E['t'][i, j]!r} with m {E['m'][i, j]:.3e} > bound "
                    f"{bm[i, j]:.3e}, but the trace returned {got}"))
    # how far inside a skipped nearer triangle was, in units of 2^-24 cond (the C clause 1 would need)
    with np.errstate(all="ignore"):
        inside = (E["m"] > 0) & sure & nearer & np.isfinite(E["cond_m"]) & (E["cond_m"] > 0)
        if inside.any():
            rep.ratios["skipped_inside"] = float((E["m"][inside] / (U * E["cond_m"][inside])).max())
        # rays that "pass between": float64 has a hit (m >= 0, in range) nearer than what came back
        rep.passed_between = int((((E["m"] >= 0) & sure & nearer).any(axis=1) & ~inf_ret).sum())

    return rep


def check_any(tris, rays, hit, chunk=32, cull=True):
    """Clause 4 for an any-hit answer (bool per ray) -> Report."""
    tris64 = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    hit = np.asarray(hit, bool)
    rep = Report()
    for i0 in range(0, len(rays), chunk):
        r = rays[i0:i0 + chunk]
        ids = _candidates(tris64, r, cull=cull)
        E = _exact_chunk(tris64[ids], r.astype(np.float64))
        sure, maybe, _ = _in_range(E, r)
        bm = bound(E["cond_m"])
        must = ((E["m"] > bm) & sure).any(axis=1)
        with np.errstate(all="ignore"):
            may = ((E["m"] >= -bm) & maybe).any(axis=1)
        h = hit[i0:i0 + chunk]
        part = Report(n=len(r))
        for i in np.nonzero(must & ~h)[0]:
            j = int(np.argmax((E["m"] > bm)[i] & sure[i]))
            part.violations["any_hit"].append((int(i), f"says miss, triangle {int(ids[j])} is hit in float64 at t {E['t'][i, j]!r} with m {E['m'][i, j]:.3e} > bound {bm[i, j]:.3e}"))
        for i in np.nonzero(~may & h)[0]:
            part.violations["any_miss"].append((int(i), "says hit, no triangle has m >= -bound in range in float64"))
        # Left out: the answer is "hit", no triangle with a finite bound can explain it, and one with an
        # infinite bound or a t within its bound of tmin / tmax might.  (A ray whose candidates lie
        # within bound_m of an edge is not left out: fp32 may answer it either way, and both pass.)
        with np.errstate(all="ignore"):
            explained = ((E["m"] >= -bm) & maybe & np.isfinite(bm) & sure).any(axis=1)
        part.left_out["any_miss"] = int((h & may & ~explained).sum())
        rep.merge(part, i0)
    return rep


def assert_contract(tris, rays, closest, any_hit, who, chunk=32):
    """Assert clauses 1-4 and the undecided cap for one tracer's answers on one ray set; prints the
    worst ratios and returns the closest-hit report."""
    rep = check_closest(tris, rays, closest, chunk)
    anyrep = check_any(tris, rays, any_hit, chunk)
    print(f"{who}: ratios " + " ".join(f"{k}={x:.3f}" for k, x in rep.ratios.items())
          + f" passed_between={rep.passed_between}/{rep.n} left_out "
          + " ".join(f"{c}={max(rep.share(c), anyrep.share(c)):.4f}" for c in CLAUSES))
    assert rep.ok(), f"{who} breaks the float64 contract:\n{rep.describe()}"
    assert anyrep.ok(), f"{who} (any-hit) breaks the float64 contract:\n{anyrep.describe()}"
    for c in CLAUSES:
        share = max(rep.share(c), anyrep.share(c))
        assert share <= MAX_UNDECIDED, f"{who}: clause '{c}' leaves out {share:.2%} of the rays"
    return rep
