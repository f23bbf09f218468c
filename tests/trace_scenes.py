"""Adversarial scenes and ray sets for the traced-hit contract (tests/trace_ref.py).

Seeded and generated, never stored.  Every variant is a product `Scene` (so the oracle, the kernels
and the renderers all take it) of at most 2000 triangles, with one light and a camera inside the box
for the render tests, plus the ray sets that go with it.  `world_triangles` gives the fp32 triangles
the tracers hold: the mesh vertices through the model matrix in the oracle's documented fp32 product
(a0 + a1) + (a2 + a3).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import trace_ref

VARIANTS = ("unit", "far", "tiny", "huge", "model", "slivers", "aligned", "coplanar", "degenerate")
RAY_SETS = ("interior", "edges", "leaving", "inplane", "ranges", "axis")
N_RAYS = 1200
FAR = np.array([1000.0, -2000.0, 500.0])
MODEL_SCALE = np.array([1.5, 0.75, 2.0])
F = np.float32


# -- geometry (float64 until the end) ---------------------------------------------------------------
def icosphere(subdiv=2, radius=0.5):
    """320 triangles at subdiv 2, 1280 at 3; outward CCW."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid = {}

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        f = [t for a, b, c in f for t in ((a, m(a, b), m(c, a)), (b, m(b, c), m(a, b)), (c, m(c, a), m(b, c)),
                                          (m(a, b), m(b, c), m(c, a)))]
    v = np.array(v)
    return v * radius, v.copy(), np.array(f, np.int32)


def box(h=1.5):
    """12 triangles, a closed cube of half-side h, inward normals, four vertices of its own per face."""
    vs, ns, idx = [], [], []
    for a in range(3):
        for s in (-1.0, 1.0):
            b, c = (a + 1) % 3, (a + 2) % 3
            q = np.zeros((4, 3))
            q[:, a] = s * h
            q[:, b] = [-h, h, h, -h]
            q[:, c] = [-h, -h, h, h]
            n = np.zeros(3)
            n[a] = -s
            k = len(vs) * 4
            vs.append(q)
            ns.append(np.tile(n, (4, 1)))
            # wound so that the geometric normal is the inward one
            idx += [(k, k + 1, k + 2), (k, k + 2, k + 3)] if np.cross(q[1] - q[0], q[2] - q[0]) @ n > 0 else \
                   [(k, k + 2, k + 1), (k, k + 3, k + 2)]
    return np.concatenate(vs), np.concatenate(ns), np.array(idx, np.int32)


def free_quads(rng, n=3):
    vs, ns, idx = [], [], []
    for k in range(n):
        c = rng.normal(size=3)
        c = c / np.linalg.norm(c) * rng.uniform(0.8, 1.2)  # between the sphere and the walls
        a = np.cross(rng.normal(size=3), c)
        a /= np.linalg.norm(a)
        b = np.cross(c, a)
        b /= np.linalg.norm(b)
        a, b = a * rng.uniform(0.2, 0.4), b * rng.uniform(0.2, 0.4)
        nrm = np.cross(a, b)
        vs.append(np.array([c - a - b, c + a - b, c + a + b, c - a + b]))
        ns.append(np.tile(nrm / np.linalg.norm(nrm), (4, 1)))
        idx += [(4 * k, 4 * k + 1, 4 * k + 2), (4 * k, 4 * k + 2, 4 * k + 3)]
    return np.concatenate(vs), np.concatenate(ns), np.array(idx, np.int32)


def slivers(rng, n=200, aspect=1e4):
    """n triangles of long edge 0.5..1 and height long / aspect, at random orientations and places."""
    vs, idx = [], []
    for k in range(n):
        c = rng.uniform(-1.0, 1.0, 3)
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        b = np.cross(a, rng.normal(size=3))
        b /= np.linalg.norm(b)
        L = rng.uniform(0.5, 1.0)
        vs.append(np.array([c - 0.5 * L * a, c + 0.5 * L * a, c + rng.uniform(-0.4, 0.4) * L * a + (L / aspect) * b]))
        idx.append((3 * k, 3 * k + 1, 3 * k + 2))
    v = np.concatenate(vs)
    n_ = np.repeat(np.cross(v[1::3] - v[0::3], v[2::3] - v[0::3]), 3, axis=0)
    return v, n_ / np.linalg.norm(n_, axis=1, keepdims=True), np.array(idx, np.int32)


def aligned_walls():
    """Axis-aligned rectangles at dyadic coordinates inside the box, two per axis."""
    vs, ns, idx = [], [], []
    k = 0
    for a in range(3):
        for pos, lo, hi in ((0.5, -0.75, 0.25), (-0.625, -0.5, 1.0)):
            b, c = (a + 1) % 3, (a + 2) % 3
            q = np.zeros((4, 3))
            q[:, a] = pos
            q[:, b] = [lo, hi, hi, lo]
            q[:, c] = [lo, lo, hi, hi]
            n = np.zeros(3)
            n[a] = 1.0
            vs.append(q)
            ns.append(np.tile(n, (4, 1)))
            idx += [(k, k + 1, k + 2), (k, k + 2, k + 3)]
            k += 4
    return np.concatenate(vs), np.concatenate(ns), np.array(idx, np.int32)


def coplanar_stack(rng):
    """In each of three tilted planes: a quad split along one diagonal, the same quad split along the
    other (overlapping coplanar triangles), a smaller triangle inside, and bit-equal duplicates of some
    of them at higher indices."""
    vs, idx = [], []
    for k in range(3):
        c = rng.uniform(-0.8, 0.8, 3)
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        b = np.cross(a, rng.normal(size=3))
        b /= np.linalg.norm(b)
        a, b = 0.5 * a, 0.5 * b
        q = np.array([c - a - b, c + a - b, c + a + b, c - a + b, c - 0.3 * a - 0.2 * b, c + 0.3 * a - 0.2 * b, c + 0.3 * b])
        base = len(vs) * 7
        vs.append(q)
        t = [(0, 1, 2), (0, 2, 3), (0, 1, 3), (1, 2, 3), (4, 5, 6)]
        t += [t[0], t[4], t[2], t[0]]  # bit-equal duplicates, the first one twice
        idx += [tuple(base + i for i in tri) for tri in t]
    v = np.concatenate(vs)
    idx = np.array(idx, np.int32)
    n = np.zeros_like(v)
    fn = np.cross(v[idx[:, 1]] - v[idx[:, 0]], v[idx[:, 2]] - v[idx[:, 0]])
    for j in range(3):
        n[idx[:, j]] = fn / np.linalg.norm(fn, axis=1, keepdims=True)
    return v, n, idx


def degenerates(sphere_v):
    """Zero-area and collinear triangles where rays go: on sphere vertices, on a wall, in free space.
    Coordinates are dyadic so that the edges' cross product is exactly zero."""
    p = np.round(sphere_v[:6] * 64.0) / 64.0
    e = np.array([0.25, -0.125, 0.5])
    tris = []
    for q in p[:3]:
        tris.append([q, q, q])                  # a point
    for q in p[3:6]:
        tris.append([q, q + e, q])              # two equal vertices
    for q in (np.array([-1.5, 0.25, -0.5]), np.array([0.5, 0.25, -0.25]), np.array([0.0, -1.5, 0.75])):
        tris.append([q, q + e, q + 2.0 * e])    # collinear
        tris.append([q + 0.5 * e, q - e, q])    # collinear, middle vertex last
    v = np.array(tris).reshape(-1, 3)
    idx = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    n = np.tile([0.0, 1.0, 0.0], (len(v), 1))
    return v, n, idx


# -- scenes -----------------------------------------------------------------------------------------
def _parts(name, rng):
    sph, wall = icosphere(2), box()
    if name == "slivers":
        return [slivers(rng), wall]
    if name == "aligned":
        return [aligned_walls(), wall]
    if name == "coplanar":
        return [coplanar_stack(rng), wall]
    if name == "degenerate":
        return [coplanar_stack(rng), degenerates(sph[0]), sph, wall, slivers(rng, 20)]
    return [sph, wall, free_quads(rng)]


def _model_matrix(scale, translate):
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[3, 3] = scale[0], scale[1], scale[2], 1.0
    m[:3, 3] = translate
    return m.astype(F).reshape(-1, order="F")


@lru_cache(maxsize=None)
def make(name):
    """(scene, scale, centre): the variant as a product Scene; scale and centre (float64, world space)
    place the ray sets, the camera and the light."""
    from optixpathtracer_amd.scenes import Mesh, Scene

    if name not in VARIANTS:
        raise ValueError(name)
    rng = np.random.default_rng(1000 + VARIANTS.index(name))
    s = {"tiny": 1e-3, "huge": 1e3}.get(name, 1.0)
    centre = FAR.copy() if name in ("far", "model") else np.zeros(3)
    axes = MODEL_SCALE if name == "model" else np.ones(3)
    meshes = []
    cols = [(0.6, 0.1, 0.1), (0.5, 0.5, 0.5), (0.1, 0.4, 0.1), (0.1, 0.1, 0.5), (0.4, 0.4, 0.1)]
    for k, (v, n, idx) in enumerate(_parts(name, rng)):
        if name == "model":
            model = _model_matrix(MODEL_SCALE, FAR)
        else:
            v = v * s + centre  # baked into the fp32 vertices
            model = _model_matrix(np.ones(3), np.zeros(3))
        meshes.append(Mesh(vertices=np.ascontiguousarray(v, F), normals=np.ascontiguousarray(n, F),
                           indices=np.ascontiguousarray(idx, np.int32), model=model, albedo=cols[k % len(cols)],
                           metallic=0.0, roughness=0.4, name=f"{name}_{k}"))
    # looks along -x from just under the ceiling: path rays end at t = 100, and in `huge` only the
    # ceiling is that near
    eye = centre + axes * s * np.array([1.3, 1.49, 0.3])
    light = centre + axes * s * np.array([0.9, 1.1, -0.7])
    power = 2.0 * s * s
    sc = Scene(meshes=meshes, lights=np.array([[*light, power, power, power]], F),
               camera_blender_pos=(eye[0], -eye[2], eye[1]), camera_blender_rot=(90.0, 0.0, 90.0),
               material_mode=1, name=f"trace_{name}")
    assert sc.n_triangles <= 2000
    return sc, s * axes, centre


def world_triangles(scene):
    """(T, 3, 3) float32, meshes concatenated: model * (v, 1) as the oracle documents it, every row
    (a0 + a1) + (a2 + a3) in fp32."""
    out = []
    for m in scene.meshes:
        v = np.asarray(m.vertices, F)
        M = np.asarray(m.model, F).reshape(-1)
        w = np.empty_like(v)
        for r in range(3):
            a0, a1, a2, a3 = M[0 + r] * v[:, 0], M[4 + r] * v[:, 1], M[8 + r] * v[:, 2], M[12 + r] * F(1.0)
            w[:, r] = (a0 + a1) + (a2 + a3)
        out.append(w[np.asarray(m.indices)])
    return np.concatenate(out)


def record_triangles(tri_records):
    """(T, 3, 3) float64 by global index from the leaf-ordered device records (OptixRenderer.bvh_arrays:
    v0 | e1 | e2 as fp32 words, word 3 the global index): v0, v0 + e1, v0 + e2, as the kernels' hit test
    sees them."""
    w = np.ascontiguousarray(tri_records, np.uint32)
    f = w.view(F).astype(np.float64)
    gi = w[:, 3].view(np.int32)
    out = np.empty((len(w), 3, 3))
    out[gi, 0] = f[:, 0:3]
    out[gi, 1] = f[:, 0:3] + f[:, 4:7]
    out[gi, 2] = f[:, 0:3] + f[:, 8:11]
    return out


# -- ray sets ---------------------------------------------------------------------------------------
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _pack(o, d, tmin, tmax):
    r = np.zeros((len(o), 8), F)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, tmin, tmax
    return r


def _tri_points(rng, T, k, kind):
    """k points on random triangles of T with area: 'in' interior, 'edge' on an edge, 'vert' a vertex."""
    ok = np.nonzero(~trace_ref.no_area(T))[0]
    ti = ok[rng.integers(0, len(ok), k)]
    w = rng.dirichlet([1.0, 1.0, 1.0], k)
    if kind == "edge":
        w[np.arange(k), rng.integers(0, 3, k)] = 0.0
        w /= w.sum(axis=1, keepdims=True)
    elif kind == "vert":
        w = np.eye(3)[rng.integers(0, 3, k)]
    return ti, np.einsum("ij,ijk->ik", w, T[ti])


def _normals(T, ti):
    n = np.cross(T[ti, 1] - T[ti, 0], T[ti, 2] - T[ti, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _inside(rng, k, scale, centre, r=1.4):
    return centre + scale * rng.uniform(-r, r, (k, 3))


def _interior(rng, T, scale, centre, n):
    o = _inside(rng, n, scale, centre)
    d = rng.normal(size=(n, 3))
    k = 2 * n // 3
    d[:k] = _tri_points(rng, T, k, "in")[1] - o[:k]
    return _pack(o, _unit(d), 0.0, 100.0 * scale.max())


def _edges(rng, T, scale, centre, n):
    """Aimed at edges and vertices: grazing from nearby, and from 40 to 95 scene units away."""
    k = n // 2
    ti, p = _tri_points(rng, T, n, "edge")
    ti[::4], p[::4] = _tri_points(rng, T, len(ti[::4]), "vert")
    nrm = _normals(T, ti)  # used by the grazing half only
    tng = _unit(np.cross(nrm, rng.normal(size=(n, 3))))
    c = rng.uniform(1e-3, 0.08, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    d = c * nrm + np.sqrt(1.0 - c * c) * tng
    dist = rng.uniform(0.05, 0.9, (n, 1)) * scale.min()
    far = _unit(rng.normal(size=(n - k, 3)))
    d[k:] = far
    dist[k:] = rng.uniform(40.0, 95.0, (n - k, 1)) * scale.max()
    # far rays are aimed at the outer shell: the box's own edges and vertices
    lo, hi = T.reshape(-1, 3).min(axis=0), T.reshape(-1, 3).max(axis=0)
    shell = np.nonzero(((T == lo) | (T == hi)).any(axis=2).all(axis=1))[0]
    if len(shell):
        p[k:] = _tri_points(rng, T[shell], n - k, "edge")[1]  # ti, nrm, tng no longer go with these
    return _pack(p - dist * d, d, 0.0, 200.0 * scale.max())


def _leaving(rng, T, scale, centre, n):
    """Origins nudged 1e-4 .. 1e-1 scene units off a triangle along its normal; random directions, a
    third of them aimed at a point next to the nearest edge (into the adjacent corner: t << |o|)."""
    ti, p = _tri_points(rng, T, n, "in")
    nrm = _normals(T, ti) * rng.choice([-1.0, 1.0], (n, 1))
    nudge = 10.0 ** rng.uniform(-4.0, -1.0, (n, 1)) * scale.min()
    d = _unit(rng.normal(size=(n, 3)))
    k = n // 3
    te, pe = _tri_points(rng, T, k, "edge")
    ne = _normals(T, te) * rng.choice([-1.0, 1.0], (k, 1))
    w = rng.uniform(1e-3, 1e-1, (k, 1))
    cen = T[te].mean(axis=1)
    p[:k] = pe + w * (cen - pe)         # just inside the triangle, next to the edge
    nrm[:k] = ne
    o = p + nudge * nrm
    tgt = pe + nudge[:k] * _unit(rng.normal(size=(k, 3)))
    d[:k] = _unit(tgt - o[:k])
    return _pack(o, d, 0.0, 100.0 * scale.max())


def _inplane(rng, T, scale, centre, n):
    """Origin in a triangle's plane, aimed across the triangle: one ray in twenty lies in the plane (to fp32
    rounding; fp32 cannot place such a hit and the contract leaves out the rays that return it), the
    others are tilted out of it by 1e-5 .. 1e-2 radians."""
    ti, p = _tri_points(rng, T, n, "in")
    e1, e2 = T[ti, 1] - T[ti, 0], T[ti, 2] - T[ti, 0]
    ab = rng.uniform(1.2, 3.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))  # outside the edges' parallelogram
    o = T[ti, 0] + ab[:, :1] * e1 + ab[:, 1:] * e2
    tilt = np.where(np.arange(n)[:, None] % 20 == 0, 0.0, 10.0 ** rng.uniform(-5.0, -2.0, (n, 1)))
    d = _unit(p - o) + tilt * rng.choice([-1.0, 1.0], (n, 1)) * _normals(T, ti)
    return _pack(o, _unit(d), 0.0, 100.0 * scale.max())


def _axis(rng, T, scale, centre, n):
    """Axis-parallel rays, the other components +0 or -0: half aimed at triangle points (interior, edge,
    vertex) along an axis, half lying in the plane of an axis-aligned wall (origin on the plane's
    coordinate exactly)."""
    k = n // 2
    parts = [_tri_points(rng, T, k // 3, "in"), _tri_points(rng, T, k // 3, "edge"),
             _tri_points(rng, T, k - 2 * (k // 3), "vert")]
    tgt = np.concatenate([p for _, p in parts]).astype(F)
    axis = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    d = np.where(rng.random((n, 3)) < 0.5, F(-0.0), F(0.0)).astype(F)
    d[np.arange(n), axis] = sign
    o = np.empty((n, 3), F)
    o[:k] = tgt
    o[np.arange(k), axis[:k]] -= (sign[:k] * rng.uniform(0.1, 3.0, k) * scale[axis[:k]]).astype(F)
    # in-plane: triangles constant in one coordinate; the ray runs along another axis through the plane
    flat = [(j, a) for a in range(3) for j in np.nonzero((T[:, :, a] == T[:, :1, a]).all(axis=1))[0]]
    for i in range(k, n):
        if not flat:
            o[i] = _inside(rng, 1, scale, centre)[0]
            continue
        j, a = flat[rng.integers(len(flat))]
        w = rng.dirichlet([1.0, 1.0, 1.0])
        pt = (w @ T[j].astype(np.float64)).astype(F)
        pt[a] = T[j, 0, a]
        ax = (a + 1 + rng.integers(0, 2)) % 3
        d[i] = np.where(rng.random(3) < 0.5, F(-0.0), F(0.0))
        d[i, ax] = sign[i]
        pt[ax] -= F(sign[i] * rng.uniform(0.1, 3.0) * scale[ax])
        o[i] = pt
    return _pack(o, d, 0.0, 100.0 * scale.max())


def _ranges(rng, T, scale, centre, n):
    """tmin > 0 ahead of and just past the first hit; tmax just short of and just past it.  'Just' is
    four times the pair's own t bound (at least 2^-17 relative), so float64 can decide every ray."""
    rays = _interior(rng, T, scale, centre, n)
    E = trace_ref.exact_hits(T, rays)
    with np.errstate(all="ignore"):
        cand = np.where((E["m"] > trace_ref.bound(E["cond_m"])) & (E["t"] > 0), E["t"], np.inf)
    j = cand.argmin(axis=1)
    t1 = cand[np.arange(n), j]
    rel = np.maximum(2.0 ** -17, 4.0 * trace_ref.bound(E["cond_t"][np.arange(n), j]))
    rel = np.where(np.isfinite(rel), rel, 2.0 ** -17)
    has = np.isfinite(t1)
    t1 = np.where(has, t1, scale.max())
    q = np.arange(n) % 4
    rays[:, 6] = np.where(q == 0, rng.uniform(0.2, 0.8, n) * t1, np.where(q == 1, t1 * (1.0 + rel), 0.0))
    rays[:, 7] = np.where(q == 2, t1 * (1.0 - rel), np.where(q == 3, t1 * (1.0 + rel), rays[:, 7]))
    return rays


_MAKERS = dict(interior=_interior, edges=_edges, leaving=_leaving, inplane=_inplane, ranges=_ranges, axis=_axis)


@lru_cache(maxsize=None)
def ray_set(name, kind, n=N_RAYS):
    """(n, 8) float32 rays of one kind for one variant."""
    sc, scale, centre = make(name)
    T = world_triangles(sc).astype(np.float64)
    rng = np.random.default_rng(7919 * VARIANTS.index(name) + RAY_SETS.index(kind))
    rays = _MAKERS[kind](rng, T, scale, centre, n)
    rays.setflags(write=False)
    return rays
