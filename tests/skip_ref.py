"""A numpy fp64 restatement of the skip table (optixpathtracer_amd/csrc/pt_skip.h), written from the
header's prose for the tests to compare the device's words with; it shares no code with the header.

The arrays are those of OptixRenderer.bvh_arrays():
  * nodes (n_nodes, 32) uint32: per BVH4 node lox hix loy hiy loz hiz child pad, 4 words each.  A child
    link >= 0 is an inner node's index, 0x80000000 an empty slot (tested first), anything else a leaf's
    code c with first = (~c) >> 3 and count = ((~c) & 7) + 1 leaf-order triangles;
  * tris (n, 12) uint32: per leaf-order triangle v0 | e1 | e2 as fp32 bits, word 3 the global triangle
    index as int bits.  The triangle is v0, v0 + e1, v0 + e2 in fp64, as the hit test sees it.

A word of (T, side) is the child link of the highest link on T's leaf-to-root path whose whole subtree
is "below" T on that side, or 0.  Side 0 is the side of e1 x e2.  U is below T when its three heights
over T's plane on that side are <= kLitDelta and U is no sliver (aspect = smallest height / longest
edge >= 2^-6); a T without a plane or with an aspect under 2^-10 has no words at all.

The second half builds the extension rays that test the header's premise: rays that leave T as
reconstruct + continue_path write them (fp32), with a direction just inside skip_pick's use condition.
"""
import numpy as np

LIT_DELTA = float(np.float32(5e-4))  # kLitDelta: the fp32 constant, widened
MIN_ASPECT = 2.0 ** -6               # kSkipMinAspect: below it U is a sliver
MIN_ASPECT_T = 2.0 ** -10            # kSkipMinAspectT
MIN_COS = np.float32(2.0 ** -6)      # kSkipMinCos
MAX_TRIS = 4096                      # kSkipMaxTris
EMPTY = -0x80000000
OFFSET = np.float32(1e-3)            # continue_path's origin offset along Ng
EDGE = (1e-6, 1e-4, 1e-2, 0.3, 3.0)  # the ray's cosine to the offset direction is 2^-6 * (1 + e)
# (u, v) of the origins: the three vertices, three edge points, three interior points
UV = np.float32([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5], [1 / 3, 1 / 3], [0.125, 0.75], [0.7, 0.05]])


# -- the predicate ----------------------------------------------------------------------------------
def vertices(tris):
    """(n, 3, 3) fp64: a, b, c of every record."""
    f = np.ascontiguousarray(tris, np.uint32).view(np.float32).astype(np.float64)
    a = f[:, 0:3]
    return np.stack([a, a + f[:, 4:7], a + f[:, 8:11]], axis=1)


def global_index(tris):
    return np.ascontiguousarray(tris, np.uint32)[:, 3].view(np.int32)


def aspect(v):
    """Smallest height / longest edge = |e1 x e2| / (longest edge)^2; NaN or 0 where that means nothing."""
    e1, e2, e3 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], v[:, 2] - v[:, 1]
    l2 = np.max(np.stack([(e * e).sum(axis=1) for e in (e1, e2, e3)]), axis=0)
    with np.errstate(all="ignore"):
        return np.linalg.norm(np.cross(e1, e2), axis=1) / l2


def unit_normals(v):
    """(normals (n, 3), has_plane (n,)): a triangle whose corner sine is under 1e-6 has no plane."""
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.cross(e1, e2)
    l2 = (n * n).sum(axis=1)
    with np.errstate(all="ignore"):
        ok = (l2 > 1e-12 * (e1 * e1).sum(axis=1) * (e2 * e2).sum(axis=1)) & (l2 > 0.0)
        return n / np.sqrt(l2)[:, None], ok


def below(tris, rows=None, chunk=256):
    """(n, 2, n) bool: below[T, side, U]; with `rows`, the rows of those T only, (len(rows), 2, n)."""
    v = vertices(tris)
    n = len(v)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    with np.errstate(all="ignore"):
        asp = aspect(v)
        nrm, plane = unit_normals(v)
        counts = asp >= MIN_ASPECT          # NaN compares false
        origin = plane & (asp >= MIN_ASPECT_T)
        out = np.zeros((len(rows), 2, n), bool)
        for lo in range(0, len(rows), chunk):
            t = rows[lo:lo + chunk]
            # heights of every vertex of every U over the planes of these T
            h = np.einsum("tk,uvk->tuv", nrm[t], v) - np.einsum("tk,tk->t", nrm[t], v[t, 0])[:, None, None]
            for side, s in ((0, 1.0), (1, -1.0)):
                out[lo:lo + chunk, side] = ((s * h) <= LIT_DELTA).all(axis=2) & counts[None, :] & origin[t, None]
    return out


# -- the tree ---------------------------------------------------------------------------------------
def _children(nodes, i):
    ch = np.ascontiguousarray(nodes, np.uint32)[i, 24:28].view(np.int32)
    return [int(c) for c in ch if int(c) != EMPTY]


def leaf_triangles(c):
    first, count = (~c) >> 3, ((~c) & 7) + 1
    return list(range(first, first + count))


def paths(nodes, n):
    """(path, under): path[t] = the child links from t's leaf up to the root's child; under[link] = the
    sorted leaf-order triangles below that link.  Enumerates the tree from the root."""
    under, parent = {}, {}
    path = [None] * n

    def visit(link, up):
        assert link not in under, f"link {link} appears twice"
        parent[link] = up
        if link < 0:
            mine = leaf_triangles(link)
            for t in mine:
                assert 0 <= t < n and path[t] is None, f"triangle {t} out of range or in two leaves"
                p, at = [], link
                while at is not None:
                    p.append(at)
                    at = parent[at]
                path[t] = p
        else:
            assert 0 < link < len(nodes), f"inner link {link}"
            mine = []
            for c in _children(nodes, link):
                mine += visit(c, link)
        under[link] = np.array(sorted(mine), np.int64)
        return mine

    for c in _children(nodes, 0):
        visit(c, None)
    assert all(p is not None for p in path), "a triangle in no leaf"
    return path, under


def _highest(path, under, bel, rows, allowed):
    words = np.zeros((len(rows), 2), np.uint32)
    for k, t in enumerate(rows):
        for side in (0, 1):
            for link in path[t]:  # leaf first; the sets are nested, so the first failure ends the climb
                if not bel[k, side, under[link]].all():
                    break
                if allowed(link):
                    words[k, side] = np.uint32(link & 0xFFFFFFFF)
    return words


def _rows(tris, bel, rows):
    rows = np.arange(len(tris)) if rows is None else np.asarray(rows, np.int64)
    return rows, (below(tris, rows) if bel is None else bel)


def expected_words(nodes, tris, bel=None, rows=None, tree=None):
    """(n, 2) uint32: the word of every (T, side) when no budget runs out.  rows: those T only, with bel
    = below(tris, rows) where it is given; tree = paths(nodes, n) where the caller has it."""
    rows, bel = _rows(tris, bel, rows)
    path, under = tree or paths(nodes, len(tris))
    return _highest(path, under, bel, rows, lambda link: True)


def floor_words(nodes, tris, bel=None, rows=None, tree=None):
    """The highest passing link with at most kSkipMaxTris - 1 triangles under it: one walk looks at every
    triangle under a link at most once, so the budget cannot run out at or below it."""
    rows, bel = _rows(tris, bel, rows)
    path, under = tree or paths(nodes, len(tris))
    return _highest(path, under, bel, rows, lambda link: len(under[link]) <= MAX_TRIS - 1)


def height_on_path(path, words, rows=None):
    """(n, 2) int: the position of each word on its triangle's path (0 = the leaf), -1 for "none";
    raises where a non-zero word is not on the path."""
    rows = range(len(words)) if rows is None else rows
    out = np.full(words.shape, -1, np.int64)
    for k, t in enumerate(rows):
        for side in (0, 1):
            w = int(np.uint32(words[k, side]).view(np.int32))
            if w != 0:
                assert w in path[t], f"the word {w:#x} of triangle {t} side {side} is not on its path"
                out[k, side] = path[t].index(w)
    return out


def names_hit(words, under, T, side, prim):
    """Per ray: the word of (T, side) -- T and prim are leaf-order indices -- names a subtree that holds
    the triangle the ray hit (prim < 0: no hit)."""
    out = np.zeros(len(T), bool)
    for k in np.flatnonzero(prim >= 0):
        w = int(np.uint32(words[T[k], side[k]]).view(np.int32))
        if w != 0:
            s = under[w]
            i = np.searchsorted(s, prim[k])
            out[k] = i < len(s) and s[i] == prim[k]
    return out


# -- records of a scene without a renderer (identity model matrices) ---------------------------------
def scene_records(scene):
    """(n, 12) uint32 records in global triangle order, and the fp32 vertices (n, 3, 3): e1 and e2 are
    the one fp32 subtraction the scene upload stores."""
    vs = []
    for m in scene.meshes:
        assert np.array_equal(np.asarray(m.model, np.float32).reshape(4, 4), np.eye(4, dtype=np.float32))
        vs.append(np.asarray(m.vertices, np.float32)[np.asarray(m.indices)])
    v = np.concatenate(vs)
    rec = np.zeros((len(v), 12), np.float32)
    rec[:, 0:3], rec[:, 4:7], rec[:, 8:11] = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    rec = rec.view(np.uint32)
    rec[:, 3] = np.arange(len(v), dtype=np.int32).view(np.uint32)
    return rec, v


# -- the premise's rays ------------------------------------------------------------------------------
def _dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize32(a):
    return a * (np.float32(1.0) / np.sqrt(_dot32(a, a)))[:, None]


def premise_rays(v32, pairs, seed=1):
    """Extension rays as the shading kernels write them, all in fp32.  v32 (n, 3, 3): the fp32 vertices
    in the order `pairs` indexes; pairs (m, 2): (T, side).  Per pair one ray per entry of UV:
    p = w v0 + u v1 + v v2, Ng = normalize(cross(v1 - v0, v2 - v0)), o = p +- 1e-3 Ng, d normalised with
    an exact cosine of 2^-6 (1 + e) to the offset direction (e cycles through EDGE) and a random
    tangent.  Returns (rays (k, 8), T (k,), side (k,), generated): only the rays whose fp32
    dot(d, off) > 2^-6 -- skip_pick's use condition -- are kept; `generated` counts all."""
    assert v32.dtype == np.float32
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    T = np.repeat(pairs[:, 0], len(UV))
    side = np.repeat(pairs[:, 1], len(UV))
    uv = np.tile(UV, (len(pairs), 1))
    e = np.float64(EDGE)[(np.arange(len(T)) + T) % len(EDGE)]
    v0, v1, v2 = v32[T, 0], v32[T, 1], v32[T, 2]
    u, v = uv[:, 0:1], uv[:, 1:2]
    w = np.float32(1.0) - u - v
    p = (w * v0 + u * v1) + v * v2
    ng = _normalize32(np.cross(v1 - v0, v2 - v0).astype(np.float32))
    off = np.where(side[:, None] == 1, -ng, ng)
    o = p + OFFSET * off
    # the direction in fp64 about the fp32 offset direction, then rounded and normalised as the kernels do
    a = off.astype(np.float64)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    r = rng.standard_normal(a.shape)
    tan = r - (r * a).sum(axis=1, keepdims=True) * a
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    c = (2.0 ** -6 * (1.0 + e))[:, None]
    d = _normalize32((c * a + np.sqrt(1.0 - c * c) * tan).astype(np.float32))
    keep = _dot32(d, off) > MIN_COS
    rays = np.concatenate([o, d, np.zeros((len(o), 1), np.float32), np.full((len(o), 1), 100, np.float32)], axis=1)
    return rays[keep].astype(np.float32), T[keep], side[keep], len(keep)


# -- a tree without a renderer -----------------------------------------------------------------------
def build_tree(tris, leaf=2):
    """A median-split BVH4 in the tracer's layout over records in any order, for the tests that run
    without a GPU: (nodes, order); tris[order] are the records in this tree's leaf order."""
    f = np.ascontiguousarray(tris, np.uint32).view(np.float32)
    v = np.stack([f[:, 0:3], f[:, 0:3] + f[:, 4:7], f[:, 0:3] + f[:, 8:11]], axis=1)
    cen = v.mean(axis=1)
    nodes, order = [], []

    def halves(idx):
        c = cen[idx]
        s = idx[np.argsort(c[:, int(np.argmax(c.max(axis=0) - c.min(axis=0)))], kind="stable")]
        return s[:len(s) // 2], s[len(s) // 2:]

    def link_of(idx):
        if len(idx) <= leaf:
            first = len(order)
            order.extend(int(i) for i in idx)
            return ~((first << 3) | (len(idx) - 1))
        me = len(nodes)
        nodes.append(None)
        fill(me, idx)
        return me

    def fill(me, idx):
        parts = []
        for h in halves(idx):
            parts += halves(h) if len(h) > leaf else [h]
        parts = [p for p in parts if len(p)]
        row = np.zeros(32, np.uint32)
        box = row[:24].view(np.float32).reshape(3, 2, 4)  # axis, lo / hi, slot
        box[:, 0], box[:, 1] = np.inf, -np.inf  # empty slots: inverted boxes
        row[24:28] = np.uint32(EMPTY & 0xFFFFFFFF)
        nodes[me] = row
        for q, p in enumerate(parts):
            box[:, 0, q], box[:, 1, q] = v[p].reshape(-1, 3).min(axis=0), v[p].reshape(-1, 3).max(axis=0)
            row[24 + q] = np.uint32(link_of(p) & 0xFFFFFFFF)

    nodes.append(None)
    fill(0, np.arange(len(f)))
    return np.stack(nodes), np.array(order, np.int64)


# -- a scene where the side matters --------------------------------------------------------------------
def open_shells():
    """The coarse sphere box with its spheres replaced by two open 8x4 hemispheres of radius 0.45.  The
    first is the half away from the camera, wound outward: the camera looks into the bowl and sees back
    faces.  The second is the half toward the camera, wound inward: the camera sees its outside, again
    back faces, and its bowl opens to the back wall.  A ray that leaves the inside of a bowl has nothing
    of the bowl below it, while the other side's word can name the whole bowl: with the sides swapped,
    such a ray would drop the triangles it hits."""
    import dataclasses

    from optixpathtracer_amd import scenes

    sc = scenes.sphere_in_box("diffuse", sphere_segments=8, sphere_rings=4, grid=2)
    shells = []
    for name, centre, far, inward in (("bowl_outward", (0.3, -0.7, 0.9), True, False),
                                      ("dome_inward", (0.3, 0.7, 0.9), False, True)):
        v, n, idx = scenes.uv_sphere(centre, 0.45, 8, 4)
        x = v[idx].mean(axis=1)[:, 0] - centre[0]
        idx = idx[x < 0] if far else idx[x > 0]
        assert len(idx) == 24  # the cut runs along two meridians
        if inward:
            idx = idx[:, [0, 2, 1]]
        shells.append(scenes.Mesh(vertices=np.ascontiguousarray(scenes.blender_to_engine(v), dtype=np.float32),
                                  normals=np.ascontiguousarray(scenes.blender_to_engine(n), dtype=np.float32),
                                  indices=np.ascontiguousarray(idx, dtype=np.int32), albedo=(0.6, 0.02, 0.02),
                                  roughness=0.2, name=name))
    walls = [m for m in sc.meshes if not m.name.startswith("sphere")]
    return dataclasses.replace(sc, meshes=shells + walls, name="open_shells")


def leaf_order_of(tris, rec):
    """leaf_of[global index] = leaf-order index, from word 3 of the leaf-order records `tris`; checks that
    they hold the geometry of `rec` (scene_records) bit for bit (words 7 and 11 are not geometry)."""
    tris = np.ascontiguousarray(tris, np.uint32)
    leaf_of = np.empty(len(tris), np.int64)
    leaf_of[global_index(tris)] = np.arange(len(tris))
    geometry = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]
    assert np.array_equal(tris[leaf_of][:, geometry], rec[:, geometry]), "the records are not the scene's triangles"
    return leaf_of


def shell_counts(pairs):
    """The (T, side) pairs of side_swap_hits on open_shells() per (shell, side): its first 24 triangles
    are the outward bowl, the next 24 the inward dome."""
    return {(name, side): int(((pairs[:, 0] // 24 == k) & (pairs[:, 1] == side)).sum())
            for k, name in enumerate(("bowl_outward", "dome_inward")) for side in (0, 1)}


def side_swap_hits(scene, nodes, tris, trace):
    """How a swap of the two sides would show on `scene`: traces premise_rays from every (T, side) that has
    words with `trace` (rays -> global prim) and returns the (T, side) pairs, T global, for which some
    ray hits a triangle under the link that the OTHER side's word names.  nodes, tris: the tree and its
    leaf-order records; the words are expected_words."""
    rec, v32 = scene_records(scene)
    leaf_of = leaf_order_of(tris, rec)
    bel = below(tris)
    tree = paths(nodes, len(tris))
    words = expected_words(nodes, tris, bel, tree=tree)
    n = len(tris)
    own = bel[np.arange(n), :, np.arange(n)]
    pairs = np.argwhere(own)  # leaf order
    pairs[:, 0] = global_index(tris)[pairs[:, 0]]
    rays, T, side, _ = premise_rays(v32, pairs)
    prim = np.asarray(trace(rays))
    hit_leaf = np.where(prim >= 0, leaf_of[np.maximum(prim, 0)], -1)
    assert not names_hit(words, tree[1], leaf_of[T], side, hit_leaf).any(), "a ray's own word names its hit"
    swapped = names_hit(words, tree[1], leaf_of[T], 1 - side, hit_leaf)
    return np.unique(np.stack([T[swapped], side[swapped]], axis=1), axis=0)
