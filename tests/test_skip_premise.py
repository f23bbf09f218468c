"""The premise of the skip table (pt_skip.h, "what is assumed"), tested with the CPU oracle, which traces
bit for bit like the kernels: an extension ray that leaves triangle T on one side, with fp32
dot(d, off) just above 2^-6, is never hit by a triangle U that counts as below T on that side
(tests/skip_ref.py).  That set holds every subtree a word of (T, side) can name, whatever the tree.
The rays start on T's vertices, edges and interior and have exact cosines 2^-6 (1 + e) to the offset
direction, e from 1e-6 to 3; the scenes put coordinates near the 128 bound and aspects on both sides of
the sliver threshold.  The first test pins skip_ref's tree walk on a hand-made tree.
"""
import numpy as np
import pytest

import skip_ref


def _leaf(first, count):
    return ~((first << 3) | (count - 1))


def _tree_and_records(sliver):
    """root -> [node 1, leaf(4)], node 1 -> [leaf(0, 1), leaf(2, 3)]: two coplanar quads at z = 0 and
    one triangle at z = 1; `sliver` squeezes triangle 3 to an aspect of 2^-8."""
    quad = lambda x: [[[x, 0, 0], [x + 1, 0, 0], [x + 1, 1, 0]], [[x, 0, 0], [x + 1, 1, 0], [x, 1, 0]]]
    v = np.float32(quad(0) + quad(2) + [[[0, 0, 1], [1, 0, 1], [0, 1, 1]]])
    if sliver:
        v[3] = [[2, 0, 0], [3, 0, 0], [2.5, 2.0 ** -8, 0]]
    rec = np.zeros((5, 12), np.float32)
    rec[:, 0:3], rec[:, 4:7], rec[:, 8:11] = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    rec = rec.view(np.uint32)
    rec[:, 3] = np.arange(5)
    nodes = np.zeros((2, 32), np.int32)
    nodes[:, 24:28] = skip_ref.EMPTY
    nodes[0, 24:26] = [1, _leaf(4, 1)]
    nodes[1, 25:27] = [_leaf(0, 2), _leaf(2, 2)]  # slot 0 stays empty
    return nodes.view(np.uint32), rec


def test_reference_on_a_hand_made_tree():
    nodes, rec = _tree_and_records(False)
    path, under = skip_ref.paths(nodes, 5)
    assert path[0] == [_leaf(0, 2), 1] and path[3] == [_leaf(2, 2), 1] and path[4] == [_leaf(4, 1)]
    assert list(under[1]) == [0, 1, 2, 3] and list(under[_leaf(2, 2)]) == [2, 3]
    bel = skip_ref.below(rec)
    assert bel[:4, :, :4].all() and bel[4, :, 4].all()
    assert bel[4, 0, :4].all() and not bel[4, 1, :4].any()  # seen from z = 1, z = 0 is below the upper side only
    assert bel[:4, 0, 4].sum() == 0 and bel[:4, 1, 4].all()
    top = np.uint32(_leaf(4, 1) & 0xFFFFFFFF)
    want = np.array([[1, 1]] * 4 + [[top, top]], np.uint32)
    assert np.array_equal(skip_ref.expected_words(nodes, rec), want)
    assert np.array_equal(skip_ref.floor_words(nodes, rec), want)
    # a sliver does not count: it blocks its own leaf and every link over it, and has no passing leaf itself
    nodes, rec = _tree_and_records(True)
    bel = skip_ref.below(rec)
    assert not bel[:, :, 3].any() and bel[3, :, :3].all()
    near = np.uint32(_leaf(0, 2) & 0xFFFFFFFF)
    want = np.array([[near, near]] * 2 + [[0, 0]] * 2 + [[top, top]], np.uint32)
    assert np.array_equal(skip_ref.expected_words(nodes, rec), want)
    assert np.array_equal(skip_ref.height_on_path(path, want), [[0, 0]] * 2 + [[-1, -1]] * 2 + [[0, 0]])
    # no plane, or an aspect under 2^-10: the whole row is false
    rec = rec.copy()
    rec.view(np.float32)[0, 8:11] = [0.5, 2.0 ** -12, 0]
    rec.view(np.float32)[1, 0] = np.nan
    bel = skip_ref.below(rec)
    assert not bel[:2].any() and not bel[:, :, :2].any() and bel[2, :, 2].all()


def test_open_shells_tell_the_sides_apart(oracle_lib):
    """The reference alone, on a median-split tree: on each hemisphere there are (T, side) pairs whose
    rays hit a triangle under the link the other side's word names -- a swap of the sides would drop
    that hit -- for a front-face approach (side 0, the inward shell's inside) and a back-face approach
    (side 1, the outward shell's inside) alike.  No ray's own word names its hit (side_swap_hits)."""
    sc = skip_ref.open_shells()
    assert [m.name for m in sc.meshes[:2]] == ["bowl_outward", "dome_inward"]
    rec, _ = skip_ref.scene_records(sc)
    nodes, order = skip_ref.build_tree(rec)
    o = oracle_lib.OracleScene(sc)
    pairs = skip_ref.side_swap_hits(sc, nodes, rec[order], lambda rays: o.trace(rays)[0])
    o.close()
    counts = skip_ref.shell_counts(pairs)
    print(f"open shells: (T, side) pairs that a side swap would change: {counts}")
    assert counts[("bowl_outward", 1)] > 0 and counts[("dome_inward", 0)] > 0


def _scaled_sphere(scale, name):
    """One 24x12 UV sphere of radius 1, scaled about its centre and moved to (64, 64, 64)."""
    from optixpathtracer_amd import scenes

    v, n, idx = scenes.uv_sphere((0.0, 0.0, 0.0), 1.0, 24, 12)
    v, n = scenes.blender_to_engine(v).astype(np.float64), scenes.blender_to_engine(n)  # the poles on the y axis
    mesh = scenes.Mesh(vertices=np.ascontiguousarray(v * np.float64(scale) + 64.0, dtype=np.float32),
                       normals=np.ascontiguousarray(n, dtype=np.float32), indices=idx.astype(np.int32), name=name)
    return scenes.Scene(meshes=[mesh], lights=np.zeros((0, 6), np.float32), camera_blender_pos=(0, 0, 0),
                        camera_blender_rot=(0, 0, 0), name=name)


def _coarse():
    from optixpathtracer_amd import scenes

    return scenes.sphere_in_box("diffuse", sphere_segments=8, sphere_rings=4, grid=2)


SCENES = {
    "coarse_box": (_coarse, None),
    "sphere_r55": (lambda: _scaled_sphere((55, 55, 55), "sphere_r55"), None),
    "sphere_flat": (lambda: _scaled_sphere((55, 55, 4), "sphere_flat"), (0.015, 0.025)),  # smallest aspect
    "sphere_long": (lambda: _scaled_sphere((2, 2, 60), "sphere_long"), (0.0, 2.0 ** -6)),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_no_ray_hits_a_triangle_that_counts_as_below(oracle_lib, name):
    make, aspects = SCENES[name]
    sc = make()
    rec, v32 = skip_ref.scene_records(sc)
    n = len(rec)
    if aspects is not None:  # the scene is the edge it claims to be
        smallest = float(skip_ref.aspect(skip_ref.vertices(rec)).min())
        assert aspects[0] < smallest < aspects[1], smallest
    assert float(np.abs(v32).max()) <= 128.0
    bel = skip_ref.below(rec)
    own = bel[np.arange(n), :, np.arange(n)]  # (n, 2): below[T, side, T]
    pairs = np.argwhere(own)
    assert len(pairs) > n // 2
    rays, T, side, generated = skip_ref.premise_rays(v32, pairs)
    assert generated >= 9 * len(pairs)
    print(f"{name}: {n} triangles, {len(pairs)} (T, side) pairs, {len(rays)} of {generated} rays pass the use condition")
    assert 4 * len(rays) >= 3 * generated
    o = oracle_lib.OracleScene(sc)
    prim = o.trace(rays)[0]
    o.close()
    hit = prim >= 0
    bad = hit & bel[T, side, np.where(hit, prim, 0)]
    print(f"{name}: {int(hit.sum())} rays hit something, {int(bad.sum())} hit a triangle below their origin")
    assert hit.any() and (prim < n).all()
    assert not bad.any(), f"{name}: rays {np.flatnonzero(bad)[:8]} hit triangles {prim[bad][:8]} of T {T[bad][:8]}"
