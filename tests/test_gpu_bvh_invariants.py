"""Structural invariants of the BVH4 every builder leaves (pt_build.hip bvh_build: one of four front
ends, then the common collapse), on the smallest triangle counts at which each stage can go wrong:
1 (the root is a leaf; the SAH builders take the Morton path), 2 (one binary node), 3 and 5 (either
side of a full 4-wide node), 18 (one more than the PLOC window, 2 * PT_PLOC_RADIUS + 1), 65
(PT_SAH_SMALL + 1: one large level before the per-wave subtrees) and 130 (two large levels).
Replaces optixAccelBuild (OptixRenderer.cpp:306-456), whose output cannot be inspected."""
import numpy as np
import pytest

from bvh_ref import EMPTY, expected_child_boxes, stored_child_boxes

pytestmark = pytest.mark.gpu

BUILDERS = {"lbvh": 1, "sah_host": 2, "ploc": 3, "sah_gpu": 4}  # capi.PT_BVH_*
SIZES = [1, 2, 3, 5, 18, 65, 130]


def _soup(n, seed):
    from optixpathtracer_amd import scenes

    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, (n, 1, 3)) + 0.2 * rng.uniform(-1.0, 1.0, (n, 3, 3))
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    idx = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    mesh = scenes.Mesh(vertices=v, indices=idx, normals=np.tile(np.float32([0, 0, 1]), (len(v), 1)))
    return scenes.Scene(meshes=[mesh], lights=np.zeros((0, 6), np.float32), camera_blender_pos=(0, 0, 0),
                        camera_blender_rot=(0, 0, 0))


def _build(sc, builder):
    from optixpathtracer_amd.renderer import OptixRenderer

    r = OptixRenderer(None, sc, bvh_builder=builder)
    try:
        nodes, recs = r.bvh_arrays()
        return nodes, recs, r.stats()
    finally:
        r.close()


def _levels(child):
    """Breadth-first levels from node 0 as lists of node indices; asserts what the numbering promises."""
    seen = np.zeros(len(child), np.int32)
    seen[0] = 1
    levels, level = [], [0]
    while level:
        # breadth-first numbering: a level's nodes are consecutive, and the next level follows it
        assert level == list(range(level[0], level[0] + len(level))), f"level {len(levels)} is not contiguous: {level}"
        if levels:
            assert level[0] == levels[-1][-1] + 1
        levels.append(level)
        nxt = []
        for p in level:
            for c in child[p]:
                if c != EMPTY and c >= 0:
                    assert p < c < len(child), f"node {p} links node {c}"
                    seen[c] += 1
                    nxt.append(int(c))
        level = nxt
    assert (seen == 1).all(), f"nodes not reached exactly once: {np.flatnonzero(seen != 1).tolist()}"
    return levels


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("builder", list(BUILDERS.values()), ids=list(BUILDERS))
def test_bvh_invariants(builder, n):
    sc = _soup(n, 7919 * n + builder)
    nodes, recs, st = _build(sc, builder)
    assert st["triangles"] == n and len(recs) == n
    assert len(nodes) == st["bvh_nodes"] >= 1
    # every original triangle exactly once
    np.testing.assert_array_equal(np.sort(recs[:, 3]), np.arange(n, dtype=np.uint32))
    child = nodes[:, 24:28].view(np.int32)
    # the leaf links' ranges partition [0, n)
    leaves = ~child[(child < 0) & (child != EMPTY)]
    first, count = leaves >> 3, (leaves & 7) + 1
    assert ((count >= 1) & (count <= 4)).all()
    order = np.argsort(first)
    np.testing.assert_array_equal(first[order], np.concatenate([[0], np.cumsum(count[order])[:-1]]))
    assert int(count.sum()) == n
    # every node once, children after their parent, levels contiguous, as many as bvh_depth
    assert len(_levels(child)) == st["bvh_depth"]
    # stored boxes: the exact unions of the padded triangle boxes below; empty slots inverted
    for k, (elo, ehi) in enumerate(expected_child_boxes(nodes, recs)):
        lo, hi = stored_child_boxes(nodes, k)
        assert lo.tobytes() == elo.tobytes() and hi.tobytes() == ehi.tobytes(), f"node {k}"
        empty = child[k] == EMPTY
        assert (lo[empty] == np.inf).all() and (hi[empty] == -np.inf).all()
    # the build is deterministic
    nodes2, recs2, st2 = _build(sc, builder)
    assert nodes2.tobytes() == nodes.tobytes() and recs2.tobytes() == recs.tobytes()
    assert (st2["bvh_nodes"], st2["bvh_depth"]) == (st["bvh_nodes"], st["bvh_depth"])
