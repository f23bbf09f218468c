"""The skip words that k_skip_parents and k_skip_build write on the device (pt_lit.hip), compared word for
word, in leaf order, with the numpy fp64 restatement of pt_skip.h in tests/skip_ref.py, on the tree and
the records downloaded from the same renderer.  Every comparison is exact.

  * scenes of at most 4000 triangles, where no walk can spend its budget: words == expected_words, for
    the four builders, after a refit (loose boxes: box tests and triangle truth diverge) and after a
    rebuild;
  * floor scenes (a planar floor under one sphere, with and without a sliver), where one side of a
    triangle has more than kSkipMaxTris triangles below it: every word is on its triangle's path, every
    triangle under it is below, and floor_words <= word <= expected_words in path height.  4608 floor
    triangles are compared in full; 18432, where more than kSkipMaxTris lie under one child of the root
    and the budget does run out, for every 31st triangle;
  * degenerate triangles have no words and lie under no word; a NaN vertex or a mesh moved beyond the
    128-unit bound switches the table off, and a move back inside rebuilds it;
  * the premise on the device: the rays of tests/test_skip_premise.py through trace_rays never hit a
    triangle under the link that the device's own word of their (T, side) names.
"""
import numpy as np
import pytest

import skip_ref

pytestmark = pytest.mark.gpu

LAMBERT = 1
BUILDERS = {"lbvh": 1, "sah": 2, "ploc": 3, "sah_gpu": 4}


def _coarse():
    from optixpathtracer_amd import scenes

    return scenes.sphere_in_box("diffuse", sphere_segments=8, sphere_rings=4, grid=2)


def _textured():
    from optixpathtracer_amd import scenes

    return scenes.textured_scene("diffuse")


def _renderer(sc, builder=0):
    from optixpathtracer_amd.renderer import OptixRenderer

    r = OptixRenderer(None, sc, material_mode=LAMBERT, kernel=1, bvh_builder=builder)
    r.set_skip_table(True)
    return r


def _download(r):
    nodes, tris = r.bvh_arrays()
    words = r.skip_table()
    assert words is not None and words.shape == (len(tris), 2)
    assert r.stats()["skip_table_bytes"] == 8 * len(tris)
    return nodes, tris, words


def _assert_exact(r, what):
    nodes, tris, words = _download(r)
    tree = skip_ref.paths(nodes, len(tris))
    want = skip_ref.expected_words(nodes, tris, tree=tree)
    diff = (words != want).any(axis=1)
    high = skip_ref.height_on_path(tree[0], want)
    print(f"{what}: {len(tris)} triangles, {len(nodes)} nodes, {int((want != 0).sum())} links of {want.size} words, "
          f"{int((high > 0).sum())} above the leaf, {int(diff.sum())} triangles differ")
    assert not diff.any(), (f"{what}: triangles {np.flatnonzero(diff)[:8]}: device {words[diff][:8].tolist()}, "
                            f"reference {want[diff][:8].tolist()}")
    assert (high > 0).any()  # not vacuous: some words name inner nodes
    return nodes, tris, words, tree


def _translation(x, y, z):
    a = np.eye(4)
    a[:3, 3] = [x, y, z]
    return np.ascontiguousarray(a.T.ravel(), dtype=np.float32)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("scene", ["coarse", "textured"])
def test_words_equal_the_reference(scene, builder):
    r = _renderer({"coarse": _coarse, "textured": _textured}[scene](), BUILDERS[builder])
    try:
        _assert_exact(r, f"{scene}, {builder}")
    finally:
        r.close()


@pytest.mark.parametrize("how", ["refit", "rebuild"])
def test_words_after_a_move(how):
    """A sphere moved on a live renderer: after a refit the old tree has loose boxes around the moved
    triangles, after a rebuild the tree is new; the words follow the triangles either way."""
    r = _renderer(_coarse())
    try:
        _, tris0, words0, _ = _assert_exact(r, "before the move")
        r.set_mesh_transform(1, _translation(0.35, 0.1, -0.2))
        r.commit_geometry(how)
        _, tris1, words1, _ = _assert_exact(r, f"after the {how}")
        assert (tris1 != tris0).any(), "the move changed no record"
    finally:
        r.close()


def floor_scene(quads, sliver):
    """A planar floor of quads x quads squares over [-2.4, 2.4]^2 at z = 0 (normals +z), one 8x4 sphere
    of radius 0.2 above its middle and, with `sliver`, one triangle of aspect 2^-8 away from both (the
    scenes of tests/skip_host_check.cpp)."""
    from optixpathtracer_amd import scenes

    g = np.linspace(-2.4, 2.4, quads + 1)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    v = np.column_stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)])
    i, j = (a.ravel() for a in np.meshgrid(np.arange(quads), np.arange(quads), indexing="ij"))
    a = i * (quads + 1) + j
    b, c, d = a + quads + 1, a + quads + 2, a + 1  # (x + s, y), (x + s, y + s), (x, y + s)
    idx = np.concatenate([np.column_stack([a, b, c]), np.column_stack([a, c, d])])
    up = np.tile([0.0, 0.0, 1.0], (len(v), 1))
    mesh = lambda v, n, idx, name: scenes.Mesh(vertices=np.ascontiguousarray(v, dtype=np.float32),
                                               normals=np.ascontiguousarray(n, dtype=np.float32),
                                               indices=np.ascontiguousarray(idx, dtype=np.int32), name=name)
    meshes = [mesh(v, up, idx, "floor")]
    sv, sn, sidx = scenes.uv_sphere((0.0, 0.0, 0.5), 0.2, 8, 4)
    meshes.append(mesh(sv, sn, sidx, "sphere"))
    if sliver:
        meshes.append(mesh([[3.5, 0, 1], [4.5, 0, 1], [4.0, 2.0 ** -8, 1]], up[:3], [[0, 1, 2]], "sliver"))
    return scenes.Scene(meshes=meshes, lights=np.zeros((0, 6), np.float32), camera_blender_pos=(0, 0, 0),
                        camera_blender_rot=(0, 0, 0), material_mode=LAMBERT, name="floor")


def check_budgeted_words(nodes, tris, words, rows, what):
    """The floor scenes' checks for the triangles `rows` (leaf order); returns what the callers assert on:
    the heights of the device's words, of expected_words and of floor_words on each path, and the rows
    of the floor's downward sides as (k, side) index arrays."""
    tree = path, under = skip_ref.paths(nodes, len(tris))
    bel = skip_ref.below(tris, rows)
    got = skip_ref.height_on_path(path, words[rows], rows)  # raises unless every non-zero word is on its path
    for k, t in enumerate(rows):
        for side in (0, 1):
            if got[k, side] >= 0:
                s = under[path[t][got[k, side]]]
                assert bel[k, side, s].all(), f"{what}: a triangle under the word of ({t}, {side}) is not below"
    top = skip_ref.height_on_path(path, skip_ref.expected_words(nodes, tris, bel, rows, tree), rows)
    low = skip_ref.height_on_path(path, skip_ref.floor_words(nodes, tris, bel, rows, tree), rows)
    assert (low <= got).all() and (got <= top).all(), \
        f"{what}: {int((got < low).sum())} words lower than the budget allows, {int((got > top).sum())} too high"
    v = skip_ref.vertices(tris)[rows]
    on_floor = (v[:, :, 2] == 0).all(axis=1)
    nz = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])[:, 2]
    down = (np.flatnonzero(on_floor), np.where(nz[on_floor] > 0, 1, 0))
    root_child = np.array([len(path[t]) - 1 for t in rows])
    biggest = max(len(under[p[-1]]) for p in path)
    print(f"{what}: {len(tris)} triangles, {len(rows)} compared, at most {biggest} under a child of the root; "
          f"{int((got < top).sum())} words kept lower than expected_words by the budget, {int((got < 0).sum())} none")
    return got, top, low, down, root_child


@pytest.mark.parametrize("sliver", [False, True], ids=["plain", "sliver"])
def test_floor_words(sliver):
    sc = floor_scene(48, sliver)
    assert sc.n_triangles == 4608 + 48 + int(sliver)
    r = _renderer(sc)
    try:
        nodes, tris, words = _download(r)
    finally:
        r.close()
    rows = np.arange(len(tris))
    got, top, low, down, root_child = check_budgeted_words(nodes, tris, words, rows, f"floor, sliver={sliver}")
    assert len(down[0]) == 4608
    if not sliver:  # box_accept spends no budget: the whole scene is below the floor's downward sides
        assert (got[down] == root_child[down[0]]).all()


@pytest.mark.parametrize("sliver", [False, True], ids=["plain", "sliver"])
def test_wide_floor_words_when_the_budget_runs_out(sliver):
    """18432 floor triangles: some child of the root has more than kSkipMaxTris triangles under it, so
    with a sliver in the scene (every triangle looked at) a walk stops short of it; without, box_accept
    still reaches it.  Every 31st triangle is compared."""
    sc = floor_scene(96, sliver)
    r = _renderer(sc)
    try:
        nodes, tris, words = _download(r)
    finally:
        r.close()
    rows = np.arange(0, len(tris), 31)
    got, top, low, down, root_child = check_budgeted_words(nodes, tris, words, rows, f"wide floor, sliver={sliver}")
    assert len(down[0]) > 500
    if sliver:
        assert (got < top).any(), "no walk ran out of budget: the fallback did not run"
    else:
        assert (got[down] == root_child[down[0]]).all() and (got == top).all()


def _soup(nan):
    """The mesh of test_degenerate_triangles_build_and_trace: 100 random triangles, of which 1 is a point,
    2 a segment, 3 and 4 nearly coincide and, with `nan`, 5 has a NaN vertex."""
    from optixpathtracer_amd import scenes

    rng = np.random.default_rng(7)
    v = rng.uniform(-1, 1, size=(300, 3)).astype(np.float32)
    idx = np.arange(300, dtype=np.int32).reshape(100, 3)
    v[3:6] = v[3]
    v[6:9] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    v[9:12] = v[12:15] + np.float32(1e-7)
    if nan:
        v[15] = np.nan
    mesh = scenes.Mesh(vertices=v, indices=idx, normals=np.tile(np.float32([0, 0, 1]), (300, 1)))
    return scenes.Scene(meshes=[mesh], lights=np.zeros((0, 6), np.float32), camera_blender_pos=(0, 0, 0),
                        camera_blender_rot=(0, 0, 0), material_mode=LAMBERT)


@pytest.mark.parametrize("builder", ["sah", "sah_gpu", "ploc"])
def test_degenerate_triangles_have_no_words(builder):
    r = _renderer(_soup(False), BUILDERS[builder])
    try:
        nodes, tris, words = _download(r)
    finally:
        r.close()
    path, under = skip_ref.paths(nodes, len(tris))
    want = skip_ref.expected_words(nodes, tris, tree=(path, under))
    assert np.array_equal(words, want), np.flatnonzero((words != want).any(axis=1))[:8]
    deg = np.flatnonzero(np.isin(skip_ref.global_index(tris), [1, 2]))
    assert len(deg) == 2, "the point and the segment are no longer among the records"
    assert (words[deg] == 0).all()
    named = [under[int(w)] for w in words[words != 0].view(np.int32)]
    print(f"{builder}: {len(named)} links of {words.size} words")
    assert len(named) > 0 and not any(np.isin(deg, s).any() for s in named)


def test_nan_vertex_switches_the_table_off():
    """A vertex that is not finite is outside the table's bound (skip_tri_in_bounds): the scene runs
    without words.  SAH: the builder the parity suite runs on this mesh."""
    r = _renderer(_soup(True), BUILDERS["sah"])
    try:
        assert r.skip_table() is None
        assert r.stats()["skip_table_bytes"] == 0
    finally:
        r.close()


def test_the_bound_switches_the_table_off_and_on():
    r = _renderer(_coarse())
    try:
        _assert_exact(r, "inside")
        r.set_mesh_transform(1, _translation(200.0, 0.0, 0.0))  # beyond kLitMaxCoord = 128
        r.commit_geometry("refit")
        assert r.skip_table() is None
        assert r.stats()["skip_table_bytes"] == 0
        r.set_mesh_transform(1, _translation(0.35, 0.1, -0.2))
        r.commit_geometry("refit")
        _assert_exact(r, "back inside")
    finally:
        r.close()


def test_premise_rays_on_the_device():
    """The coarse scene's rays of test_skip_premise.py through the tracer, against the device's own words:
    no hit lies under the link its (T, side) names."""
    sc = _coarse()
    r = _renderer(sc)
    try:
        nodes, tris, words = _download(r)
        rec, v32 = skip_ref.scene_records(sc)
        gi = skip_ref.global_index(tris)
        leaf_of = skip_ref.leaf_order_of(tris, rec)
        bel = skip_ref.below(tris)
        pairs = np.argwhere(bel[np.arange(len(tris)), :, np.arange(len(tris))])
        pairs[:, 0] = gi[pairs[:, 0]]
        pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]  # global order: the rays of the CPU test
        rays, T, side, generated = skip_ref.premise_rays(v32, pairs)
        prim = r.trace_rays(rays)[0]
    finally:
        r.close()
    assert 4 * len(rays) >= 3 * generated
    hit = prim >= 0
    assert (prim < len(tris)).all()
    hit_leaf = np.where(hit, leaf_of[np.maximum(prim, 0)], -1)
    carried = words[leaf_of[T], side] != 0
    bad = skip_ref.names_hit(words, skip_ref.paths(nodes, len(tris))[1], leaf_of[T], side, hit_leaf)
    print(f"{len(rays)} of {generated} rays, {int(hit.sum())} hit, {int((carried & hit).sum())} hit with a word, "
          f"{int(bad.sum())} hit under their own word")
    assert (carried & hit).sum() > 100
    assert not bad.any(), f"rays {np.flatnonzero(bad)[:8]}: T {T[bad][:8]} side {side[bad][:8]} hit {prim[bad][:8]}"
    # and a triangle that counts as below is never hit, as on the CPU
    assert not (hit & bel[leaf_of[T], side, np.maximum(hit_leaf, 0)]).any()
