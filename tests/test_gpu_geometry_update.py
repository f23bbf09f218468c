"""Geometry updates on a live renderer (pt_set_mesh_transform / pt_set_mesh_vertices /
pt_commit_geometry, pt_refit.hip).

Closest hits are the (t, original index) minimum over acceptable hits for any BVH, and a refit
stores for its topology exactly the boxes a build would, so everything here is held to the
project's standard: after a commit the image and the triangle records are bit-identical to a
renderer created from the moved scene ("fresh") and to the CPU oracle of the moved scene.
"""
import dataclasses

import numpy as np
import pytest

from bvh_ref import EMPTY, expected_child_boxes, stored_child_boxes
from helpers import oracle_render, random_rays

pytestmark = pytest.mark.gpu

W, H, DEPTH, FIRST, FRAMES = 48, 32, 5, 3, 4


def assert_identical(g, o, what):
    diff = g != o
    if diff.any():
        idx = np.argwhere(diff)[:5]
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} values differ, first at {idx.tolist()}: "
                             f"got {g[tuple(idx[0])]!r} want {o[tuple(idx[0])]!r}")


def col_major(a) -> np.ndarray:
    """4x4 (row, column) matrix -> the 16 column-major floats of pt_mesh.model_matrix."""
    return np.ascontiguousarray(np.asarray(a, np.float64).T.ravel(), dtype=np.float32)


def translation(t) -> np.ndarray:
    a = np.eye(4)
    a[:3, 3] = t
    return col_major(a)


def rot_scale_about(c) -> np.ndarray:
    """Rotation about a skew axis and a non-uniform scale, about the point c (the mesh stays where
    it was): normals take the w = 0 path through a matrix that is not a rigid motion."""
    ax = np.array([0.3, 1.0, 0.5])
    ax /= np.linalg.norm(ax)
    th = 0.7
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    A = R @ np.diag([1.3, 0.6, 0.9])
    a = np.eye(4)
    a[:3, :3] = A
    a[:3, 3] = np.asarray(c, np.float64) - A @ np.asarray(c, np.float64)
    return col_major(a)


def moved_scene(sc, mesh, **kw):
    meshes = list(sc.meshes)
    meshes[mesh] = dataclasses.replace(meshes[mesh], **kw)
    return dataclasses.replace(sc, meshes=meshes)


def make(sc, kernel=2, w=W, h=H, **kw):
    from optixpathtracer_amd.renderer import setup_renderer

    return setup_renderer(sc, w, h, DEPTH, kernel=kernel, **kw)


def render(r, first=FIRST, n=FRAMES):
    r.stats_reset()
    r.accum_clear()
    r.render_frames(first, n)
    return r.accum(), r.stats()["segments"]


def fresh_render(sc, kernel=2, w=W, h=H):
    r = make(sc, kernel, w, h)
    out = render(r)
    r.close()
    return out


_ORACLE = {}


def oracle(key, sc, w=W, h=H):
    """The oracle's image and segment count of a moved scene, computed once per key."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_render(sc, w, h, DEPTH, FIRST, FRAMES)
    return _ORACLE[key]


def sphere_moves(sc, mesh):
    c = np.asarray(sc.meshes[mesh].vertices, np.float64).mean(axis=0)
    # the last step goes back from object-space normals (a general matrix) to baked ones
    t = translation([0.35, 0.1, -0.2])
    return [("translate", t), ("rot_scale", rot_scale_about(c)), ("translate", t)]


def check_refit_sequence(variant, kernel):
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene(variant)
    mesh = 1
    r = make(sc, kernel)
    before, _ = render(r)
    for name, M in sphere_moves(sc, mesh):
        r.set_mesh_transform(mesh, M)
        r.commit_geometry("refit")
        img, seg = render(r)
        moved = moved_scene(sc, mesh, model=M)
        fimg, fseg = fresh_render(moved, kernel)
        oimg, oseg = oracle((variant, name), moved)
        assert (img != before).any(), f"{name}: the move changed nothing"
        before = img
        assert_identical(img, fimg, f"{variant} {name} vs fresh")
        assert_identical(img, oimg, f"{variant} {name} vs oracle")
        assert seg == fseg == oseg
        np.testing.assert_array_equal(r.model.meshes[mesh].model, M)  # r.model follows, with copies
        np.testing.assert_array_equal(sc.meshes[mesh].model, np.eye(4, dtype=np.float32).ravel())
    r.close()


@pytest.mark.parametrize("kernel", [0, 1], ids=["mega", "wavefront"])
@pytest.mark.parametrize("variant", ["diffuse", "conductor"])
def test_transform_refit_matches_fresh_and_oracle(variant, kernel):
    check_refit_sequence(variant, kernel)


def test_transform_refit_layered_wavefront():
    check_refit_sequence("layered", 1)


def squashed(m):
    v = np.asarray(m.vertices, np.float64)
    c = v.mean(axis=0)
    s = np.array([1.0, 0.5, 1.25])
    nv = (c + (v - c) * s).astype(np.float32)
    nn = np.asarray(m.normals, np.float64) / s
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(np.float32)
    return nv, nn


@pytest.mark.parametrize("with_normals", [True, False], ids=["normals", "keep_normals"])
def test_vertex_update_refit(with_normals):
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")
    mesh = 2
    nv, nn = squashed(sc.meshes[mesh])
    old_vertices = sc.meshes[mesh].vertices.copy()
    r = make(sc)
    render(r)
    if with_normals:
        r.set_mesh_vertices(mesh, nv, nn)
        moved = moved_scene(sc, mesh, vertices=nv, normals=nn)
    else:
        r.set_mesh_vertices(mesh, nv)  # normals=None: the old normals stay
        moved = moved_scene(sc, mesh, vertices=nv)
    r.commit_geometry("refit")
    img, seg = render(r)
    np.testing.assert_array_equal(sc.meshes[mesh].vertices, old_vertices)  # the caller's scene is not touched
    np.testing.assert_array_equal(r.model.meshes[mesh].vertices, nv)
    np.testing.assert_array_equal(r.model.meshes[mesh].normals, moved.meshes[mesh].normals)
    r.close()
    fimg, fseg = fresh_render(moved)
    oimg, oseg = oracle(("squash", with_normals), moved)
    assert_identical(img, fimg, "vertex update vs fresh")
    assert_identical(img, oimg, "vertex update vs oracle")
    assert seg == fseg == oseg


def test_rebuild_reproduces_a_fresh_build():
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")
    M = translation([0.35, 0.1, -0.2])
    r = make(sc)
    r.set_mesh_transform(1, M)
    r.commit_geometry("rebuild")
    f = make(moved_scene(sc, 1, model=M))
    for a, b, what in zip(r.bvh_arrays(), f.bvh_arrays(), ("nodes", "triangle records")):
        assert a.tobytes() == b.tobytes(), what
    sr, sf = r.stats(), f.stats()
    assert sr["bvh_nodes"] == sf["bvh_nodes"] and sr["bvh_depth"] == sf["bvh_depth"]
    assert sr["bvh_sah_cost"] == sr["bvh_sah_cost_built"] == sf["bvh_sah_cost"] == sf["bvh_sah_cost_built"]
    assert sr["bvh_sah_cost"] > 1.0
    assert sr["geometry_rebuilds"] == 1 and sr["geometry_refits"] == 0
    assert_identical(render(r)[0], render(f)[0], "rebuilt vs fresh image")
    r.close()
    f.close()


def test_refit_invariants():
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")
    r = make(sc)
    nodes0, recs0 = r.bvh_arrays()
    cost0 = r.stats()["bvh_sah_cost"]
    assert len(nodes0) > 5 and r.stats()["bvh_depth"] >= 3  # several levels, as the refit walks them
    # an identity refit re-bakes the mesh and recomputes every box: nothing may change
    r.set_mesh_transform(1, np.eye(4, dtype=np.float32).ravel())
    r.commit_geometry("refit")
    nodes1, recs1 = r.bvh_arrays()
    assert nodes1.tobytes() == nodes0.tobytes() and recs1.tobytes() == recs0.tobytes()
    assert r.stats()["bvh_sah_cost"] == cost0 == r.stats()["bvh_sah_cost_built"]
    # a real move
    c = np.asarray(sc.meshes[1].vertices, np.float64).mean(axis=0)
    M = rot_scale_about(c)
    r.set_mesh_transform(1, M)
    r.commit_geometry("refit")
    nodes, recs = r.bvh_arrays()
    f = make(moved_scene(sc, 1, model=M))
    _, frecs = f.bvh_arrays()
    f.close()
    r.close()
    np.testing.assert_array_equal(nodes[:, 24:28], nodes0[:, 24:28])  # child links are never written
    assert (recs != recs0).any()
    # the record of every original triangle equals the fresh renderer's record of that triangle
    by_orig, fby_orig = recs[np.argsort(recs[:, 3])], frecs[np.argsort(frecs[:, 3])]
    np.testing.assert_array_equal(by_orig[:, 3], np.arange(len(recs), dtype=np.uint32))
    assert by_orig.tobytes() == fby_orig.tobytes()
    child = nodes[:, 24:28].view(np.int32)
    for n, (elo, ehi) in enumerate(expected_child_boxes(nodes, recs)):
        lo, hi = stored_child_boxes(nodes, n)
        assert lo.tobytes() == elo.tobytes() and hi.tobytes() == ehi.tobytes(), f"node {n}"
        for k in range(4):
            if child[n, k] == EMPTY:
                assert (lo[k] == np.inf).all() and (hi[k] == -np.inf).all()


def _small_scenes():
    """(name, scene, mesh to move): one triangle (the root is a single leaf); a quad and a triangle
    (one node); the same with a mesh of zero triangles, moved itself or left alone."""
    from optixpathtracer_amd import scenes

    base = scenes.tiny_scene("diffuse")
    tri = scenes._mesh_from_blender(np.array([[0.0, -0.6, 0.4], [0.0, 0.6, 0.4], [0.0, 0.0, 1.5]]),
                                    np.tile([1.0, 0.0, 0.0], (3, 1)), np.array([[0, 1, 2]]), albedo=(0.7, 0.3, 0.2))
    floor = next(m for m in base.meshes if m.name == "floor")
    empty = dataclasses.replace(tri, indices=np.zeros((0, 3), np.int32), name="empty")
    with_meshes = lambda meshes: dataclasses.replace(base, meshes=meshes)
    return [("one_triangle", with_meshes([tri]), 0),
            ("quad_and_triangle", with_meshes([floor, tri]), 1),
            ("empty_mesh_moved", with_meshes([floor, empty, tri]), 1),
            ("empty_mesh_beside", with_meshes([floor, empty, tri]), 2)]


@pytest.mark.parametrize("case", range(4), ids=["one_triangle", "quad_and_triangle", "empty_mesh_moved",
                                                "empty_mesh_beside"])
def test_edge_sizes(case):
    _, sc, mesh = _small_scenes()[case]
    M = translation([0.2, -0.15, 0.3])
    moved = moved_scene(sc, mesh, model=M)
    f = make(moved)
    fimg, fseg = render(f)
    fnodes, frecs = f.bvh_arrays()
    f.close()
    for how in ("refit", "rebuild"):
        r = make(sc)
        render(r)
        r.set_mesh_transform(mesh, M)
        r.commit_geometry(how)
        img, seg = render(r)
        nodes, recs = r.bvh_arrays()
        r.close()
        assert_identical(img, fimg, f"{how} vs fresh")
        assert seg == fseg
        assert recs[np.argsort(recs[:, 3])].tobytes() == frecs[np.argsort(frecs[:, 3])].tobytes()
        if how == "rebuild":
            assert nodes.tobytes() == fnodes.tobytes() and recs.tobytes() == frecs.tobytes()


def test_lit_table_follows_the_geometry():
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")  # Lambert: the lit table is on by default
    shadow = translation([1.0, 0.0, -0.8])  # sphere 0 out over floor cells that were lit
    r = make(sc)
    before, _ = render(r)
    assert r.lit_table()[0]["active"] == 1
    r.set_mesh_transform(0, shadow)
    r.commit_geometry("refit")
    img, seg = render(r)
    assert r.stats()["lit_table_answers"] > 0
    moved = moved_scene(sc, 0, model=shadow)
    oimg, oseg = oracle("lit_shadow", moved)
    assert (img != before).any()
    assert_identical(img, oimg, "lit table after a refit vs oracle")
    assert seg == oseg
    # after a rebuild the table's cut equals a fresh renderer's
    r.set_mesh_transform(0, shadow)
    r.commit_geometry("rebuild")
    f = make(moved)
    info, tri_words, _ = r.lit_table()
    finfo, ftri_words, _ = f.lit_table()
    f.close()
    assert info["active"] == finfo["active"] == 1
    assert info["cells"] == finfo["cells"] and info["triangles"] == finfo["triangles"]
    np.testing.assert_array_equal(tri_words, ftri_words)
    assert_identical(render(r)[0], oimg, "lit table after a rebuild vs oracle")
    # a mesh beyond 128 units switches the table off; the image is still right
    far = translation([200.0, 0.0, 0.0])
    r.set_mesh_transform(0, far)
    r.commit_geometry("refit")
    assert r.lit_table()[0]["active"] == 0
    img, _ = render(r)
    assert r.stats()["lit_table_answers"] == 0
    assert_identical(img, oracle("lit_far", moved_scene(sc, 0, model=far))[0], "table off vs oracle")
    # and back inside switches it on again
    r.set_mesh_transform(0, shadow)
    r.commit_geometry("refit")
    assert r.lit_table()[0]["active"] == 1
    img, _ = render(r)
    assert r.stats()["lit_table_answers"] > 0
    assert_identical(img, oimg, "table on again vs oracle")
    r.close()


def test_textured_mesh_refit():
    from optixpathtracer_amd import scenes

    sc = scenes.textured_scene("diffuse")
    mesh = next(i for i, m in enumerate(sc.meshes) if m.name == "back")  # albedo cut-outs and a normal map
    assert sc.meshes[mesh].albedo_tex >= 0 and sc.meshes[mesh].normal_tex >= 0
    M = translation([0.3, 0.05, -0.1])
    r = make(sc)
    before, _ = render(r)
    r.set_mesh_transform(mesh, M)
    r.commit_geometry("refit")
    img, seg = render(r)
    r.close()
    oimg, oseg = oracle("textured_back", moved_scene(sc, mesh, model=M))
    assert (img != before).any()
    assert_identical(img, oimg, "textured refit vs oracle")
    assert seg == oseg


def test_render_ahead_serves_no_stale_frame():
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")
    M = translation([0.35, 0.1, -0.2])
    r = make(sc)
    r.set_render_ahead(8)
    for _ in range(4):
        r.Render()
    st0 = r.stats()
    assert st0["frames_rendered_ahead"] > 4  # frames of the old geometry wait in the ring
    r.set_mesh_transform(1, M)
    r.commit_geometry("refit")
    fid = r.frame_id
    img = r.Render().copy()
    st1 = r.stats()
    f = make(moved_scene(sc, 1, model=M))
    f.set_render_ahead(1)
    f.frame_id = fid
    fimg = f.Render().copy()
    assert f.frame_id == r.frame_id
    f.close()
    r.close()
    assert_identical(img, fimg, "first Render() after the commit vs fresh")
    # the call rendered its frame anew (or a look-ahead batch was cancelled): nothing came from the old ring
    assert (st1["frames_rendered_ahead"] > st0["frames_rendered_ahead"]
            or st1["look_ahead_cancelled"] > st0["look_ahead_cancelled"])


def test_trace_rays_after_refit():
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")
    c = np.asarray(sc.meshes[3].vertices, np.float64).mean(axis=0)
    M = rot_scale_about(c)
    moved = moved_scene(sc, 3, model=M)
    rays = random_rays(moved, 4096, seed=11)
    r = make(sc)
    r.set_mesh_transform(3, M)
    r.commit_geometry("refit")
    f = make(moved)
    got, want = r.trace_rays(rays), f.trace_rays(rays)
    hit = want[0] >= 0
    assert hit.sum() > 500 and (~hit).sum() > 100
    np.testing.assert_array_equal(got[0], want[0])
    for g, w, name in zip(got[1:], want[1:], ("t", "u", "v", "backface")):
        assert g[hit].tobytes() == w[hit].tobytes(), name
    # any-hit: which triangle ends the ray depends on the tree; whether one does, does not
    np.testing.assert_array_equal(r.trace_rays(rays, any_hit=True)[0] >= 0, f.trace_rays(rays, any_hit=True)[0] >= 0)
    r.close()
    f.close()


def test_staging_errors_and_stats():
    from optixpathtracer_amd import capi, scenes
    from optixpathtracer_amd.capi import PTError

    sc = scenes.tiny_scene("diffuse")
    r = make(sc)
    before, _ = render(r)
    st = r.stats()
    assert st["geometry_commits"] == 0 and st["geometry_commit_ms"] == 0.0
    assert st["bvh_sah_cost"] == st["bvh_sah_cost_built"] > 1.0
    r.commit_geometry("refit")  # nothing staged: a no-op
    r.commit_geometry("rebuild")
    assert r.stats()["geometry_commits"] == 0
    ident = np.eye(4, dtype=np.float32).ravel()
    for bad in (-1, len(sc.meshes)):
        with pytest.raises(PTError):
            r.set_mesh_transform(bad, ident)
        with pytest.raises(PTError):
            r.set_mesh_vertices(bad, sc.meshes[0].vertices)
    with pytest.raises(PTError):
        r.commit_geometry("bogus")
    assert r.lib.pt_commit_geometry(r.h, 7) == capi.PT_ERR_INVALID
    assert r.lib.pt_set_mesh_transform(r.h, 0, None) == capi.PT_ERR_INVALID
    assert r.lib.pt_set_mesh_vertices(r.h, 0, None, None) == capi.PT_ERR_INVALID
    assert r.stats()["geometry_commits"] == 0
    # staged, not committed: the image does not change
    far = translation([50.0, 0.0, 0.0])
    r.set_mesh_transform(1, far)
    assert_identical(render(r)[0], before, "staged but uncommitted")
    r.commit_geometry("refit")
    st = r.stats()
    assert (st["geometry_commits"], st["geometry_refits"], st["geometry_rebuilds"]) == (1, 1, 0)
    assert st["geometry_commit_ms"] > 0.0
    # one sphere far outside the box stretches the boxes above it: the refitted tree costs more
    assert st["bvh_sah_cost"] > st["bvh_sah_cost_built"]
    assert (render(r)[0] != before).any()
    r.set_mesh_transform(1, far)
    r.commit_geometry("rebuild")
    st = r.stats()
    assert (st["geometry_commits"], st["geometry_refits"], st["geometry_rebuilds"]) == (2, 1, 1)
    assert st["bvh_sah_cost"] == st["bvh_sah_cost_built"]
    r.close()


def test_one_rank_multi_device_refit():
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")
    M = translation([0.35, 0.1, -0.2])
    r = make(sc, devices=[0])
    render(r)
    r.set_mesh_transform(1, M)
    r.commit_geometry("refit")
    img, seg = render(r)
    r.close()
    oimg, oseg = oracle(("diffuse", "translate"), moved_scene(sc, 1, model=M))
    assert_identical(img, oimg, "device-list renderer after a refit vs oracle")
    assert seg == oseg
