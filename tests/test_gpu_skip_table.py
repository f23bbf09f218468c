"""The skip table (pt_skip.h, pt_set_skip_table): per (triangle, side) one BVH4 subtree at or below the
triangle's plane, which an extension ray that climbs from that side drops unvisited.

  * bit identity at 96x54, 8 frames, depth 8 on the coarse sphere box (8x4 spheres: the shading normals
    differ from the face normals, so rays that dip below the geometric plane fall back to "none"):
    Lambert (auto) and Conductor and Dielectric forced on give the accumulators of the table off, bit
    for bit; so do the textured scene, a scene of one planar mesh, and a renderer whose sphere was moved
    (against a fresh renderer of the moved scene); and the same three modes on two open hemispheres,
    one wound outward and one inward (skip_ref.open_shells), where the reference alone first shows that
    the other side's word would drop triangles the rays hit;
  * traversal statistics on the same scene: nodes visited and triangle tests per ray are strictly
    lower with the table, the segments equal, and the rays that carried a skip are more than none and
    fewer than the extension rays;
  * the words: 0 or a link of the tree, two per triangle.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, DEPTH, FRAMES = 96, 54, 8, 8
LAMBERT, CONDUCTOR, DIELECTRIC = 1, 2, 3
MODES = {"lambert": (LAMBERT, None), "conductor": (CONDUCTOR, True), "dielectric": (DIELECTRIC, True)}


def _coarse(variant="diffuse"):
    from optixpathtracer_amd import scenes

    return scenes.sphere_in_box(variant, sphere_segments=8, sphere_rings=4, grid=2)


def _make(sc, mode, skip, stats=False):
    """skip: None = auto, True / False = forced."""
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_material_mode(mode)
    r.set_frames_per_launch(3)  # 8 frames: batches of 3, 3 and a ragged 2
    r.set_skip_table(skip)
    r.set_traversal_stats(stats)
    return r


def _frames(r, first=1, n=FRAMES):
    r.stats_reset()
    r.accum_clear()
    r.render_frames(first, n)
    return r.accum(), r.stats()


def _render(sc, mode, skip, stats=False):
    r = _make(sc, mode, skip, stats)
    out = _frames(r)
    r.close()
    return out


def _identical(a, b, what):
    diff = a != b
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ"


@pytest.fixture(scope="module")
def off_images():
    """The accumulators with the table off, per (scene, mode): computed once, never modified."""
    cache = {}

    def get(name, sc, mode):
        if (name, mode) not in cache:
            cache[(name, mode)] = _render(sc, mode, False)
        return cache[(name, mode)]

    return get


@pytest.fixture(scope="module")
def shells_tell_sides_apart():
    """The reference alone (skip_ref.side_swap_hits on the tree the renderer built, traced by the CPU
    oracle), once: per (hemisphere, side) the (T, side) pairs whose rays hit a triangle under the link
    that the other side's word names.  Where that is positive a swap of the sides changes hits."""
    import skip_ref
    from optixpathtracer_amd.renderer import setup_renderer
    from oracle.oracle import OracleScene

    sc = skip_ref.open_shells()
    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    nodes, tris = r.bvh_arrays()
    r.close()
    o = OracleScene(sc)
    pairs = skip_ref.side_swap_hits(sc, nodes, tris, lambda rays: o.trace(rays)[0])
    o.close()
    return skip_ref.shell_counts(pairs)


@pytest.mark.parametrize("scene,name", [("coarse", m) for m in MODES] + [("open_shells", m) for m in MODES],
                         ids=list(MODES) + [f"open_shells-{m}" for m in MODES])
def test_images_unchanged(off_images, shells_tell_sides_apart, scene, name):
    mode, skip = MODES[name]
    if scene == "open_shells":
        # two open hemispheres, one wound outward and one inward: on a closed convex mesh the wrong
        # side's word names nothing a ray can hit; here it names the bowl the ray is inside of, for a
        # front-face approach (the inward shell's inside, side 0) and a back-face approach (the outward
        # shell's inside, side 1) alike
        import skip_ref

        sc = skip_ref.open_shells()
        print(f"open shells: (T, side) pairs that a side swap would change: {shells_tell_sides_apart}")
        assert shells_tell_sides_apart[("bowl_outward", 1)] > 0 and shells_tell_sides_apart[("dome_inward", 0)] > 0
    else:
        sc = _coarse()
    off, st_off = off_images(scene, sc, mode)
    on, st_on = _render(sc, mode, skip)
    _identical(on, off, f"{scene}, {name}")
    assert off.any()
    assert st_on["segments"] == st_off["segments"] and st_on["shadow_rays"] == st_off["shadow_rays"]
    assert st_off["skip_table_bytes"] == 0 and st_off["skip_table_build_ms"] == 0
    print(f"{name}: skip table {st_on['skip_table_bytes']} B, built in {st_on['skip_table_build_ms']:.3f} ms")
    assert st_on["skip_table_bytes"] == 8 * st_on["triangles"]


@pytest.mark.parametrize("name", list(MODES))
def test_traversal_statistics(name):
    mode, skip = MODES[name]
    sc = _coarse()
    off, st_off = _render(sc, mode, False, stats=True)
    on, st_on = _render(sc, mode, skip, stats=True)
    _identical(on, off, name + " (statistics kernels)")
    assert st_on["segments"] == st_off["segments"]
    assert st_on["rays"] == st_off["rays"] > 0
    per = lambda st, k: st[k] / st["rays"]
    print(f"{name}: nodes/ray {per(st_off, 'nodes_visited'):.3f} -> {per(st_on, 'nodes_visited'):.3f}, "
          f"tri tests/ray {per(st_off, 'tri_tests'):.3f} -> {per(st_on, 'tri_tests'):.3f}, "
          f"skip rays {st_on['skip_table_rays']} of {st_on['segments']} segments")
    assert st_on["nodes_visited"] < st_off["nodes_visited"]
    assert st_on["tri_tests"] < st_off["tri_tests"]
    # the extension rays of the bounces after the camera's: every segment but the W * H * frames primary ones
    extension = st_on["segments"] - W * H * FRAMES
    assert st_off["skip_table_rays"] == 0
    assert 0 < st_on["skip_table_rays"] < extension


def test_images_unchanged_textured(off_images):
    from optixpathtracer_amd import scenes

    sc = scenes.textured_scene("diffuse")
    off, _ = off_images("textured", sc, LAMBERT)
    on, st = _render(sc, LAMBERT, None)
    _identical(on, off, "textured")
    assert st["skip_table_bytes"] > 0


def test_planar_mesh():
    """One planar mesh: both sides of both triangles drop the whole mesh, and the image is the same."""
    sc = _coarse()
    back = [m for m in sc.meshes if m.name == "back"]
    assert len(back) == 1
    flat = dataclasses.replace(sc, meshes=back)
    off, _ = _render(flat, LAMBERT, False)
    r = _make(flat, LAMBERT, True)
    on, st = _frames(r)
    words = r.skip_table()
    r.close()
    _identical(on, off, "planar mesh")
    assert off.any()
    assert words.shape == (2, 2) and (words != 0).all()


def test_words_name_links_of_the_tree():
    r = _make(_coarse(), LAMBERT, None)
    words = r.skip_table()
    st = r.stats()
    r.close()
    assert words.shape == (st["triangles"], 2)
    links = words[words != 0].view(np.int32)
    assert links.size > 0
    inner = links[links >= 0]
    assert (inner > 0).all() and (inner < st["bvh_nodes"]).all()  # the root is nobody's child
    leaves = ~links[links < 0]
    assert ((leaves >> 3) + (leaves & 7) < st["triangles"]).all()


def test_geometry_update_rebuilds_the_words():
    """Move one sphere on a live renderer: its images equal a fresh renderer's of the moved scene, with
    the table and without, after a refit and after a rebuild."""
    sc = _coarse()
    mesh = 1
    a = np.eye(4)
    a[:3, 3] = [0.35, 0.1, -0.2]
    M = np.ascontiguousarray(a.T.ravel(), dtype=np.float32)
    meshes = list(sc.meshes)
    meshes[mesh] = dataclasses.replace(meshes[mesh], model=M)
    moved = dataclasses.replace(sc, meshes=meshes)
    fresh_off, _ = _render(moved, LAMBERT, False)
    fresh_on, _ = _render(moved, LAMBERT, None)
    _identical(fresh_on, fresh_off, "fresh renderer of the moved scene")
    for how in ("refit", "rebuild"):
        r = _make(sc, LAMBERT, None)
        before, _ = _frames(r)
        old = r.skip_table()
        r.set_mesh_transform(mesh, M)
        r.commit_geometry(how)
        img, st = _frames(r)
        new = r.skip_table()
        r.close()
        assert (img != before).any(), "the move changed nothing"
        _identical(img, fresh_off, how)
        assert st["skip_table_bytes"] == 8 * st["triangles"]
        assert new.shape == old.shape and (new != 0).any()
