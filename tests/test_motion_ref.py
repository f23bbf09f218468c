"""The motion-vector restatement on the CPU (motion_ref.py, DESIGN.md §11 "Motion vectors"): a hit's
barycentrics applied to the scene's own triangles give the oracle's position bit for bit; without a
previous position the restatement is temporal_ref's; following a moved wall accepts its history
where the plain reprojection resets it; and pixels off the moved mesh do not notice."""
import functools

import numpy as np
import pytest
from denoise_ref import same_bits, scene_by_name
from motion_ref import (left_multiplied, mesh_of_triangle, motion_ref, oracle_guides, prev_position, translation, wall_matrix,
                        world_triangles)
from temporal_ref import camera_of, oracle_view, temporal_ref

W, H = 48, 32
WALL = 4  # tiny:diffuse's back wall


@pytest.mark.parametrize("name", ["tiny:diffuse", "textured:diffuse"])
def test_own_triangles_give_the_position(name):
    """(a) prev_position over a scene's own triangles is the oracle's position, before and after a move of mesh 0."""
    sc = scene_by_name(name)
    for scene in (sc, left_multiplied(sc, 0, translation(0.2, 0.1, -0.15))):
        g = oracle_guides(scene, W, H)
        pp = prev_position(world_triangles(scene), g["prim"], g["u"], g["v"])
        hit = g["prim"] >= 0
        assert hit.any()
        equal = (pp.view(np.uint32) == g["position"].view(np.uint32)).all(-1)
        assert equal.all(), (int(equal.sum()), equal.size)
        assert (g["u"][~hit] == 0).all() and (g["v"][~hit] == 0).all()


@pytest.mark.parametrize("iterations", [1, 5])
def test_without_motion_it_is_temporal_ref(iterations):
    """(b) No previous position, or one equal to the position: temporal_ref's output and state over
    the six-camera sequence of test_gpu_temporal.py (pans, a cut, NaN and inf inputs)."""
    from test_gpu_temporal import CAMERAS, NAME, _images

    keys = ["normal", "position", "inv_view", "inv_proj", "length", "moments", "variance", "color", "color_variance"]
    st = [None, None, None]
    for k, img in enumerate(_images(W, H)):
        g, cam = oracle_view(NAME, *CAMERAS[k], W, H)
        want, st[0] = temporal_ref(st[0], img, g, cam, iterations=iterations)
        for j, pp in ((1, None), (2, g["position"])):
            got, st[j] = motion_ref(st[j], img, g, cam, prev_pos=pp, iterations=iterations)
            assert same_bits(got, want), (k, j)
            assert [q for q in keys if not same_bits(st[j][q], st[0][q])] == [], (k, j)
            assert (st[j]["valid"] == st[0]["valid"]).all()
            assert (st[j]["reprojected"], st[j]["reset"], st[j]["moved"]) == (st[0]["reprojected"], st[0]["reset"], 0)
            assert same_bits(st[j]["prev_position"], g["position"])


@functools.lru_cache(maxsize=None)
def _wall_case():
    """Two static calls on tiny:diffuse, then the wall moves: the third call with and without the previous position."""
    sc = scene_by_name("tiny:diffuse")
    cam = camera_of(sc, W, H)
    rng = np.random.default_rng(21)
    imgs = [rng.random((H, W, 3)).astype(np.float32) for _ in range(3)]
    g0 = oracle_guides(sc, W, H)
    st = None
    for img in imgs[:2]:
        _, st = motion_ref(st, img, g0, cam)
    moved = left_multiplied(sc, WALL, wall_matrix())
    g1 = oracle_guides(moved, W, H)
    pp = prev_position(world_triangles(sc), g1["prim"], g1["u"], g1["v"])
    _, on = motion_ref(st, imgs[2], g1, cam, prev_pos=pp)
    _, off = motion_ref(st, imgs[2], g1, cam)
    on_wall = (g1["prim"] >= 0) & (mesh_of_triangle(moved)[np.clip(g1["prim"], 0, None)] == WALL)
    return g1, on, off, on_wall


def test_following_the_wall_keeps_its_history():
    """(c) With the previous position at least 95 % of the wall's pixels take up history, without it
    at most 70 % (measured: 1018 of 1018 against 600 of 1018)."""
    g1, on, off, on_wall = _wall_case()
    n = int(on_wall.sum())
    a_on, a_off = int(on["accepted"][on_wall].sum()), int(off["accepted"][on_wall].sum())
    print(f"wall pixels={n} accepted with={a_on} without={a_off} moved={on['moved']}")
    assert n >= 900
    assert a_on >= 0.95 * n
    assert a_off <= 0.70 * n
    assert on["moved"] >= a_on and off["moved"] == 0


def test_pixels_off_the_moved_mesh_do_not_notice():
    """(d) The history length of every pixel not on the moved mesh is the same either way, and so is its previous position."""
    g1, on, off, on_wall = _wall_case()
    assert (~on_wall).any()
    assert same_bits(on["length"][~on_wall], off["length"][~on_wall])
    assert same_bits(on["prev_position"][~on_wall], g1["position"][~on_wall])
