"""The lit table with the per-cell margin (pt_lit.h lit_margin_cell): a cell's pyramid is grown by
2e-3 + 1.01 * 2^-12 * (min(reach, diag) + 2e-3) instead of the scene-wide 2e-3 + diag * 2^-10, so
bits are set closer to every shadow's edge.  The tracer is the check on that derivation:

  * every set bit of a blocker scene (one large triangle over a floor, the light above it), of a
    2 x 2 box of coarse spheres and of the tiny scene is sampled at its three corners pulled inward
    by one part in 1e4 and at 16 random points; the shadow rays are built as the shading kernels
    build them, and none may hit for the library's tracer.  Every set bit is checked, none is
    sampled away;
  * on the blocker scene the floor under the triangle's interior has no bit, the floor outside its
    shadow has, and bits reach as close to the shadow's edge as the cell's own margin allows, closer
    than the scene-wide margin did;
  * the images equal the oracle's in all five material modes (streams 1 and 2 in Lambert and
    Default), table answers replace shadow rays one for one;
  * new lights rebuild the bits, and the image still equals the oracle's.

The single-triangle "dark" proof of the same header is not built into the table (the
host probe's stop rule); tests/test_lit_dark_host.py checks its predicate on the host.
"""
import dataclasses

import numpy as np
import pytest

from test_gpu_lit_table import _cell_corners, _shadow_rays, _world_tris, kNoCells

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 64, 8
F = np.float32
kRandom = 16


kLeg = -0.5965625  # the blocker's two straight edges (Blender x and y); their shadows lie at 2 * kLeg


def blocker_scene():
    """A 4 x 4 floor at z = 0 (Blender axes), a right triangle at z = 1 with its legs along x = kLeg
    and y = kLeg, and a light at (0, 0, 2): the shadow is the triangle scaled by 2, with straight
    edges at x = 2 kLeg and y = 2 kLeg across the floor."""
    from optixpathtracer_amd import scenes
    from optixpathtracer_amd.capi import PT_MAT_LAMBERT

    v, n, idx = scenes.quad((-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0), (0, 0, 1))
    floor = scenes._mesh_from_blender(v, n, idx, albedo=(0.6, 0.6, 0.6), metallic=0.0, roughness=0.5, name="floor")
    tv = np.array([(kLeg, kLeg, 1.0), (2.4, kLeg, 1.0), (kLeg, 2.4, 1.0)])
    tn = np.tile(np.array([0.0, 0.0, 1.0]), (3, 1))
    tidx = scenes._orient(tv, np.array([[0, 1, 2]], dtype=np.int64), tn[:1])
    tri = scenes._mesh_from_blender(tv, tn, tidx, albedo=(0.7, 0.2, 0.2), metallic=0.3, roughness=0.4, name="blocker")
    lights = np.array([[*scenes.blender_to_engine((0.0, 0.0, 2.0)), 4.0, 4.0, 4.0]], dtype=F)
    return scenes.Scene(meshes=[floor, tri], lights=lights, camera_blender_pos=(5.0, 0.0, 8.0),
                        camera_blender_rot=(32.0, 0.0, 90.0), material_mode=PT_MAT_LAMBERT, name="blocker")


def _scene(name):
    from optixpathtracer_amd import scenes

    if name == "blocker":
        return blocker_scene()
    if name == "box2":
        return scenes.sphere_in_box("diffuse", sphere_segments=8, sphere_rings=4, grid=2)
    return scenes.tiny_scene("conductor")  # metallic spheres, dielectric walls: every mode's branches


def _cells_of(tri_words, cells):
    first = (tri_words & 0xFFFFFF).astype(np.int64)
    level = (tri_words >> 24).astype(np.int64)
    idx = np.flatnonzero(level != kNoCells)
    t = idx[np.searchsorted(first[idx], cells, side="right") - 1]
    return t, level[t], cells - first[t]


def _rays_of_cells(info, tri_words, recs, wtris, light, rng, cells):
    """Shadow rays of 3 pulled-in corners and kRandom random points of every cell in `cells`."""
    t, k, local = _cells_of(tri_words, cells)
    cu, cv = _cell_corners(k, local)
    pull = 1e-4
    bary = np.concatenate([np.eye(3) * (1 - pull) + pull / 3, rng.dirichlet(np.ones(3), kRandom)])
    per = len(bary)
    N = (np.int64(1) << k).astype(np.float64)[:, None]
    u = ((cu.astype(np.float64) @ bary.T) / N).astype(F).ravel()
    v = ((cv.astype(np.float64) @ bary.T) / N).astype(F).ravel()
    orig = recs[:, 3].view(np.int32)[t]
    tri = np.repeat(wtris[orig], per, axis=0)
    rays, side = _shadow_rays(tri[:, 0], tri[:, 1], tri[:, 2], u, v, light.astype(F), info["delta"])
    assert (side > info["delta"]).all()
    return rays, np.repeat(np.arange(len(cells)), per)


@pytest.mark.parametrize("scene_name", ["blocker", "box2", "tiny"])
def test_every_set_bit_is_unoccluded(scene_name):
    from optixpathtracer_amd.renderer import setup_renderer

    sc = _scene(scene_name)
    r = setup_renderer(sc, W, H, DEPTH)
    info, tri_words, bits = r.lit_table()
    assert info["active"] == 1 and info["lights"] == len(sc.lights)
    _, recs = r.bvh_arrays()
    wtris = _world_tris(sc)
    rng = np.random.default_rng(5)
    total = 0
    for li in range(len(sc.lights)):
        flat = np.unpackbits(bits[li].view(np.uint8), bitorder="little")[: info["cells"]].astype(bool)
        cells = np.flatnonzero(flat).astype(np.int64)
        assert len(cells) > 0
        total += len(cells)
        bad = 0
        for a in range(0, len(cells), 50_000):
            rays, owner = _rays_of_cells(info, tri_words, recs, wtris, sc.lights[li, :3], rng, cells[a:a + 50_000])
            prim = r.trace_rays(rays, any_hit=True)[0]
            bad += len(np.unique(owner[prim >= 0]))
        assert bad == 0, f"light {li}: {bad} set cells with an occluded shadow ray"
        if scene_name == "blocker":
            _check_blocker_classes(info, tri_words, recs, wtris, flat)
    print(f"{scene_name}: {total} set bits of {info['cells'] * len(sc.lights)} (light, cell) pairs checked, "
          f"margin bound {info['margin']:.5f}")
    r.close()


def _check_blocker_classes(info, tri_words, recs, wtris, flat):
    """Floor cells by their centroid (Blender x, y = engine x, -z).  Well inside the shadow: no bit.
    Well outside its two straight edges: bits, though not everywhere -- a bit needs one of the cell's
    own three side planes to separate the blocker, and only some of a cell's edge directions face it.
    Close to the edge x = 2 kLeg: the floor's cells are 4 / 256 wide (level 8), a grid line lies
    0.010 outside that edge, and a cell ending there has its side plane 4.3e-3 from the blocker:
    more than its own margin (2.8e-3), less than the scene-wide lit_margin(diag) (8.2e-3).  Its
    centroid is 0.0152 from the edge; with the scene-wide margin the nearest bit sat at 0.031."""
    cells = np.arange(info["cells"], dtype=np.int64)
    t, k, local = _cells_of(tri_words, cells)
    orig = recs[:, 3].view(np.int32)[t]
    floor = orig < 2  # the floor's two triangles come first in the scene
    assert (k[floor] == 8).all()
    cu, cv = _cell_corners(k, local)
    N = (np.int64(1) << k).astype(np.float64)
    gu, gv = cu.sum(1) / (3 * N), cv.sum(1) / (3 * N)
    tri = wtris[orig].astype(np.float64)
    c = (1 - gu - gv)[:, None] * tri[:, 0] + gu[:, None] * tri[:, 1] + gv[:, None] * tri[:, 2]
    x, y = c[:, 0], -c[:, 2]
    xs = ys = 2 * kLeg
    hyp = 2 * (2.4 + kLeg)  # the shadow's slanted edge: x + y = hyp
    inside = floor & (x > xs + 0.1) & (y > ys + 0.1) & (x + y < hyp - 0.15)
    outside = floor & ((x < xs - 0.1) | (y < ys - 0.1))
    near = floor & (x < xs) & (x > xs - 0.02) & (y > -1.0) & (y < 1.8)
    assert inside.sum() > 1000 and outside.sum() > 1000 and near.sum() > 100
    assert not flat[inside].any(), "a lit bit under the blocker"
    assert flat[outside].mean() > 0.25, "too few bits outside the shadow"
    assert flat[near].any(), "no bit within 0.02 of the shadow's edge: the margin is not the cell's own"


def _render(sc, mode, lit, streams=1, lights=None, n=5):
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_material_mode(mode)
    r.set_frames_per_launch(2)
    r.set_wavefront_streams(streams)
    r.set_lit_table(lit)
    if lights is not None:
        r.SetLights(lights)
    r.accum_clear()
    r.render_frames(1, n)
    img, st = r.accum(), r.stats()
    r.close()
    return img, st


@pytest.fixture(scope="module")
def oracle_images():
    """Oracle sums of frames 1..5 at 64 x 64, depth 8, per scene and material mode (computed once)."""
    from oracle.oracle import OracleScene

    out = {}
    for name in ("blocker", "box2"):
        sc = _scene(name)
        o = OracleScene(sc)
        out[name] = (sc, {m: o.render(o.launch(W, H, DEPTH, material_mode=m), 1, 5)[0] for m in range(5)})
        o.close()
    return out


MODES = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (3, 1), (4, 1)]


@pytest.mark.parametrize("mode,streams", MODES, ids=[f"{'default lambert conductor dielectric layered'.split()[m]}-{s}"
                                                     for m, s in MODES])
@pytest.mark.parametrize("scene_name", ["blocker", "box2"])
def test_images_unchanged(oracle_images, scene_name, mode, streams):
    sc, ref = oracle_images[scene_name]
    on, st_on = _render(sc, mode, True, streams)
    off, st_off = _render(sc, mode, False, streams)
    np.testing.assert_array_equal(on, ref[mode])
    np.testing.assert_array_equal(on, off)
    assert st_on["lit_table_answers"] > 0 and st_off["lit_table_answers"] == 0
    assert st_on["shadow_rays"] + st_on["lit_table_answers"] == st_off["shadow_rays"]
    assert st_on["segments"] == st_off["segments"]


def test_rebuild_on_a_light_change():
    from optixpathtracer_amd.renderer import setup_renderer
    from oracle.oracle import OracleScene

    sc = blocker_scene()
    moved = sc.lights.copy()
    moved[0, 0] += F(0.7)  # the shadow moves along the floor
    moved[0, 2] -= F(0.4)
    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_material_mode(1)
    # batches of 2 and a ragged 1, as in _render: a one-frame batch has no bounce-0 (pixel, light)
    # table, so its first hits ask the lit table (in this open scene few later bounces hit anything)
    r.set_frames_per_launch(2)
    r.set_lit_table(True)
    before = r.lit_table()[2].copy()
    r.SetLights(moved)
    after = r.lit_table()[2]
    assert before.any() and after.any() and not np.array_equal(before, after)
    r.accum_clear()
    r.render_frames(1, 3)
    got, st = r.accum(), r.stats()
    assert st["lit_table_answers"] > 0
    r.close()
    o = OracleScene(dataclasses.replace(sc, lights=moved))
    want = o.render(o.launch(W, H, DEPTH, material_mode=1), 1, 3)[0]
    o.close()
    np.testing.assert_array_equal(got, want)
