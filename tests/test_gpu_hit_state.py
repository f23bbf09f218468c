"""The wavefront trace loop keeps a ray's running hit in its lane's LDS slot (pt_device.h TriBatchLds,
hit_slot_*): the 64-bit key (t bits, original index) lives there from fetch to finish and the batch's
atomic min is the whole closest-hit update; a shadow ray's slot carries its contribution and the ray
is occluded iff its key moved.

  * ties across rounds and batches: 12 coincident copies of one triangle, each a mesh of its own with
    its own albedo (more copies than a leaf holds, so equal-t candidates meet the running key in
    different rounds and batches), a neighbour sharing an edge, a wall behind and a floor below; mesh
    order as given and reversed (the winning copy, hence the image, changes with the order);
  * equality at tmax: a point light in the plane of a triangle, inside its outline, so the shadow
    rays end on the triangle within a rounding of their length; lit and occluder tables off, so every
    NEE test is a traced shadow ray;
    both bit-identical to the CPU oracle at 96x64, depth 4, 8 frames in one batch, in Lambert and
    Dielectric.  The oracle's image is first checked on its own: finite, and (ties) the camera ray
    through the copies' centroid returns the copy with the lowest original index;
  * slot reuse: the tiny open scene at 320x240, 16 frames in one batch: 1.2 M paths over the 6144
    resident waves of an MI355X are some 200 rays per wave, so every lane is refilled several times,
    misses (the open front) follow hits in the same lane, and the wave whose slice spans the end of
    the extension rays holds both ray kinds.  The accumulator's SHA-256 is the same on one and two
    wavefront streams (768- and 256-thread trace workgroups), with traversal statistics on, with the
    lit, occluder and skip tables forced on and forced off, and with the primary dedup off.
"""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, DEPTH, FRAMES = 96, 64, 4, 8
LAMBERT, DIELECTRIC = 1, 3
MODES = {"lambert": LAMBERT, "dielectric": DIELECTRIC}
N_COPIES = 12
# Blender coordinates (scenes.blender_to_engine); the camera of scenes.SCENE1_CAMERA looks along -x
TRI = [(0.5, -0.8, 0.3), (0.5, 0.6, 0.3), (0.5, -0.1, 1.7)]
NEIGHBOUR = [(0.5, 0.6, 0.3), (0.5, 1.3, 1.7), (0.5, -0.1, 1.7)]  # shares the edge TRI[1]-TRI[2]
PANEL = [(1.0, -1.0, 0.2), (1.0, 1.0, 0.2), (1.0, 0.0, 1.9)]
PANEL_LIGHT = (1.0, 0.0, 0.8)  # in the panel's plane x = 1 (exact in fp32), inside its outline


def _tri_mesh(pts, albedo, name):
    from optixpathtracer_amd import scenes

    v = scenes.blender_to_engine(np.array(pts, np.float32))
    n = scenes.blender_to_engine(np.tile(np.array([1.0, 0.0, 0.0], np.float32), (3, 1)))
    return scenes.Mesh(vertices=np.ascontiguousarray(v, np.float32), indices=np.array([[0, 1, 2]], np.int32),
                       normals=np.ascontiguousarray(n, np.float32), albedo=albedo, name=name)


def _room():
    """A wall behind (x = -0.6) and a floor (z = -0.6), as in scenes.sphere_in_box."""
    from optixpathtracer_amd import scenes

    x0, x1, y0, y1, z0, z1 = -0.6, 2.4, -1.8, 1.8, -0.6, 2.6
    out = []
    for name, pts, nrm in (("back", [(x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)], (1, 0, 0)),
                           ("floor", [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)], (0, 0, 1))):
        v, n, idx = scenes.quad(*pts, nrm)
        out.append(scenes.Mesh(vertices=np.ascontiguousarray(scenes.blender_to_engine(v), np.float32),
                               indices=np.ascontiguousarray(idx, np.int32),
                               normals=np.ascontiguousarray(scenes.blender_to_engine(n), np.float32),
                               albedo=(0.5, 0.5, 0.5), name=name))
    return out


def _scene(meshes, lights_blender, name):
    from optixpathtracer_amd import scenes

    lights = np.array([[*scenes.blender_to_engine(p), 1.0, 1.0, 1.0] for p in lights_blender], np.float32)
    return scenes.Scene(meshes=meshes, lights=lights, camera_blender_pos=scenes.SCENE1_CAMERA[0],
                        camera_blender_rot=scenes.SCENE1_CAMERA[1], material_mode=LAMBERT, name=name)


def ties_scene(reverse=False):
    from optixpathtracer_amd import scenes

    copies = [_tri_mesh(TRI, (0.05 + 0.08 * k, 0.9 - 0.07 * k, 0.3), f"copy_{k}") for k in range(N_COPIES)]
    meshes = _room() + copies + [_tri_mesh(NEIGHBOUR, (0.7, 0.2, 0.7), "neighbour")]
    if reverse:
        meshes = meshes[::-1]
    return _scene(meshes, scenes.SCENE1_LIGHTS_BLENDER, "hit_state_ties" + ("_reversed" if reverse else ""))


def tmax_scene():
    from optixpathtracer_amd import scenes

    meshes = _room() + [_tri_mesh(PANEL, (0.6, 0.6, 0.2), "panel")]
    return _scene(meshes, [PANEL_LIGHT, scenes.SCENE1_LIGHTS_BLENDER[2]], "hit_state_tmax")


def _gpu(sc, w, h, mode, frames, streams=None, stats=False, tables=None, lit_occ_off=False, dedup=True):
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(sc, w, h, DEPTH, kernel=1)  # the wavefront
    r.set_material_mode(mode)
    r.set_frames_per_launch(frames)  # one batch
    if streams is not None:
        r.set_wavefront_streams(streams)
    r.set_traversal_stats(stats)
    if tables is not None:
        r.set_lit_table(tables)
        r.set_occluder_table(tables)
        r.set_skip_table(tables)
    if lit_occ_off:
        r.set_lit_table(False)
        r.set_occluder_table(False)
    if not dedup:
        r.set_primary_dedup(False)
    r.accum_clear()
    r.render_frames(1, frames)
    img = r.accum()
    r.close()
    return img


def _oracle(sc, mode):
    from helpers import oracle_render

    ref, _ = oracle_render(sc, W, H, DEPTH, 1, FRAMES, mode=mode)
    assert np.isfinite(ref).all(), f"{sc.name}: the oracle's image is not finite"
    assert ref.max() > 0.0, f"{sc.name}: the oracle's image is black"
    return ref


def _identical(g, ref, what):
    diff = g != ref
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {diff.size} values differ from the oracle, "
                            f"max abs {float(np.abs(g.astype(np.float64) - ref).max()):.3e}")


def copies_visible(sc):
    """The oracle alone: the camera ray through the copies' centroid hits the coincident copy with the
    lowest original index (original index = position in the concatenated mesh order)."""
    from optixpathtracer_amd import scenes
    from oracle.oracle import OracleScene, camera_from_blender

    cam, _, _ = camera_from_blender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg, W, H)
    c = scenes.blender_to_engine(np.mean(np.array(TRI, np.float32), axis=0))
    d = (c - cam) / np.linalg.norm(c - cam)
    o = OracleScene(sc)
    prim, t, _, _, _ = o.trace(np.array([[*cam, *d, 0.0, 100.0]], np.float32))
    o.close()
    first, copy_ids = 0, []
    for m in sc.meshes:
        if m.name.startswith("copy_"):
            copy_ids.append(first)
        first += m.n_triangles
    return int(prim[0]), copy_ids


@pytest.fixture(scope="module")
def oracle_images():
    """The oracle's accumulators per (scene, mode): computed once, never modified."""
    cache = {}

    def get(name, sc, mode):
        if (name, mode) not in cache:
            cache[(name, mode)] = _oracle(sc, mode)
        return cache[(name, mode)]

    return get


@pytest.mark.parametrize("reverse", [False, True], ids=["as_given", "reversed"])
@pytest.mark.parametrize("mode", list(MODES))
def test_ties_across_rounds_and_batches(oracle_images, mode, reverse):
    sc = ties_scene(reverse)
    prim, copy_ids = copies_visible(sc)
    assert len(copy_ids) == N_COPIES and prim == min(copy_ids), (prim, copy_ids)
    ref = oracle_images(sc.name, sc, MODES[mode])
    _identical(_gpu(sc, W, H, MODES[mode], FRAMES), ref, f"{sc.name} {mode}")


@pytest.mark.parametrize("mode", list(MODES))
def test_equality_at_tmax(oracle_images, mode):
    sc = tmax_scene()
    ref = oracle_images(sc.name, sc, MODES[mode])
    _identical(_gpu(sc, W, H, MODES[mode], FRAMES, lit_occ_off=True), ref, f"{sc.name} {mode}")


REUSE_W, REUSE_H, REUSE_FRAMES = 320, 240, 16
REUSE_VARIANTS = {
    "two_streams": dict(streams=2),
    "stats": dict(streams=1, stats=True),
    "tables_on": dict(streams=1, tables=True),
    "tables_off": dict(streams=1, tables=False),
    "stats_tables_off": dict(streams=1, stats=True, tables=False),
    "two_streams_tables_off": dict(streams=2, tables=False),
    "no_dedup": dict(streams=1, dedup=False),
}


@pytest.fixture(scope="module")
def reuse_base():
    """The tiny open scene on one stream, everything else by default: its accumulator's SHA-256."""
    from optixpathtracer_amd import scenes

    img = _gpu(scenes.tiny_scene("diffuse"), REUSE_W, REUSE_H, LAMBERT, REUSE_FRAMES, streams=1)
    assert np.isfinite(img).all() and float(np.asarray(img).max()) > 0.0
    return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()


@pytest.mark.parametrize("variant", list(REUSE_VARIANTS))
def test_slot_reuse(reuse_base, variant):
    from optixpathtracer_amd import scenes

    img = _gpu(scenes.tiny_scene("diffuse"), REUSE_W, REUSE_H, LAMBERT, REUSE_FRAMES, **REUSE_VARIANTS[variant])
    sha = hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()
    assert sha == reuse_base, f"{variant}: accumulator SHA-256 {sha} != {reuse_base} of the one-stream default"
