"""The occluder candidate table (pt_lit.hip k_occ_build, pt_set_occluder_table): one triangle index
per (point light, surface cell) that probably occludes the cell's shadow rays.  Before a shading
kernel emits a shadow ray the lit table left open, it tests that one triangle with the tracer's own
tri_test + tri_accept on the very ray; a hit is the tracer's "occluded", so the ray is dropped.

  * images: table on, table off and the oracle give the same bits in all five material modes, on
    one and two wavefront streams, and on the textured scene (cut-outs);
  * the central claim: the answer is exact for ANY entry -- random triangle indices in every entry
    give the same bits, and all -1 gives the same bits with no answer at all;
  * counters: an answer replaces one traced, occluded shadow ray;
  * lifetime: new lights, a refit and a BVH rebuild (new leaf order) each leave a table whose images
    equal a fresh renderer's, with every entry -1 or a triangle of the scene.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 48, 8  # as tests/test_gpu_lit_table.py
F = np.float32
MODE_IDS = ["default", "lambert", "conductor", "dielectric", "layered"]
OCC_MODES = (0, 1, 4)  # the kernels that carry the test: k_shade_a (Default, Layered), k_shade_fused<Lambert>


def _scene(name):
    from optixpathtracer_amd import scenes

    return {"tiny": lambda: scenes.tiny_scene("conductor"), "tiny_diffuse": lambda: scenes.tiny_scene("diffuse"),
            "textured": lambda: scenes.textured_scene("diffuse")}[name]()


def _make(sc, mode, occ, streams=1, lights=None):
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_material_mode(mode)
    r.set_frames_per_launch(2)  # 5 frames: batches of 2, 2 and a ragged 1
    r.set_wavefront_streams(streams)
    r.set_lit_table(True)
    r.set_occluder_table(occ)
    if lights is not None:
        r.SetLights(lights)
    return r


def _frames(r, n=5, first=1):
    r.stats_reset()
    r.accum_clear()
    r.render_frames(first, n)
    return r.accum(), r.stats()


def _render(sc, mode, occ, streams=1, lights=None, n=5, first=1):
    r = _make(sc, mode, occ, streams, lights)
    out = _frames(r, n, first)
    r.close()
    return out


@pytest.fixture(scope="module")
def oracle_images():
    """Oracle sums of frames 1..5 at 64x48, depth 8: the tiny scene in every material mode, the
    textured scene in the modes whose kernels carry the test (computed once, never modified)."""
    from oracle.oracle import OracleScene

    out = {}
    for name, modes in (("tiny", range(5)), ("textured", OCC_MODES)):
        sc = _scene(name)
        o = OracleScene(sc)
        out[name] = (sc, {m: o.render(o.launch(W, H, DEPTH, material_mode=m), 1, 5)[0] for m in modes})
        o.close()
    return out


def _check_on_off(sc, ref, mode, streams):
    on, st_on = _render(sc, mode, True, streams)
    off, st_off = _render(sc, mode, False, streams)
    np.testing.assert_array_equal(on, off)
    np.testing.assert_array_equal(on, ref)
    print(f"mode {mode} streams {streams}: shadow rays {st_off['shadow_rays']} -> {st_on['shadow_rays']}, "
          f"answers {st_on['occluder_table_answers']}, candidates {st_on['occluder_table_candidates']}")
    assert st_off["occluder_table_answers"] == 0 and st_off["occluder_table_bytes"] == 0
    assert st_off["occluder_table_candidates"] == 0 and st_off["occluder_table_build_ms"] == 0
    if mode in OCC_MODES:
        assert st_on["occluder_table_answers"] > 0
        assert st_on["occluder_table_bytes"] == 4 * st_on["lit_table_cells"] * len(sc.lights)
        assert 0 < st_on["occluder_table_candidates"] <= st_on["lit_table_cells"] * len(sc.lights)
    else:  # Conductor, Dielectric: the code is compiled out of their kernels, the table is not built
        assert st_on["occluder_table_answers"] == 0 and st_on["occluder_table_bytes"] == 0
    # an answer replaces one traced shadow ray; the lit table's answers are the same on both sides
    assert st_on["lit_table_answers"] == st_off["lit_table_answers"] > 0
    assert st_on["shadow_rays"] + st_on["occluder_table_answers"] == st_off["shadow_rays"]
    assert st_on["segments"] == st_off["segments"]


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4], ids=MODE_IDS)
def test_images_unchanged(oracle_images, mode, streams):
    sc, ref = oracle_images["tiny"]
    _check_on_off(sc, ref[mode], mode, streams)


@pytest.mark.parametrize("mode", OCC_MODES, ids=[MODE_IDS[m] for m in OCC_MODES])
def test_images_unchanged_textured(oracle_images, mode):
    sc, ref = oracle_images["textured"]
    _check_on_off(sc, ref[mode], mode, 1)


@pytest.mark.parametrize("mode", [1, 0], ids=["lambert", "default"])
@pytest.mark.parametrize("scene_name", ["tiny", "textured"])
def test_any_entry_gives_the_same_image(oracle_images, scene_name, mode):
    """The table is a hint: whatever triangle an entry names, a passing test is the tracer's answer."""
    from optixpathtracer_amd import capi

    sc, ref = oracle_images[scene_name]
    r = _make(sc, mode, True)
    built, st = _frames(r)
    np.testing.assert_array_equal(built, ref[mode])
    tab = r.occluder_table()
    ntri = st["triangles"]
    assert tab.dtype == np.int32 and tab.shape == (st["lit_table_cells"] * len(sc.lights),)
    assert tab.min() >= -1 and tab.max() < ntri and (tab >= 0).sum() == st["occluder_table_candidates"]
    if scene_name == "textured":  # no candidate is a cut-out triangle (E2.w of its isect record)
        recs = r.bvh_arrays()[1]
        assert not recs[tab[tab >= 0], 11].any() and recs[:, 11].any()
    rnd = np.random.default_rng(61).integers(0, ntri, size=tab.shape, dtype=np.int32)
    r.upload_occluder_table(rnd)
    np.testing.assert_array_equal(r.occluder_table(), rnd)
    img, st_rnd = _frames(r)
    np.testing.assert_array_equal(img, built)
    assert st_rnd["occluder_table_candidates"] == tab.size
    assert st_rnd["shadow_rays"] + st_rnd["occluder_table_answers"] == st["shadow_rays"] + st["occluder_table_answers"]
    r.upload_occluder_table(np.full(tab.shape, -1, np.int32))
    img, st_none = _frames(r)
    np.testing.assert_array_equal(img, built)
    assert st_none["occluder_table_answers"] == 0 and st_none["occluder_table_candidates"] == 0
    assert st_none["shadow_rays"] == st["shadow_rays"] + st["occluder_table_answers"]
    print(f"{scene_name} mode {mode}: answers built {st['occluder_table_answers']}, random {st_rnd['occluder_table_answers']}")
    # out-of-range entries are rejected and nothing is written
    for bad in (ntri, -2, np.iinfo(np.int32).max):
        e = np.full(tab.shape, -1, np.int32)
        e[e.size // 2] = bad
        with pytest.raises(capi.PTError):
            r.upload_occluder_table(e)
    with pytest.raises(capi.PTError):
        r.upload_occluder_table(np.full(tab.size - 1, -1, np.int32))
    np.testing.assert_array_equal(r.occluder_table(), np.full(tab.shape, -1, np.int32))
    r.close()


def test_counter_invariants():
    """One render_frames call on the tiny Lambert scene, traversal statistics on (they count
    nee_unoccluded): only occluded rays disappear."""
    sc = _scene("tiny_diffuse")
    st = {}
    for occ in (True, False):
        r = _make(sc, 1, occ)
        r.set_traversal_stats(True)
        r.stats_reset()
        r.accum_clear()
        r.render_frames(1, 5)
        st[occ] = r.stats()
        r.close()
    on, off = st[True], st[False]
    print(f"shadow rays {off['shadow_rays']} -> {on['shadow_rays']}, lit answers {on['lit_table_answers']}, "
          f"occluder answers {on['occluder_table_answers']}, unoccluded {on['nee_unoccluded']}")
    assert off["occluder_table_answers"] == 0
    assert (on["shadow_rays"] + on["lit_table_answers"] + on["occluder_table_answers"]
            == off["shadow_rays"] + off["lit_table_answers"] + off["occluder_table_answers"])
    assert on["nee_unoccluded"] == off["nee_unoccluded"] > 0
    assert on["occluder_table_answers"] > 0


def test_auto_follows_the_lit_table():
    """Auto: on in Lambert while the lit table is itself in auto; a lit table forced on or off leaves
    the candidates to their own switch; the figures are reported only while the table is in use."""
    from optixpathtracer_amd.renderer import setup_renderer

    sc = _scene("tiny_diffuse")
    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_material_mode(1)
    _, st = _frames(r)
    assert st["occluder_table_answers"] > 0 and st["occluder_table_bytes"] > 0
    r.set_lit_table(True)
    _, st = _frames(r)
    assert st["occluder_table_answers"] == 0 and st["occluder_table_bytes"] == 0 and r.occluder_table() is None
    r.set_occluder_table(True)
    r.set_lit_table(False)  # no lit table, no candidates
    _, st = _frames(r)
    assert st["occluder_table_answers"] == 0 and st["occluder_table_bytes"] == 0 and r.occluder_table() is None
    r.close()


def _moved(lights):
    out = np.array(lights, F, copy=True)
    out[:, 0] += F(0.35)
    out[:, 2] *= F(-0.6)
    return out


@pytest.mark.parametrize("mode", [1, 0], ids=["lambert", "default"])
def test_set_lights_rebuilds(mode):
    sc = _scene("tiny")
    r = _make(sc, mode, True)
    _frames(r, 3)
    old = r.occluder_table()
    lights = _moved(sc.lights)
    r.SetLights(lights)
    got, st = _frames(r, 3, 4)
    assert st["occluder_table_answers"] > 0
    fresh = _make(sc, mode, True, lights=lights)
    want, _ = _frames(fresh, 3, 4)
    np.testing.assert_array_equal(got, want)
    new = r.occluder_table()
    np.testing.assert_array_equal(new, fresh.occluder_table())  # same scene, same lights: the same build
    assert (new != old).any()
    fresh.close()
    off, _ = _render(sc, mode, False, lights=lights, n=3, first=4)
    np.testing.assert_array_equal(got, off)
    r.close()


def _translation(t):
    m = np.eye(4, dtype=F)
    m[:3, 3] = t
    return np.ascontiguousarray(m.T).ravel()  # column-major


@pytest.mark.parametrize("how", ["refit", "rebuild"])
@pytest.mark.parametrize("mode", [1, 0], ids=["lambert", "default"])
def test_mesh_moved(mode, how):
    """A moved mesh, by a refit (the leaf order stays) and by a rebuild (a new leaf order: stale
    entries would name other triangles, or none)."""
    sc = _scene("tiny")
    mesh, M = 1, _translation([0.35, 0.1, -0.2])
    r = _make(sc, mode, True)
    before, st0 = _frames(r)
    r.set_mesh_transform(mesh, M)
    r.commit_geometry(how)
    got, st = _frames(r)
    assert (got != before).any() and st["occluder_table_answers"] > 0
    tab = r.occluder_table()
    assert tab.min() >= -1 and tab.max() < st["triangles"] and (tab >= 0).any()
    meshes = list(sc.meshes)
    meshes[mesh] = dataclasses.replace(meshes[mesh], model=M)
    moved = dataclasses.replace(sc, meshes=meshes)
    for occ in (True, False):
        want, _ = _render(moved, mode, occ)
        np.testing.assert_array_equal(got, want)
    r.close()
