"""The lit table (pt_lit.h, pt_lit.hip, pt_set_lit_table): one bit per (point light, surface cell),
set only where every NEE shadow ray from the cell toward the light is provably unoccluded, so the
wavefront shading kernels add the light's contribution without tracing.

  * conservative: every set bit is sampled at its cell's corners, centroid and 8 interior points, the
    shadow rays are built as the shading kernels build them, and none may hit, neither for the GPU
    tracer (every ray of every set bit) nor for the CPU oracle (its per-ray Python loop traces ~1e5
    rays a second, so it gets kOracleRays rays per case, up to half of them from set cells next to
    a cleared one, where a wrong bit would sit);
  * images: table on, table off and the oracle give the same bits in all five material modes;
  * invalidation: new lights through pt_set_lights, through pt_launch, 0 / 1 / 17 lights, a light
    beyond the coordinate bound, and a light change under a speculative render-ahead batch.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 48, 8
F = np.float32
kOracleRays = 60_000
kNoCells = 0xFF

# engine coordinates: the box spans x [-0.6, 2.4], y [-0.6, 2.6], z [-1.8, 1.8]
LIGHT_SETS = {
    "standard": None,  # the scene's four lights
    "near_wall": [[1.0, 1.0, 1.797, 1, 1, 1]],      # 3 mm in front of the z = 1.8 wall
    "outside": [[-1.5, 1.0, 0.2, 1, 1, 1]],         # behind the back wall (x = -0.6)
    "in_wall_plane": [[1.0, 1.0, 1.8, 1, 1, 1]],    # in the plane of the z = 1.8 wall
}


def _scene(name):
    from optixpathtracer_amd import scenes

    return scenes.tiny_scene("diffuse") if name == "tiny" else scenes.textured_scene("diffuse")


def _world_tris(sc):
    parts = []
    for m in sc.meshes:
        M = np.asarray(m.model, F).reshape(4, 4, order="F")
        v = (np.c_[m.vertices, np.ones(len(m.vertices), F)] @ M.T).astype(F)
        parts.append(v[m.indices.reshape(-1), :3].reshape(-1, 3, 3))
    return np.concatenate(parts).astype(F)


def _cell_corners(k, c):
    """Vectorised lit_cell_corners: (n, 3) grid coordinates cu, cv."""
    N = np.int64(1) << k
    r = N * N - c
    s = np.ceil(np.sqrt(r.astype(np.float64))).astype(np.int64)
    s += (s * s < r)
    s -= ((s - 1) * (s - 1) >= r)
    j = N - s
    rem = c - j * (2 * N - j)
    i, up = rem >> 1, (rem & 1).astype(bool)
    cu = np.where(up[:, None], np.stack([i + 1, i + 1, i], 1), np.stack([i, i + 1, i], 1))
    cv = np.where(up[:, None], np.stack([j, j + 1, j + 1], 1), np.stack([j, j, j + 1], 1))
    return cu, cv


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _shadow_rays(v0, v1, v2, u, v, light, delta):
    """The shading kernels' shadow ray (pt_wavefront.hip k_shade_fused, pt_shade.h reconstruct) in
    fp32: p = w v0 + u v1 + v v2, Ng = normalize(cross(v1 - v0, v2 - v0)) on the light's side, origin
    p + 1e-3 Ng, direction normalize(l - p), tmax = |l - p|.  Returns the rays and dot(l - p, Ng)."""
    u, v = u[:, None], v[:, None]
    w = F(1) - u - v
    p = (w * v0 + u * v1 + v * v2).astype(F)
    e1, e2 = v1 - v0, v2 - v0
    ng = np.stack([e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0],
                   e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]], 1).astype(F)
    ng = ng * (F(1) / np.sqrt(_dot(ng, ng)))[:, None]
    ldir = (light[None, :] - p).astype(F)
    side = _dot(ldir, ng)
    ng = np.where((side < 0)[:, None], -ng, ng)
    o = p + F(1e-3) * ng
    tmax = np.sqrt(_dot(ldir, ldir))
    d = ldir * (F(1) / tmax)[:, None]
    rays = np.concatenate([o, d, np.zeros((len(o), 1), F), tmax[:, None]], 1).astype(F)
    return rays, np.abs(side)


def _set_bit_rays(info, tri_words, bits_row, recs, wtris, light, rng, cells):
    """Rays of the 12 sample points of every cell in `cells` (all of them set for this light)."""
    first = (tri_words & 0xFFFFFF).astype(np.int64)
    level = (tri_words >> 24).astype(np.int64)
    has = level != kNoCells
    idx = np.flatnonzero(has)
    t = idx[np.searchsorted(first[idx], cells, side="right") - 1]
    k = level[t]
    local = cells - first[t]
    assert (local >= 0).all() and (local < (np.int64(1) << (2 * k))).all()
    cu, cv = _cell_corners(k, local)
    n = len(cells)
    bary = np.concatenate([np.eye(3), np.full((1, 3), 1 / 3), rng.dirichlet(np.ones(3), 8)])  # 12 x 3
    N = (np.int64(1) << k).astype(np.float64)[:, None]
    gu = (cu.astype(np.float64) @ bary.T) / N  # n x 12
    gv = (cv.astype(np.float64) @ bary.T) / N
    u, v = gu.astype(F).ravel(), gv.astype(F).ravel()
    orig = recs[:, 3].view(np.int32)[t]
    tri = np.repeat(wtris[orig], 12, axis=0)
    assert np.array_equal(wtris[orig][:, 0], recs[t, 0:3].view(F))  # v0 as the tracer holds it
    rays, side = _shadow_rays(tri[:, 0], tri[:, 1], tri[:, 2], u, v, light.astype(F), info["delta"])
    assert (side > info["delta"]).all()  # a set bit: the light is above the plane by more than delta
    return rays, np.repeat(np.arange(n), 12)


@pytest.mark.parametrize("lights_name", list(LIGHT_SETS))
@pytest.mark.parametrize("scene_name", ["tiny", "textured"])
def test_set_bits_are_unoccluded(scene_name, lights_name):
    from optixpathtracer_amd.renderer import setup_renderer
    from oracle.oracle import OracleScene

    sc = _scene(scene_name)
    lights = sc.lights if LIGHT_SETS[lights_name] is None else np.asarray(LIGHT_SETS[lights_name], F)
    r = setup_renderer(sc, W, H, DEPTH)
    r.SetLights(lights)
    info, tri_words, bits = r.lit_table()
    assert info["active"] == 1 and info["lights"] == len(lights) and info["triangles"] == sc.n_triangles
    assert 0 < info["delta"] < 1e-3 and info["margin"] > 1e-3
    level = tri_words >> 24
    ncell = np.where(level == kNoCells, 0, np.uint64(1) << (2 * level.astype(np.uint64))).astype(np.int64)
    assert int(ncell.sum()) == info["cells"]  # N^2 cells per triangle, packed in triangle order
    assert np.array_equal((tri_words & 0xFFFFFF).astype(np.int64), np.cumsum(ncell) - ncell)
    _, recs = r.bvh_arrays()
    wtris = _world_tris(sc)
    o = OracleScene(sc)
    rng = np.random.default_rng(11)
    shares = []
    for li in range(len(lights)):
        flat = np.unpackbits(bits[li].view(np.uint8), bitorder="little")[: info["cells"]].astype(bool)
        cells = np.flatnonzero(flat).astype(np.int64)
        shares.append(len(cells) / info["cells"])
        # not vacuous: every light that lights a surface from the front has bits set.  The light in
        # the wall's plane does not: each of its shadow rays ends at l + 1e-3 Ng, in or beyond that
        # wall's plane, so whether the wall occludes it is a matter of rounding and no bit may be set
        assert len(cells) > 0 or lights_name == "in_wall_plane", f"light {li}: no bit set"
        if len(cells) == 0:
            continue
        hit_cells = 0
        for a in range(0, len(cells), 100_000):
            chunk = cells[a:a + 100_000]
            rays, owner = _set_bit_rays(info, tri_words, bits[li], recs, wtris, lights[li, :3], rng, chunk)
            prim = r.trace_rays(rays, any_hit=True)[0]
            hit_cells += len(np.unique(owner[prim >= 0]))
        assert hit_cells == 0, f"light {li}: {hit_cells} set cells with an occluded shadow ray (GPU tracer)"
        # the oracle: set cells beside a cleared one first, then a random share of the rest
        edge = cells[(~flat[np.minimum(cells + 1, info["cells"] - 1)]) | (~flat[np.maximum(cells - 1, 0)])]
        per = kOracleRays // len(lights) // 12
        pick = np.concatenate([rng.permutation(edge)[: per // 2], rng.permutation(cells)[: per - min(per // 2, len(edge))]])
        rays, _ = _set_bit_rays(info, tri_words, bits[li], recs, wtris, lights[li, :3], rng, np.sort(pick))
        assert (o.trace(rays, any_hit=True)[0] < 0).all(), f"light {li}: an oracle shadow ray of a set cell hits"
    print(f"lit table {scene_name}/{lights_name}: cells {info['cells']}, set share per light "
          f"{[round(s, 4) for s in shares]}, margin {info['margin']:.5f}")
    o.close()
    r.close()


def _render(sc, mode, lit, streams=1, lights=None, n=5, first=1):
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_material_mode(mode)
    r.set_frames_per_launch(2)  # 5 frames: batches of 2, 2 and a ragged 1
    r.set_wavefront_streams(streams)
    r.set_lit_table(lit)
    if lights is not None:
        r.SetLights(lights)
    r.accum_clear()
    r.render_frames(first, n)
    img, st = r.accum(), r.stats()
    r.close()
    return img, st


@pytest.fixture(scope="module")
def oracle_images():
    """Oracle sums of frames 1..5 at 64x48, depth 8, per material mode (computed once)."""
    from optixpathtracer_amd import scenes
    from oracle.oracle import OracleScene

    sc = scenes.tiny_scene("conductor")  # metallic spheres, dielectric walls: every mode's branches
    o = OracleScene(sc)
    out = {m: o.render(o.launch(W, H, DEPTH, material_mode=m), 1, 5)[0] for m in range(5)}
    o.close()
    return sc, out


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4], ids=["default", "lambert", "conductor", "dielectric", "layered"])
def test_images_unchanged(oracle_images, mode, streams):
    sc, ref = oracle_images
    on, st_on = _render(sc, mode, True, streams)
    off, st_off = _render(sc, mode, False, streams)
    np.testing.assert_array_equal(on, off)
    np.testing.assert_array_equal(on, ref[mode])
    assert st_on["lit_table_answers"] > 0 and st_off["lit_table_answers"] == 0
    assert st_on["lit_table_cells"] > 0 and 0 < st_on["lit_table_bits_set"] <= 4 * st_on["lit_table_cells"]
    assert st_on["lit_table_bytes"] > 0
    # the table's answers replace traced shadow rays one for one
    assert st_on["shadow_rays"] + st_on["lit_table_answers"] == st_off["shadow_rays"]
    assert st_on["segments"] == st_off["segments"]


def _moved(lights):
    out = np.array(lights, F, copy=True)
    out[:, 0] += F(0.35)
    out[:, 2] *= F(-0.6)
    return out


@pytest.mark.parametrize("mode", [1, 0], ids=["lambert", "default"])
def test_set_lights_rebuilds(mode):
    """pt_set_lights between two renders, then 1, 0 and 17 lights: every image equals the one of a
    fresh renderer that only ever saw the final lights (and, transitively, the table-off image)."""
    from optixpathtracer_amd import scenes
    from optixpathtracer_amd.renderer import setup_renderer

    sc = scenes.tiny_scene("conductor")
    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_material_mode(mode)
    r.set_frames_per_launch(2)
    r.accum_clear()
    r.render_frames(1, 3)  # the table of the first lights is built and used
    assert r.stats()["lit_table_answers"] > 0
    many = np.concatenate([_moved(sc.lights)] * 5)[:17].copy()
    many[:, 1] += np.linspace(0, 0.5, 17, dtype=F)
    for lights, active in ((_moved(sc.lights), 1), (_moved(sc.lights)[:1], 1), (np.zeros((0, 6), F), 0), (many, 0)):
        r.SetLights(lights)
        assert r.lit_table()[0]["active"] == active
        r.stats_reset()
        r.accum_clear()
        r.render_frames(4, 3)
        got, st = r.accum(), r.stats()
        assert (st["lit_table_answers"] > 0) == bool(active)
        for lit in (True, False):
            want, _ = _render(sc, mode, lit, lights=lights, n=3, first=4)
            np.testing.assert_array_equal(got, want)
    r.close()


@pytest.mark.parametrize("forced", [True, False], ids=["on", "auto"])
def test_launch_params_lights_rebuild(forced):
    """pt_launch carries its own device light array.  With the table forced on it follows the array
    call by call, and the renderer's own lights get their table back afterwards; in auto a pt_launch
    neither uses nor rebuilds the table (one frame cannot pay for a build), and the table of the
    renderer's own lights stays as built."""
    import ctypes as C

    from optixpathtracer_amd import scenes
    from optixpathtracer_amd.renderer import camera_from_blender, setup_renderer

    hip = C.CDLL("libamdhip64.so.7")
    sc = scenes.tiny_scene("diffuse")
    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.set_render_ahead(1)  # every Render() renders: none is served from frames rendered ahead
    if forced:
        r.set_lit_table(True)
    ref_own = r.Render()  # frame 1, the scene's lights
    own = r.stats()
    assert own["lit_table_answers"] > 0 and own["lit_table_bits_set"] > 0
    r.stats_reset()
    p, iv, ip = camera_from_blender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg, W, H)
    ptrs = []

    def dev(nbytes):
        q = C.c_void_p()
        assert hip.hipMalloc(C.byref(q), C.c_size_t(nbytes)) == 0
        ptrs.append(q.value)
        return q.value

    d_lights, d_img = dev(sc.lights.nbytes), dev(W * H * 3 * 4)
    for k, lights in enumerate((_moved(sc.lights), sc.lights.astype(F))):  # same array, new contents
        arr = np.ascontiguousarray(lights, F)
        assert hip.hipMemcpy(C.c_void_p(d_lights), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1) == 0
        r.launch(d_img, (W, H), 7 + k, p, iv, ip, d_lights, len(lights), DEPTH)
        r.synchronize()
        got = np.empty((H, W, 3), F)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), C.c_void_p(d_img), C.c_size_t(got.nbytes), 2) == 0
        want, _ = _render(sc, 1, False, lights=lights, n=1, first=7 + k)
        np.testing.assert_array_equal(got, want)
    st = r.stats()
    assert (st["lit_table_answers"] > 0) == forced
    if not forced:  # the own lights' table was neither used nor touched
        assert st["lit_table_bits_set"] == own["lit_table_bits_set"] and st["lit_table_build_ms"] == own["lit_table_build_ms"]
    r.frame_id = 0
    np.testing.assert_array_equal(r.Render(), ref_own)
    assert r.stats()["lit_table_answers"] > 0
    for q in ptrs:
        hip.hipFree(C.c_void_p(q))
    r.close()


def test_far_light_has_no_bits_and_stats_follow_the_switch():
    """A light beyond the coordinate bound (128 units) gets no bits, one within it keeps its own; the
    image equals the traced one.  The table's pt_stats figures are reported only while it is in use."""
    from optixpathtracer_amd import scenes
    from optixpathtracer_amd.renderer import setup_renderer

    sc = scenes.tiny_scene("diffuse")
    lights = np.array([[1.0, 1.0, 0.5, 1, 1, 1], [1.0, 2.0e4, 0.5, 3e8, 3e8, 3e8], [129.0, 1.0, 0.5, 1, 1, 1]], F)
    r = setup_renderer(sc, W, H, DEPTH, kernel=1)
    r.SetLights(lights)
    info, _, bits = r.lit_table()
    assert info["active"] == 1 and bits[0].any() and not bits[1].any() and not bits[2].any()
    r.accum_clear()
    r.render_frames(1, 3)
    got, st = r.accum(), r.stats()
    want, st_off = _render(sc, 1, False, lights=lights, n=3)
    np.testing.assert_array_equal(got, want)
    assert st["lit_table_answers"] > 0 and st["lit_table_cells"] == info["cells"] and st["lit_table_bytes"] > 0
    assert st_off["lit_table_cells"] == 0 and st_off["lit_table_bits_set"] == 0 and st_off["lit_table_bytes"] == 0
    assert st_off["lit_table_build_ms"] == 0
    r.set_lit_table(False)
    st = r.stats()
    assert st["lit_table_cells"] == 0 and st["lit_table_bits_set"] == 0 and st["lit_table_build_ms"] == 0
    r.close()


def test_light_change_under_a_speculative_batch():
    """Render-ahead keeps a speculative batch in flight (held by pt_set_debug_hold); new lights
    cancel it and rebuild the table behind it: the following frames equal the table-off renderer's."""
    from optixpathtracer_amd import scenes
    from optixpathtracer_amd.renderer import setup_renderer

    sc = scenes.tiny_scene("diffuse")
    shape = (H, W, 3)
    a = setup_renderer(sc, W, H, DEPTH)
    b = setup_renderer(sc, W, H, DEPTH)
    b.set_lit_table(False)
    for r in (a, b):
        r.set_render_ahead_budget(0)  # the ramp reaches 64 frames: call 64 enqueues the next 64 ahead
    a.set_debug_hold(True)
    fa = [a.Render(np.empty(shape, F)).copy() for _ in range(64)]
    a.SetLights(_moved(sc.lights))  # the look-ahead batch waits in k_hold
    a.set_debug_hold(False)
    st = a.stats()
    assert st["look_ahead_held"] == 1 and st["look_ahead_cancelled"] == 1
    fa += [a.Render(np.empty(shape, F)).copy() for _ in range(4)]
    # the table-off renderer replays the calls afterwards (its allocations would wait for the held batch)
    for k in range(68):
        if k == 64:
            b.SetLights(_moved(sc.lights))
        np.testing.assert_array_equal(fa[k], b.Render(np.empty(shape, F)))
    assert a.stats()["lit_table_answers"] > 0 and b.stats()["lit_table_answers"] == 0
    for r in (a, b):
        r.close()
