"""pt_set_pixel_filter on the GPU against the numpy restatement (pixel_filter_ref.py), bit for bit.

With supersample = s every sample is a pixel of an image that the oracle and the plain kernels
already produce at s times the resolution, and the filtered accumulation is a fixed fp32 tap loop:
so the sum buffer can be restated exactly from one-frame images of an sW x sH renderer (given the
same camera triple, computed once for W x H) or of the oracle.  19x17 is more than one 16x16 tile
both ways with ragged edges, so the halo loads, the tile seams and the border clamp all occur; 18
frames from 3 wrap F mod 16 for s = 4, and batches of 5 are ragged.
"""
import numpy as np
import pytest

import pixel_filter_ref as ref
from pixel_filter_ref import BASE, DEFAULT, DIELECTRIC, LAMBERT

pytestmark = pytest.mark.gpu

W, H, DEPTH, FIRST, N, BATCH = (BASE[k] for k in ("w", "h", "depth", "first", "frames", "batch"))
FILTERS = {  # name -> (supersample, kind)
    "box2": (2, "box"), "box4": (4, "box"), "tent4": (4, "tent"), "gaussian4": (4, "gaussian"),
    "mitchell4": (4, "mitchell"), "tent1": (1, "tent"),
}


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    ab, bb = a.view(np.uint8).reshape(a.shape + (-1,)), b.view(np.uint8).reshape(b.shape + (-1,))
    if not np.array_equal(ab, bb):  # the raw bits: a NaN equals itself
        bad = np.argwhere((ab != bb).any(-1))
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ, first at {first}: {a[first]!r} against {b[first]!r}")


FIELDS = ["position", "albedo", "shading_normal", "geometry_normal", "roughness", "metallic", "beta", "radiance"]


def _gpu_records(r):
    """The debug path's records in the oracle's layout (22 floats per bounce)."""
    out = []
    for d in r.debug_path():
        row = [np.int32(d["bounce"]).view(np.float32), np.int32(d["prim"]).view(np.float32)]
        for f in FIELDS:
            v = d[f]
            row += v if isinstance(v, list) else [v]
        out.append(row)
    return np.array(out, np.float32).reshape(-1, 22)


def tiny():
    from optixpathtracer_amd import scenes

    return scenes.tiny_scene("diffuse")


def camera(scene):
    """The camera triple of the W x H image: the virtual renderers and the oracle take this one."""
    from optixpathtracer_amd.renderer import camera_from_blender

    return camera_from_blender(scene.camera_blender_pos, scene.camera_blender_rot, scene.fov_deg, W, H)


def renderer(scene=None, mode=LAMBERT, w=W, h=H, batch=BATCH, **kw):
    from optixpathtracer_amd.renderer import setup_renderer

    scene = scene or tiny()
    r = setup_renderer(scene, w, h, DEPTH, **kw)
    r.SetCamera(*camera(scene))
    r.set_material_mode(mode)
    if batch:
        r.set_frames_per_launch(batch)
    return r


class VirtualFrames:
    """frame(F) of the s-fold image, one render_frames(F, 1) each, from one renderer per (mode, s)."""

    def __init__(self):
        self.renderers, self.cache, self.scenes = {}, {}, {}

    def frames(self, s, mode=LAMBERT, scene_key="tiny", scene=None):
        key = (scene_key, mode, s)
        if key not in self.renderers:
            self.scenes[key] = scene or tiny()
            self.renderers[key] = renderer(self.scenes[key], mode, s * W, s * H, batch=0)

        def frame(f):
            if (key, f) not in self.cache:
                r = self.renderers[key]
                r.accum_clear()
                r.render_frames(f, 1)
                self.cache[key, f] = r.accum()
            return self.cache[key, f]

        return frame

    def close(self):
        for r in self.renderers.values():
            r.close()


@pytest.fixture(scope="module")
def virtual():
    v = VirtualFrames()
    yield v
    v.close()


@pytest.fixture(scope="module")
def want(virtual):
    """The restated sum of the base case per filter name (Lambert), computed once."""
    cache = {}

    def get(name, fp64=False):
        if (name, fp64) not in cache:
            s, kind = FILTERS[name]
            cache[name, fp64] = ref.accumulate(virtual.frames(s), s, FIRST, N, kind, fp64=fp64)
        return cache[name, fp64]

    return get


def run(r, name, first=FIRST, n=N):
    s, kind = FILTERS[name]
    r.set_pixel_filter(s, kind)
    r.accum_clear()
    r.render_frames(first, n)
    return r.accum()


# ---- 1. the box: sub-pixel cells alone ----------------------------------------------------------
@pytest.mark.parametrize("name", ["box2", "box4"])
def test_box_lambert_equals_restatement(name, want):
    r = renderer()
    got = run(r, name)
    assert r.pixel_filter() == {"supersample": FILTERS[name][0], "kind": "box", "radius": 0.5, "param": 0.0}
    r.close()
    same_bits(got, want(name), name)
    assert np.isfinite(got).all() and got.any()


@pytest.mark.parametrize("name", ["box2", "box4"])
def test_box_lambert_equals_restatement_from_oracle_frames(name):
    from oracle.oracle import OracleScene

    s, _ = FILTERS[name]
    sc = tiny()
    o = OracleScene(sc)
    lp = o.launch(s * W, s * H, DEPTH, material_mode=LAMBERT, camera=camera(sc))
    sums = ref.accumulate(lambda f: o.render(lp, f, 1)[0], s, FIRST, N)
    o.close()
    r = renderer()
    got = run(r, name)
    r.close()
    same_bits(got, sums, f"{name}, oracle frames")


@pytest.mark.parametrize("name", ["box2", "box4"])
@pytest.mark.parametrize("mode", [DIELECTRIC, DEFAULT], ids=["dielectric", "default"])
def test_box_other_modes_equal_restatement(mode, name, virtual):
    """Dielectric: two streams by default.  Default: the bucketed kernels, whose k_extend copies the
    primary hit to every frame of the batch under the dedup."""
    s, _ = FILTERS[name]
    r = renderer(mode=mode)
    got = run(r, name)
    r.close()
    same_bits(got, ref.accumulate(virtual.frames(s, mode), s, FIRST, N), f"{name}, mode {mode}")


# ---- 2. the filters ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tent4", "gaussian4", "mitchell4", "tent1"])
def test_filters_equal_restatement(name, want):
    r = renderer()
    got = run(r, name)
    r.close()
    same_bits(got, want(name), name)
    assert np.isfinite(got).all() and got.any()


def test_filters_with_other_radii(virtual):
    """R = 2 for the tent and R = 1 for Mitchell: each kernel instance under the other profile."""
    r = renderer()
    for kind, radius, param in (("tent", 2.5, 0.0), ("mitchell", 1.5, 0.75), ("gaussian", 2.0, 0.8), ("tent", 0.5, 0.0)):
        r.set_pixel_filter(4, kind, radius, param)
        r.accum_clear()
        r.render_frames(FIRST, N)
        same_bits(r.accum(), ref.accumulate(virtual.frames(4), 4, FIRST, N, kind, radius, param), f"{kind} {radius}")
    r.close()


# ---- 3. schedules ---------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", [
    pytest.param(lambda r: r.set_wavefront_streams(1), id="one-stream"),
    pytest.param(lambda r: r.set_wavefront_streams(2), id="two-streams"),
    pytest.param(lambda r: r.set_frames_per_launch(18), id="one-batch"),
    pytest.param(lambda r: (r.set_wavefront_streams(2), r.set_frames_per_launch(4)), id="two-streams-batches-of-4"),
    pytest.param(lambda r: r.set_primary_dedup(True), id="dedup-on"),
    pytest.param(lambda r: r.set_primary_dedup(False), id="dedup-off"),
    pytest.param(lambda r: (r.set_lit_table(True), r.set_skip_table(True)), id="tables-on"),
    pytest.param(lambda r: (r.set_lit_table(False), r.set_skip_table(False), r.set_occluder_table(False)), id="tables-off"),
])
def test_result_does_not_depend_on_the_schedule(setup, want):
    r = renderer()
    setup(r)
    for name in ("box4", "tent4", "tent1", "mitchell4"):
        same_bits(run(r, name), want(name), name)
    r.close()


def test_sum_continues_across_calls_and_settings(virtual, want):
    """The setting does not clear the sum: frames under one filter, then the rest under another."""
    r = renderer()
    r.set_pixel_filter(4, "tent")
    r.accum_clear()
    r.render_frames(FIRST, 7)
    r.set_pixel_filter(4, "box")
    r.render_frames(FIRST + 7, N - 7)
    got = r.accum()
    r.close()
    part = ref.accumulate(virtual.frames(4), 4, FIRST, 7, "tent")
    same_bits(got, ref.accumulate(virtual.frames(4), 4, FIRST + 7, N - 7, "box", start=part), "tent then box")


# ---- 4. Render(), bands, fp64 -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box4", "tent4"])
@pytest.mark.parametrize("ahead", [64, 1], ids=["render-ahead", "frame-by-frame"])
def test_render_loop_returns_each_frame(name, ahead, virtual):
    s, kind = FILTERS[name]
    r = renderer(batch=0)
    r.set_render_ahead(ahead)
    r.set_pixel_filter(s, kind)
    r.frame_id = FIRST - 1
    for f in range(FIRST, FIRST + N):
        got = r.Render().copy()
        assert r.frame_id == f
        same_bits(got, ref.single_frame(virtual.frames(s), s, f, kind), f"{name}: Render() of frame {f}")
    if ahead > 1:
        assert r.stats()["frames_served_ahead"] > 0
    r.close()


@pytest.mark.parametrize("name", ["box4", "tent4"])
def test_band_split_on_and_off(name, virtual):
    """One-frame calls: the box splits into row bands (17 rows >= 16), a wider filter does not, and
    either way the bits are those of the unsplit call and of the restatement."""
    s, kind = FILTERS[name]
    out = {}
    for band in (True, False):
        r = renderer()
        r.set_band_split(band)
        r.set_pixel_filter(s, kind)
        r.accum_clear()
        for f in range(FIRST, FIRST + 6):
            r.render_frames(f, 1)
        out[band] = r.accum()
        r.close()
    same_bits(out[True], out[False], f"{name}: band split on against off")
    same_bits(out[True], ref.accumulate(virtual.frames(s), s, FIRST, 6, kind), f"{name}: one-frame calls")


@pytest.mark.parametrize("name", ["box4", "tent4"])
def test_accum_fp64(name, want):
    r = renderer()
    r.set_accum_fp64(True)
    got = run(r, name)
    r.close()
    same_bits(got, want(name, fp64=True), f"{name}, fp64 sum")


# ---- 5. adaptive sampling, the debug path, a miss-only view -----------------------------------------
def test_render_adaptive_under_supersampled_box(virtual):
    from adaptive_ref import adaptive_reference

    opt = dict(threshold=0.2, min_samples=8, max_samples=24, round_frames=8, luminance_floor=0.01)
    frames = virtual.frames(2)
    want_run = adaptive_reference(lambda f: ref.subsample(frames(f), 2, f), W, H, FIRST, **opt)
    r = renderer()
    r.set_pixel_filter(2, "box")
    mean = r.render_adaptive(FIRST, **opt)
    got_sum, n = r.accum(), r.adaptive_state("samples")
    moments, tile_rounds = r.adaptive_state("moments"), r.adaptive_state("tile_rounds")
    r.close()
    print("adaptive tile rounds:", sorted(set(want_run.tile_rounds.ravel().tolist())))
    same_bits(n, want_run.n, "adaptive: counts")
    same_bits(tile_rounds, want_run.tile_rounds, "adaptive: tile rounds")
    same_bits(got_sum, want_run.sum, "adaptive: sum")
    same_bits(moments, want_run.moments, "adaptive: moments")
    same_bits(mean, want_run.mean, "adaptive: mean")


def test_debug_path_is_that_of_the_virtual_pixel():
    from oracle.oracle import OracleScene

    s = 4
    sc = tiny()
    o = OracleScene(sc)
    lp = o.launch(s * W, s * H, DEPTH, material_mode=LAMBERT, camera=camera(sc))
    r = renderer()
    r.set_pixel_filter(s, "tent")
    checked = 0
    for x, y, frame in [(9, 8, 10), (17, 16, 19), (2, 11, 4)]:
        sx, sy = ref.cell(s, frame)
        r.set_debug_pixel(x, y, frame)
        r.accum_clear()
        r.render_frames(FIRST, N)  # the debug frame is one of several in its batch
        g = _gpu_records(r)
        want_rec, _ = o.sample_path_debug(lp, s * x + sx, s * y + sy, frame)
        assert g.shape == want_rec.shape, (x, y, frame, g.shape, want_rec.shape)
        np.testing.assert_array_equal(g.view(np.uint32), want_rec.view(np.uint32))
        checked += len(want_rec)
    assert checked >= 1
    r.set_debug_pixel(-1, 0, 0)
    r.close()
    o.close()


def test_miss_only_view():
    sc = tiny()
    sc.camera_blender_pos = (-3.0, 0.0, 1.0)  # behind the back wall, looking away from the box
    r = renderer(sc)
    for name in ("box4", "mitchell4"):
        got = run(r, name)
        same_bits(got, np.zeros((H, W, 3), np.float32), f"{name}: a view of nothing")
    r.close()


# ---- 6. no trace left behind, refusals ------------------------------------------------------------------
def test_back_at_the_default_and_aovs():
    def views(r):
        r.accum_clear()
        r.render_frames(FIRST, N)
        out = {"render_frames": r.accum()}
        r.frame_id = 7
        out["Render"] = r.Render().copy()
        r.display_reset(8)
        r.display_add_frame()
        r.display_add_frame()
        out["display"] = r.display()
        return out

    fresh = renderer()
    want_views = views(fresh)
    aovs = {k: fresh.aov(k) for k in ("position", "normal", "albedo", "depth")}
    fresh.close()
    r = renderer()
    for name in ("box4", "mitchell4", "tent1"):
        s, kind = FILTERS[name]
        r.set_pixel_filter(s, kind)
        r.render_frames(FIRST, 3)
        for k, v in aovs.items():  # pixel-centre whatever the setting
            same_bits(r.aov(k), v, f"aov {k} under {name}")
    r.set_pixel_filter()
    assert r.pixel_filter() == {"supersample": 1, "kind": "box", "radius": 0.5, "param": 0.0}
    got_views = views(r)
    r.close()
    for k in want_views:
        same_bits(got_views[k], want_views[k], f"back at the default: {k}")


def test_refusals():
    from optixpathtracer_amd import capi

    r = renderer()
    r.accum_clear()
    r.render_frames(1, 2)
    before = r.accum()

    def refused(call, what):
        with pytest.raises(capi.PTError) as e:
            call()
        assert e.value.status == capi.PT_ERR_INVALID, str(e.value)
        same_bits(r.accum(), before, f"the accumulator after {what}")

    for bad in (dict(supersample=3), dict(kind=7), dict(radius=0.3), dict(radius=3.0)):
        refused(lambda: r.set_pixel_filter(**bad), f"set_pixel_filter({bad})")
    assert r.pixel_filter()["supersample"] == 1
    # the megakernel takes no filter, whichever half of it is set
    for s, kind in ((4, "box"), (1, "tent")):
        r.set_pixel_filter(s, kind)
        r.set_kernel(capi.PT_KERNEL_MEGA)
        refused(lambda: r.render_frames(3, 2), "render_frames under the megakernel")
        refused(lambda: r.Render(), "Render under the megakernel")
        r.set_kernel(capi.PT_KERNEL_AUTO)
    # adaptive rounds are not filtered
    r.set_pixel_filter(4, "tent")
    refused(lambda: r.render_adaptive(1, min_samples=8, max_samples=16, round_frames=8), "render_adaptive with a tent")
    # 8^2 * 8192 * 4096 = 2^31 pixels in the virtual image
    r.set_pixel_filter(8, "box")
    refused(lambda: r.Resize((8192, 4096)), "a resize past 2^31 virtual pixels")
    assert r.size == (W, H)
    r.set_pixel_filter()
    r.set_kernel(capi.PT_KERNEL_MEGA)
    r.render_frames(3, 1)  # the default setting leaves the megakernel alone
    r.close()


def test_multi_device_renderer_is_refused():
    from optixpathtracer_amd import capi
    from optixpathtracer_amd.renderer import setup_renderer

    multi = setup_renderer(tiny(), W, H, DEPTH, devices=[0])
    with pytest.raises(capi.PTError) as e:
        multi.set_pixel_filter(2)
    assert e.value.status == capi.PT_ERR_INVALID
    multi.set_pixel_filter()  # the default is no setting at all
    multi.close()
