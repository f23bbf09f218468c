"""pt_render_adaptive on the GPU against the numpy restatement (adaptive_ref.py), bit for bit.

GPU frames equal the oracle's bit for bit, a pixel's path depends only on (image pixel, frame id),
and the estimate is IEEE fp64 with a fixed summation tree: so an adaptive run can be restated
exactly from one-frame images, and everything the library shows of it -- counts, sums, moments,
errors, the schedule, the mean -- must equal the restatement's bits.  test_adaptive_ref.py checks
that the base case's threshold gives a mixed schedule, so these comparisons are not vacuous.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from adaptive_ref import BASE, DEFAULT, DIELECTRIC, LAMBERT, OPTIONS, PULLED_BACK, TILE, adaptive_reference

pytestmark = pytest.mark.gpu


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    ab, bb = a.view(np.uint8).reshape(a.shape + (-1,)), b.view(np.uint8).reshape(b.shape + (-1,))
    if not np.array_equal(ab, bb):  # the raw bits: a NaN equals itself
        bad = np.argwhere((ab != bb).any(-1))
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ, first at {first}: {a[first]!r} against {b[first]!r}")


def renderer(scene, w, h, depth, mode):
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(scene, w, h, depth)
    r.set_material_mode(mode)
    return r


def gpu_frames(scene, w, h, depth, mode):
    """frame(f): the GPU's own one-frame image, from a renderer of its own."""
    r = renderer(scene, w, h, depth, mode)
    cache = {}

    def frame(f):
        if f not in cache:
            r.accum_clear()
            r.render_frames(f, 1)
            cache[f] = r.accum()
        return cache[f]

    frame.close = r.close
    return frame


def adaptive_run(r, first, **options):
    mean = r.render_adaptive(first, **options)
    return SimpleNamespace(mean=mean, sum=r.accum(), n=r.adaptive_state("samples"), error=r.adaptive_state("error"),
                           moments=r.adaptive_state("moments"), tile_error=r.adaptive_state("tile_error"),
                           tile_rounds=r.adaptive_state("tile_rounds"), info=r.adaptive_info())


def assert_equals_reference(got, ref, what):
    same_bits(got.n, ref.n, f"{what}: counts")
    same_bits(got.tile_rounds, ref.tile_rounds, f"{what}: tile rounds")
    same_bits(got.sum, ref.sum, f"{what}: sum")
    same_bits(got.moments, ref.moments, f"{what}: moments")
    same_bits(got.error, ref.error, f"{what}: per-pixel error")
    same_bits(got.tile_error, ref.tile_error, f"{what}: tile error")
    same_bits(got.mean, ref.mean, f"{what}: mean")
    assert got.info["samples"] == ref.samples, what
    assert got.info["rounds"] == ref.rounds and got.info["tiles"] == ref.stopped.size, what
    assert got.info["tiles_stopped"] == int(ref.stopped.sum()), what
    assert got.info["samples_uniform"] == ref.n.size * int(ref.n.max()), what


def assert_same_run(a, b, what):
    for k in ("n", "tile_rounds", "sum", "moments", "error", "tile_error", "mean"):
        same_bits(getattr(a, k), getattr(b, k), f"{what}: {k}")
    assert a.info["samples"] == b.info["samples"], what


def tiny():
    from optixpathtracer_amd import scenes

    return scenes.tiny_scene("diffuse")


def base_run(mode=LAMBERT, scene=None, setup=None, **over):
    r = renderer(scene or tiny(), BASE["w"], BASE["h"], BASE["depth"], mode)
    if setup:
        setup(r)
    got = adaptive_run(r, BASE["first"], **{**OPTIONS, **over})
    r.close()
    return got


@pytest.fixture(scope="module")
def lambert_frames():
    frame = gpu_frames(tiny(), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    yield frame
    frame.close()


@pytest.fixture(scope="module")
def lambert_ref(lambert_frames):
    return adaptive_reference(lambert_frames, BASE["w"], BASE["h"], BASE["first"], **OPTIONS)


@pytest.fixture(scope="module")
def lambert_run():
    return base_run()


# ---- 1. against the reference ---------------------------------------------------------------
def test_lambert_equals_reference(lambert_run, lambert_ref):
    """The k_shade0_pixel path.  The schedule is the mixed one test_adaptive_ref.py asks for."""
    early = lambert_ref.stopped & (lambert_ref.n[::TILE, ::TILE] < lambert_ref.max_n)
    assert 0.2 <= early.mean() <= 0.8 and len(set(lambert_ref.tile_rounds[early].tolist())) >= 3
    assert_equals_reference(lambert_run, lambert_ref, "lambert")


@pytest.mark.parametrize("mode", [DIELECTRIC, DEFAULT], ids=["dielectric", "default"])
def test_other_modes_equal_reference(mode):
    """Dielectric: two streams, frame-order accumulate events.  Default: the bucketed kernels."""
    frame = gpu_frames(tiny(), BASE["w"], BASE["h"], BASE["depth"], mode)
    ref = adaptive_reference(frame, BASE["w"], BASE["h"], BASE["first"], **OPTIONS)
    frame.close()
    assert_equals_reference(base_run(mode), ref, f"mode {mode}")


def test_lambert_equals_reference_from_oracle_frames(lambert_run):
    from helpers import oracle_render

    cache = {}

    def frame(f):
        if f not in cache:
            cache[f] = oracle_render(tiny(), BASE["w"], BASE["h"], BASE["depth"], f, 1, mode=LAMBERT)[0]
        return cache[f]

    ref = adaptive_reference(frame, BASE["w"], BASE["h"], BASE["first"], **OPTIONS)
    assert_equals_reference(lambert_run, ref, "lambert, oracle frames")


# ---- 2. machinery independence -------------------------------------------------------------
@pytest.mark.parametrize("setup", [
    pytest.param(lambda r: r.set_primary_dedup(False), id="no-dedup"),
    pytest.param(lambda r: r.set_frames_per_launch(3), id="ragged-batches"),
    pytest.param(lambda r: r.set_wavefront_streams(1), id="one-stream"),
    pytest.param(lambda r: r.set_wavefront_streams(2), id="two-streams"),
    pytest.param(lambda r: (r.set_wavefront_streams(2), r.set_frames_per_launch(3)), id="two-streams-ragged"),
    pytest.param(lambda r: (r.set_lit_table(True), r.set_skip_table(True)), id="tables-on"),
    pytest.param(lambda r: (r.set_lit_table(False), r.set_skip_table(False), r.set_occluder_table(False)), id="tables-off"),
])
def test_result_does_not_depend_on_the_machinery(setup, lambert_run):
    assert_same_run(base_run(setup=setup), lambert_run, "machinery")


def test_rounds_of_two_frames(lambert_frames):
    """R = 2 is below the scene's four lights: no bounce-0 visibility table, unlike R = 8.  With
    32 samples at most the tile errors stay above 0.07, so the threshold is 0.1 here: the CPU
    reference then stops 31 of the 35 tiles, in rounds 8 to 16."""
    opt = {**OPTIONS, "round_frames": 2, "max_samples": 32, "threshold": 0.1}
    ref = adaptive_reference(lambert_frames, BASE["w"], BASE["h"], BASE["first"], **opt)
    assert len(set(ref.tile_rounds.ravel().tolist())) >= 3
    assert_equals_reference(base_run(**{"round_frames": 2, "max_samples": 32, "threshold": 0.1}), ref, "R = 2")


def test_textured_scene():
    from optixpathtracer_amd import scenes

    sc, w, h, depth = scenes.textured_scene("diffuse"), 40, 28, 4
    opt = {**OPTIONS, "max_samples": 32}
    frame = gpu_frames(sc, w, h, depth, sc.material_mode)
    ref = adaptive_reference(frame, w, h, 1, **opt)
    frame.close()
    r = renderer(sc, w, h, depth, sc.material_mode)
    got = adaptive_run(r, 1, **opt)
    r.close()
    assert_equals_reference(got, ref, "textured")


# ---- 3. degenerate thresholds ----------------------------------------------------------------
@pytest.mark.parametrize("threshold, which", [(0.0, "max_samples"), (float("inf"), "min_samples")])
def test_degenerate_thresholds(threshold, which):
    opt = {**OPTIONS, "threshold": threshold, "min_samples": 16, "max_samples": 24}
    r = renderer(tiny(), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    got = adaptive_run(r, 5, **opt)
    r.accum_clear()
    r.render_frames(5, opt[which])
    plain = r.accum()
    r.close()
    assert (got.n == opt[which]).all()
    same_bits(got.sum, plain, f"threshold {threshold}: sum")
    same_bits(got.mean, plain / np.float32(opt[which]), f"threshold {threshold}: mean")


# ---- 4. edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 1])
@pytest.mark.parametrize("size", [8, 9])
def test_small_images(size, bounces):
    """8x8: one full tile.  9x9: four tiles, three of them partial (8x1, 1x8, 1x1)."""
    opt = {**OPTIONS, "max_samples": 32, "threshold": 0.12}
    frame = gpu_frames(tiny(), size, size, bounces, LAMBERT)
    ref = adaptive_reference(frame, size, size, 1, **opt)
    frame.close()
    r = renderer(tiny(), size, size, bounces, LAMBERT)
    got = adaptive_run(r, 1, **opt)
    r.close()
    assert got.tile_rounds.shape == ((1, 1) if size == 8 else (2, 2))
    if bounces == 0:  # black frames: no variance, every tile stops at min_samples
        assert (got.n == ref.min_n).all() and not got.sum.any()
    assert_equals_reference(got, ref, f"{size}x{size}, {bounces} bounces")


def test_miss_only_view_stops_at_min_samples():
    sc = tiny()
    sc.camera_blender_pos = (-3.0, 0.0, 1.0)  # behind the back wall, looking away from the box
    got = base_run(scene=sc, min_samples=16)
    assert (got.n == 16).all() and (got.tile_rounds == 2).all()
    assert not got.sum.any() and not got.error.any() and not got.tile_error.any()
    assert got.info["tiles_stopped"] == got.info["tiles"] == 35


def test_pulled_back_view_equals_reference():
    """Tiles that see only misses stop at min_samples beside tiles that go on."""
    sc = tiny()
    sc.camera_blender_pos = PULLED_BACK
    opt = {**OPTIONS, "min_samples": 16}
    frame = gpu_frames(sc, BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    ref = adaptive_reference(frame, BASE["w"], BASE["h"], BASE["first"], **opt)
    frame.close()
    assert (ref.tile_rounds == 2).sum() >= 5 and (ref.tile_rounds > 2).any()
    assert_equals_reference(base_run(scene=sc, min_samples=16), ref, "pulled back")


# ---- 5. no trace left behind ------------------------------------------------------------------
def test_leaves_no_trace():
    def views(r):
        r.accum_clear()
        r.render_frames(3, 5)
        out = {"render_frames": r.accum()}
        r.frame_id = 7
        out["Render"] = r.Render().copy()
        r.display_reset(8)
        r.display_add_frame()
        r.display_add_frame()
        out["display"] = r.display()
        out["aov"] = r.aov("position")
        return out

    r = renderer(tiny(), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    r.render_adaptive(BASE["first"], **OPTIONS)
    after = views(r)
    from optixpathtracer_amd import capi

    with pytest.raises(capi.PTError) as e:  # pt_accum_clear dropped the adaptive state
        r.adaptive_state("samples")
    assert e.value.status == capi.PT_ERR_STATE
    r.close()
    fresh = renderer(tiny(), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    want = views(fresh)
    fresh.close()
    for k in want:
        same_bits(after[k], want[k], f"after an adaptive call: {k}")


# ---- 6. stats, the denoise source, refusals ---------------------------------------------------
def test_stats_count_the_samples_rendered():
    r = renderer(tiny(), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    before = r.stats()
    got = adaptive_run(r, BASE["first"], **OPTIONS)
    after = r.stats()
    r.close()
    assert after["samples"] - before["samples"] == int(got.n.sum(dtype=np.uint64)) == got.info["samples"]
    assert after["segments"] > before["segments"] and after["render_calls"] - before["render_calls"] == got.info["rounds"]
    assert got.info["samples"] < got.info["samples_uniform"]
    assert got.info["render_ms"] > 0 and got.info["estimate_ms"] > 0


def test_denoise_source_adaptive():
    from optixpathtracer_amd import capi

    r = renderer(tiny(), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    with pytest.raises(capi.PTError) as e:  # no adaptive render yet
        r.denoise(source="adaptive")
    assert e.value.status == capi.PT_ERR_STATE
    mean = r.render_adaptive(BASE["first"], **OPTIONS)
    a = r.denoise(source="adaptive")
    b = r.denoise(source=mean)
    a2 = r.denoise(source="adaptive", scale=0.5)
    b2 = r.denoise(source=mean, scale=0.5)
    t = r.denoise_temporal(source="adaptive")
    r.temporal_reset()
    t2 = r.denoise_temporal(source=mean)
    r.close()
    same_bits(a, b, "denoise(adaptive) against denoise(mean)")
    same_bits(a2, b2, "denoise(adaptive, scale) against denoise(mean, scale)")
    same_bits(t, t2, "denoise_temporal(adaptive) against denoise_temporal(mean)")


def test_refusals_leave_the_accumulator():
    from optixpathtracer_amd import capi
    from optixpathtracer_amd.renderer import OptixRenderer

    r = renderer(tiny(), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    r.accum_clear()
    r.render_frames(1, 2)
    before = r.accum()

    def refused(status, **options):
        with pytest.raises(capi.PTError) as e:
            r.render_adaptive(BASE["first"], **{**OPTIONS, **options})
        assert e.value.status == status, str(e.value)
        same_bits(r.accum(), before, "the accumulator after a refused call")

    r.set_kernel(capi.PT_KERNEL_MEGA)
    refused(capi.PT_ERR_INVALID)
    r.set_kernel(capi.PT_KERNEL_AUTO)
    r.set_debug_pixel(3, 4, 1)
    refused(capi.PT_ERR_INVALID)
    r.set_debug_pixel(-1, -1, 0)
    r.set_accum_device_buffer(r.lib.pt_accum_device_ptr(r.h))
    refused(capi.PT_ERR_INVALID)
    r.set_accum_device_buffer(None)
    for bad in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(round_frames=1), dict(min_samples=0),
                dict(max_samples=4), dict(luminance_floor=0.0)):
        refused(capi.PT_ERR_INVALID, **bad)
    r.set_accum_fp64(True)
    with pytest.raises(capi.PTError) as e:
        r.render_adaptive(BASE["first"], **OPTIONS)
    assert e.value.status == capi.PT_ERR_INVALID
    r.set_accum_fp64(False)
    same_bits(r.accum(), before, "the accumulator after the fp64 refusal")
    r.close()

    unsized = OptixRenderer(None, tiny())  # no Resize yet
    with pytest.raises(capi.PTError) as e:
        unsized.render_adaptive(BASE["first"], **OPTIONS)
    assert e.value.status == capi.PT_ERR_STATE
    unsized.close()


def test_multi_device_renderer_is_refused():
    from optixpathtracer_amd import capi
    from optixpathtracer_amd.renderer import setup_renderer

    multi = setup_renderer(tiny(), BASE["w"], BASE["h"], BASE["depth"], devices=[0])
    multi.accum_clear()
    multi.render_frames(1, 2)
    before = multi.accum()
    with pytest.raises(capi.PTError) as e:
        multi.render_adaptive(BASE["first"], **OPTIONS)
    assert e.value.status == capi.PT_ERR_INVALID
    same_bits(multi.accum(), before, "the accumulator after a refused call")
    multi.close()
