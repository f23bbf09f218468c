"""The adaptive sampler's definitions restated in numpy (adaptive_ref.py), driven
with the CPU oracle's one-frame images.

What is checked here is the reference itself and the case the GPU test (test_gpu_adaptive.py) holds
the library to: its threshold must give a mixed schedule -- tiles that stop early, in several
different rounds, beside tiles that run to max_samples -- or a bit-exact comparison of the schedule
would pass vacuously.
"""
import math

import numpy as np
import pytest

from adaptive_ref import BASE, LAMBERT, OPTIONS, PULLED_BACK, TILE, adaptive_reference, tile_slots, tree_sum64
from helpers import oracle_render

THRESHOLD = OPTIONS["threshold"]


def oracle_frames(scene, w, h, depth, mode):
    cache = {}

    def frame(f):
        if f not in cache:
            cache[f] = oracle_render(scene, w, h, depth, f, 1, mode=mode)[0]
        return cache[f]

    return frame


@pytest.fixture(scope="module")
def base():
    from optixpathtracer_amd import scenes

    frame = oracle_frames(scenes.tiny_scene("diffuse"), BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    return adaptive_reference(frame, BASE["w"], BASE["h"], BASE["first"], **OPTIONS), frame


def per_tile(a):
    h, w = a.shape[:2]
    for ty in range((h + TILE - 1) // TILE):
        for tx in range((w + TILE - 1) // TILE):
            yield ty, tx, a[ty * TILE:ty * TILE + TILE, tx * TILE:tx * TILE + TILE]


def test_counts(base):
    ref, _ = base
    R = ref.round_frames
    assert ref.n.shape == (36, 52) and ref.tile_rounds.shape == (5, 7)
    assert (ref.n % R == 0).all()
    assert ref.n.min() >= ref.min_n and ref.n.max() <= ref.max_n
    for ty, tx, t in per_tile(ref.n):
        assert (t == t.flat[0]).all(), (ty, tx)
        assert t.flat[0] == R * ref.tile_rounds[ty, tx]
    assert ref.samples == int(ref.n.sum())
    # every round's list: the active tiles' pixels, no pixel twice, tile order
    for px in ref.round_pixels:
        assert len(set(px.tolist())) == len(px)
    assert len(ref.round_pixels[0]) == 52 * 36
    assert [len(p) for p in ref.round_pixels] == sorted((len(p) for p in ref.round_pixels), reverse=True)


def test_sums_are_the_plain_renders(base):
    """A pixel's sum is what frames first .. first + n - 1 add up to in frame order."""
    ref, frame = base
    acc = np.zeros_like(ref.sum)
    for k in range(ref.max_n):
        acc = acc + frame(BASE["first"] + k)
        done = ref.n == k + 1
        assert np.array_equal(ref.sum[done].view(np.uint32), acc[done].view(np.uint32))


def test_tree_sum_against_fsum(base):
    ref, _ = base
    from adaptive_ref import pixel_error

    e = pixel_error(ref.n, ref.moments[..., 0], ref.moments[..., 1], OPTIONS["luminance_floor"])
    assert np.array_equal(e.astype(np.float32).view(np.uint32), ref.error.view(np.uint32))
    for ty in range(5):
        for tx in range(7):
            slots, cnt = tile_slots(e, tx, ty)
            assert cnt == min(8, 52 - 8 * tx) * min(8, 36 - 8 * ty)
            tree, exact = float(tree_sum64(slots)), math.fsum(slots.tolist())
            assert abs(tree - exact) <= 1e-12 * abs(exact)
            assert np.float32(tree / cnt) == ref.tile_error[ty, tx]
    rng = np.random.default_rng(7)
    for _ in range(50):
        v = rng.uniform(0.0, 1.0, 64) * 10.0 ** rng.integers(-6, 3, 64)
        assert abs(float(tree_sum64(v)) - math.fsum(v.tolist())) <= 1e-12 * math.fsum(v.tolist())


def test_threshold_gives_a_mixed_schedule(base):
    """The condition that keeps the GPU comparison from passing vacuously."""
    ref, _ = base
    early = ref.stopped & (ref.n[::TILE, ::TILE] < ref.max_n)
    share = early.mean()
    assert 0.2 <= share <= 0.8, share
    assert len(set(ref.tile_rounds[early].tolist())) >= 3, sorted(set(ref.tile_rounds[early].tolist()))
    assert (ref.tile_error[early] <= np.float32(THRESHOLD)).all()
    assert (ref.tile_error[~ref.stopped] > np.float32(THRESHOLD)).all()
    assert (ref.n[::TILE, ::TILE][~ref.stopped] == ref.max_n).all()


def test_miss_only_tiles_stop_at_min_samples():
    from optixpathtracer_amd import scenes

    sc = scenes.tiny_scene("diffuse")
    sc.camera_blender_pos = PULLED_BACK
    frame = oracle_frames(sc, BASE["w"], BASE["h"], BASE["depth"], LAMBERT)
    ref = adaptive_reference(frame, BASE["w"], BASE["h"], BASE["first"], **{**OPTIONS, "min_samples": 16})
    black = np.ones((5, 7), bool)
    for f in range(BASE["first"], BASE["first"] + 16):
        for ty, tx, t in per_tile(frame(f)):
            black[ty, tx] &= not t.any()
    assert 5 <= black.sum() < 35  # some tiles see only misses, some see the box
    assert (ref.tile_error[black] == 0).all() and ref.stopped[black].all()
    assert (ref.tile_rounds[black] == 2).all()  # min_samples 16 = two rounds of 8
    assert (ref.n[::TILE, ::TILE][black] == 16).all()
    assert (ref.tile_rounds[~black] >= 2).all() and (ref.tile_rounds[~black] > 2).any()


def test_nan_keeps_a_tile_running():
    """A NaN sample makes the tile's error NaN, which never satisfies <=: it runs to max_samples."""
    def frame(f):
        img = np.full((8, 16, 3), 0.5, np.float32)
        if f == 3:
            img[2, 3] = np.nan
        return img

    ref = adaptive_reference(frame, 16, 8, 1, threshold=0.5, min_samples=4, max_samples=16, round_frames=4)
    assert np.isnan(ref.tile_error[0, 0]) and ref.tile_rounds[0, 0] == 4 and not ref.stopped[0, 0]
    assert ref.tile_error[0, 1] == 0 and ref.tile_rounds[0, 1] == 1 and ref.stopped[0, 1]
