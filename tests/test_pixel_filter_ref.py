"""The pixel filter's host side without a GPU: the sub-pixel cells and the tap tables of the library
(pt_pixel_filter_cells, pt_pixel_filter_taps) against the numpy restatement (pixel_filter_ref.py),
the cells' known answers and stratification, and checks that the restatement itself is not vacuous."""
import math

import numpy as np
import pytest

import pixel_filter_ref as ref

S2 = [(0, 0), (1, 1), (0, 1), (1, 0)]
S4 = [(0, 0), (2, 2), (1, 3), (3, 1), (0, 2), (2, 0), (1, 1), (3, 3), (0, 3), (2, 1), (1, 0), (3, 2), (0, 1), (2, 3),
      (1, 2), (3, 0)]
SETTINGS = [(k, 0.0, 0.0) for k in ref.KINDS] + [("box", 1.5, 0.0), ("tent", 2.5, 0.0), ("gaussian", 2.5, 1.0),
                                                 ("mitchell", 1.0, 0.75), ("tent", 0.5, 0.0)]


# ---- cells ------------------------------------------------------------------------------------
def test_known_cells():
    assert [tuple(c) for c in ref.cells(2)] == S2
    assert [tuple(c) for c in ref.cells(4)] == S4
    assert [tuple(c) for c in ref.cells(1)] == [(0, 0)]
    # the frame id itself picks the cell, as a uint32
    assert ref.cell(4, 16 + 5) == S4[5] and ref.cell(4, 2**32 - 1) == S4[15] and ref.cell(2, 2**32 + 2) == S2[2]


@pytest.mark.parametrize("s", [2, 4, 8])
def test_cells_are_a_stratified_permutation(s):
    c = ref.cells(s)
    assert sorted(map(tuple, c)) == [(x, y) for x in range(s) for y in range(s)]
    # every aligned run of 4^k cell indices puts one sample in each cell of the 2^k x 2^k coarsening
    b = s.bit_length() - 1
    for k in range(1, b + 1):
        run, shift = 4**k, b - k
        for start in range(0, s * s, run):
            coarse = {(int(x) >> shift, int(y) >> shift) for x, y in c[start:start + run]}
            assert len(coarse) == run, (s, k, start)


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_library_cells_equal_the_restatement(s, ptlib):
    from optixpathtracer_amd.renderer import pixel_filter_cells

    got = pixel_filter_cells(s)
    assert got.dtype == np.int32 and np.array_equal(got, ref.cells(s))


# ---- taps -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, radius, param", SETTINGS)
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_library_taps_within_one_rounding_of_the_restatement(s, kind, radius, param, ptlib):
    from optixpathtracer_amd.renderer import pixel_filter_taps

    r, _ = ref.resolve(kind, radius, param)
    R = math.ceil(r - 0.5)
    assert R == ref.tap_radius(kind, radius) and 0 <= R <= 2
    for c in range(s * s):
        sx, sy = ref.cell(s, c)
        gR, wx, wy = pixel_filter_taps(s, kind, radius, param, cell=c)
        assert gR == R and wx.dtype == wy.dtype == np.float32 and len(wx) == len(wy) == 2 * R + 1
        for got, coord in ((wx, sx), (wy, sy)):
            want = ref.tap_row64(s, coord, kind, radius, param)
            assert np.all(np.abs(got.astype(np.float64) - want) <= np.abs(want) * 2.0**-24), (s, kind, c, got, want)
            assert abs(float(got.astype(np.float64).sum()) - 1.0) <= (2 * R + 1) * 2.0**-24
        if R == 0:
            assert wx[0] == 1.0 and wy[0] == 1.0


def test_default_radii_and_tap_radius():
    assert [ref.tap_radius(k) for k in ref.KINDS] == [0, 1, 1, 2]
    assert ref.tap_radius("tent", 0.5) == 0 and ref.tap_radius("tent", 1.5) == 1 and ref.tap_radius("box", 2.5) == 2
    # the centre cell of an odd tap row is symmetric: s = 1 puts the sample on the pixel centre
    for k in ("tent", "gaussian", "mitchell"):
        w = ref.tap_row64(1, 0, k)
        assert np.array_equal(w, w[::-1]) and w[len(w) // 2] == w.max()


# ---- the restatement is not vacuous -----------------------------------------------------------------
def _frames(s, w, h, seed=7):
    rng = np.random.default_rng(seed)
    cache = {}

    def frame(f):
        if f not in cache:
            cache[f] = rng.random((s * h, s * w, 3), np.float32) * np.float32(3.0)
        return cache[f]

    return frame


@pytest.mark.parametrize("kind, radius, param", SETTINGS)
def test_constant_image_stays_constant(kind, radius, param):
    w, h, s = 19, 17, 4
    value = np.float32(0.7310585)
    R = ref.tap_radius(kind, radius)
    for f in range(16):
        img = np.full((s * h, s * w, 3), value, np.float32)
        g = ref.frame_image(lambda _: img, s, f, kind, radius, param)
        assert g.shape == (h, w, 3)
        ulps = np.abs(g.astype(np.float64) - float(value)) / float(np.spacing(value))
        assert ulps.max() <= (2 * R + 1) ** 2, (kind, f, ulps.max())


def test_box_without_supersampling_is_the_plain_sum():
    w, h = 19, 17
    frame = _frames(1, w, h)
    plain = np.zeros((h, w, 3), np.float32)
    for f in range(3, 21):
        plain = plain + frame(f)
    got = ref.accumulate(frame, 1, 3, 18)
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


def test_subsample_takes_the_frames_cell():
    s, w, h = 4, 5, 3
    frame = _frames(s, w, h)
    for f in (0, 5, 17):
        sx, sy = ref.cell(s, f)
        sub = ref.subsample(frame(f), s, f)
        assert sub.shape == (h, w, 3)
        for y in range(h):
            for x in range(w):
                assert np.array_equal(sub[y, x], frame(f)[s * y + sy, s * x + sx])


def test_filter_moves_what_it_should():
    """A single bright sample spreads over its (2R+1)^2 footprint with the outer product of the taps,
    clamped borders fold the outside taps onto the edge, and a NaN reaches the whole footprint."""
    w, h = 7, 6
    wx, wy = ref.taps(4, 5, "mitchell")
    img = np.zeros((h, w, 3), np.float32)
    img[2, 3] = 1.0
    g = ref.filter_frame(img, wx, wy)
    for j in range(-2, 3):
        for i in range(-2, 3):  # output (3 - i, 2 - j) reads the sample through tap (i, j)
            assert g[2 - j, 3 - i, 0] == np.float32(wy[j + 2] * wx[i + 2])
    assert not g[5].any() and not g[:, 6].any()
    corner = np.zeros((h, w, 3), np.float32)
    corner[0, 0] = 1.0
    gc = ref.filter_frame(corner, wx, wy)
    want = np.float32(0.0)
    for j in range(-2, 1):
        for i in range(-2, 1):
            want = want + np.float32(wy[j + 2] * wx[i + 2]) * np.float32(1.0)
    assert gc[0, 0, 0] == want
    nan = np.zeros((h, w, 3), np.float32)
    nan[2, 3, 1] = np.nan
    gn = ref.filter_frame(nan, wx, wy)
    assert np.isnan(gn[0:5, 1:6, 1]).all() and np.isnan(gn[..., 1]).sum() == 25 and not np.isnan(gn[..., 0]).any()
