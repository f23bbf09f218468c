"""Temporal reprojection and the variance-guided filter (pt_denoise_temporal): a sequence of calls
equals the numpy restatement of DESIGN.md §11 (temporal_ref.temporal_ref, guided by the CPU oracle's
first-hit records) bit for bit, output and state; the history starts and ends where it must; the
reprojection decision agrees with a float64 reading of it; and it denoises better than the spatial
filter alone."""
import functools

import numpy as np
import pytest
from denoise_ref import atrous_ref, oracle_gbuffer, oracle_gbuffer_of, same_bits, scene_by_name
from helpers import image_mse
from temporal_ref import FAULTS, camera_of, mat4_inverse, oracle_view, reprojection_f64, temporal_ref

pytestmark = pytest.mark.gpu

KINDS = ["history_length", "moments", "variance", "color"]
NAME = "textured:diffuse"
# Blender-style (position, rotation in degrees).  From inside the box and low above the floor (seen at
# a grazing angle, where the plane test depends on its normal): the back wall with its cut-outs (hits
# and misses), twice more from the same place, a pan of about a fifth of a pixel at 48 x 32, a
# pan of several pixels with two degrees of yaw, and a cut to a view that looks back past where the
# camera was: many of its points lie behind the previous camera (clip.w <= 0).
CAMERAS = [
    ((1.2, 0.0, 0.25), (90.0, 0.0, 90.0)),
    ((1.2, 0.0, 0.25), (90.0, 0.0, 90.0)),
    ((1.2, 0.0, 0.25), (90.0, 0.0, 90.0)),
    ((1.2, 0.01, 0.257), (90.0, 0.0, 90.0)),
    ((1.25, 0.16, 0.3), (90.0, 0.0, 92.0)),
    ((0.2, 0.3, 1.0), (80.0, 0.0, -30.0)),
]
SUBPIXEL_PAN, WIDE_PAN, CUT = 3, 4, 5


def _renderer(name, w, h, depth=4):
    from optixpathtracer_amd.renderer import setup_renderer

    return setup_renderer(scene_by_name(name), w, h, depth)


def _image(g, seed, specials):
    """Uniform random in [0, 2); with `specials`, one NaN and one +inf pixel, both at hits."""
    h, w = g["prim"].shape
    img = (np.random.default_rng(seed).random((h, w, 3)) * 2.0).astype(np.float32)
    hits = np.argwhere(g["prim"] >= 0)
    if specials and len(hits) >= 3:
        y, x = hits[len(hits) // 3]
        img[y, x, 1] = np.nan
        y, x = hits[2 * len(hits) // 3]
        img[y, x] = np.inf
    return img


def _images(w, h):
    """The six inputs of the sequence; the first and the fourth carry the NaN and the inf pixel."""
    return [_image(oracle_view(NAME, *CAMERAS[k], w, h)[0], 1000 * k + 10 * w + h, k in (0, 3)) for k in range(len(CAMERAS))]


@functools.lru_cache(maxsize=None)
def _reference_sequence(w, h, iterations, demodulate):
    """[(out, state)] of the six calls, computed once for both builds of the iterations."""
    seq, st = [], None
    for k, img in enumerate(_images(w, h)):
        g, cam = oracle_view(NAME, *CAMERAS[k], w, h)
        out, st = temporal_ref(st, img, g, cam, iterations=iterations, demodulate=demodulate)
        seq.append((out, st))
    return seq


def _state_equals(r, st):
    want = {"history_length": st["length"], "moments": st["moments"], "variance": st["variance"], "color": st["color"]}
    return [k for k in KINDS if not same_bits(r.temporal_state(k), want[k])]


@pytest.mark.parametrize("demodulate", [0, 1], ids=["plain", "demod"])
@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("lds", [0, 16], ids=["global", "lds16"])
@pytest.mark.parametrize("size", [(48, 32), (33, 17), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sequence_matches_restatement(size, lds, iterations, demodulate, monkeypatch):
    monkeypatch.setenv("PTAMD_DENOISE_LDS", str(lds))
    w, h = size
    seq = _reference_sequence(w, h, iterations, demodulate)
    # the sequence is what it is meant to be: first call without history, the static calls take all of it,
    # and the cut leaves points behind the old camera
    g_cut, _ = oracle_view(NAME, *CAMERAS[CUT], w, h)
    prev = seq[CUT - 1][1]
    pos = g_cut["position"].astype(np.float64)
    m = (np.linalg.inv(prev["inv_proj"].astype(np.float64).reshape(4, 4).T)
         @ np.linalg.inv(prev["inv_view"].astype(np.float64).reshape(4, 4).T))
    clip_w = np.concatenate([pos, np.ones((h, w, 1))], -1) @ m[3]
    assert ((g_cut["prim"] >= 0) & (clip_w <= 0)).any()
    assert seq[0][1]["reprojected"] == 0 and seq[2][1]["reprojected"] > 0 and seq[CUT][1]["reset"] > 0
    if size != (5, 3):  # (the inf pixel makes all of a 5 x 3 history non-finite once)
        assert seq[1][1]["reprojected"] > 0 and seq[WIDE_PAN][1]["reprojected"] > 0 and seq[WIDE_PAN][1]["reset"] > 0
    r = _renderer(NAME, w, h)
    sc = scene_by_name(NAME)
    for k, img in enumerate(_images(w, h)):
        r.SetCameraBlender(*CAMERAS[k], sc.fov_deg)
        got = r.denoise_temporal(img, iterations=iterations, demodulate=demodulate)
        out, st = seq[k]
        assert same_bits(got, out), (k, int((got.view(np.uint32) != out.view(np.uint32)).sum()))
        assert _state_equals(r, st) == [], k
        info = r.temporal_info()
        assert (info["reprojected_pixels"], info["reset_pixels"]) == (st["reprojected"], st["reset"]), k
        assert info["calls"] == k + 1 and info["history_valid"] == 1
    r.close()


def test_static_view():
    """k calls from one camera: the reprojected point is the pixel's own centre up to the rounding of
    the fp32 chain (about 20 operations on coordinates below 96: under 2e-4 of a pixel), so the pixel's
    own tap carries all but 4e-4 of the weight and every hit pixel's length is min(k, max_history), to
    4e-4 times the largest difference of lengths among neighbours (max_history); the pixel that was NaN
    in the first image starts again at the second call."""
    name, w, h, max_history = "tiny:diffuse", 96, 64, 3
    g = oracle_gbuffer(name, w, h)
    hit = g["prim"] >= 0
    r = _renderer(name, w, h)
    ny, nx = np.argwhere(hit)[len(np.argwhere(hit)) // 2]
    for k in range(1, 6):
        img = (np.random.default_rng(k).random((h, w, 3)) * 2.0).astype(np.float32)
        if k == 1:
            img[ny, nx, 0] = np.nan
        r.denoise_temporal(img, max_history=max_history)
        length = r.temporal_state("history_length")
        want = np.where(hit, np.float32(min(k, max_history)), np.float32(0))
        if k > 1:
            want[ny, nx] = min(k - 1, max_history)
        assert np.abs(length - want).max() <= 4e-4 * max_history, k
        assert (length[~hit] == 0).all()
        info = r.temporal_info()
        if k == 1:
            assert info["reprojected_pixels"] == 0 and info["reset_pixels"] == int(hit.sum())
        else:
            assert info["reset_pixels"] == (1 if k == 2 else 0), k
    assert r.denoise_info()["gbuffer_renders"] == 1
    r.close()


def test_history_boundaries():
    """A first call, temporal_reset and a resize all start every hit pixel at length 1; a pt_denoise in
    between leaves the temporal state alone and keeps its own bits; one G-buffer render per view."""
    w, h = 48, 32
    sc = scene_by_name(NAME)
    views = [oracle_view(NAME, *CAMERAS[k], w, h) for k in (0, WIDE_PAN)]
    imgs = [_image(views[0][0], 70 + k, False) for k in range(5)]
    r = _renderer(NAME, w, h)
    with pytest.raises(Exception) as e:
        r.temporal_state("variance")
    assert "pt_denoise_temporal first" in str(e.value)
    assert r.temporal_info()["history_valid"] == 0

    def call(view, img, st):
        r.SetCameraBlender(*CAMERAS[view], sc.fov_deg)
        got = r.denoise_temporal(img)
        out, st = temporal_ref(st, img, *views[0 if view == 0 else 1])
        assert same_bits(got, out) and _state_equals(r, st) == []
        return st

    def starts_again(st):
        info = r.temporal_info()
        hits = int((views[0][0]["prim"] >= 0).sum())
        assert info["reprojected_pixels"] == 0 and info["reset_pixels"] == hits
        assert (st["length"][views[0][0]["prim"] >= 0] == 1).all()

    st = call(0, imgs[0], None)
    starts_again(st)
    st = call(WIDE_PAN, imgs[1], st)
    assert r.temporal_info()["reprojected_pixels"] > 0
    before = [r.temporal_state(k) for k in KINDS]
    plain = r.denoise(imgs[2])  # the spatial filter in between, on the same scratch buffers
    assert same_bits(plain, atrous_ref(imgs[2], views[1][0]))
    assert all(same_bits(a, r.temporal_state(k)) for a, k in zip(before, KINDS))
    st = call(0, imgs[2], st)  # ... and the history it left alone is taken up
    assert r.temporal_info()["reprojected_pixels"] > 0
    assert r.denoise_info()["gbuffer_renders"] == 3  # view 0, the pan, view 0 again
    r.temporal_reset()
    assert r.temporal_info()["history_valid"] == 0
    starts_again(call(0, imgs[3], None))
    assert r.denoise_info()["gbuffer_renders"] == 3
    r.Resize((w, h))
    with pytest.raises(Exception):
        r.temporal_state("color")
    starts_again(call(0, imgs[4], None))
    r.close()


@pytest.mark.parametrize("size", [(48, 32), (33, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reprojection_agrees_with_float64_reading(size):
    """For the two pans the downloaded lengths say accept (> 1) or reset (1) at every hit pixel as the
    float64 reading does, except where that reading is within 1e-4 relative of a threshold or 1e-3 of
    a pixel boundary: at most 2 % of the hit pixels.  The restatement meets the same criterion on the
    CPU, and three seeded faults in it do not."""
    w, h = size
    sc = scene_by_name(NAME)

    def disagreements(lengths, k, prev):
        g, _ = oracle_view(NAME, *CAMERAS[k], w, h)
        accept, near = reprojection_f64(prev, g)
        hit = g["prim"] >= 0
        assert near[hit].mean() <= 0.02, (k, float(near[hit].mean()))
        return int((hit & ~near & (accept != (lengths > 1))).sum())

    states = [None]
    for k in range(WIDE_PAN + 1):  # finite inputs: history is never refused for its values
        g, cam = oracle_view(NAME, *CAMERAS[k], w, h)
        states.append(temporal_ref(states[-1], _image(g, 300 + k, False), g, cam, iterations=1)[1])
    r = _renderer(NAME, w, h)
    for k in range(WIDE_PAN + 1):
        g, cam = oracle_view(NAME, *CAMERAS[k], w, h)
        r.SetCameraBlender(*CAMERAS[k], sc.fov_deg)
        r.denoise_temporal(_image(g, 300 + k, False), iterations=1)
        if k in (SUBPIXEL_PAN, WIDE_PAN):
            assert disagreements(states[k + 1]["length"], k, states[k]) == 0  # the restatement, on the CPU
            assert disagreements(r.temporal_state("history_length"), k, states[k]) == 0
    r.close()
    for fault in FAULTS:
        wrong = 0
        for k in (SUBPIXEL_PAN, WIDE_PAN):
            g, cam = oracle_view(NAME, *CAMERAS[k], w, h)
            st = temporal_ref(states[k], _image(g, 300 + k, False), g, cam, iterations=1, fault=fault)[1]
            wrong += disagreements(st["length"], k, states[k])
        assert wrong > 0, fault


def test_follows_a_mesh_move():
    """A committed mesh move changes the guides, not the camera: the points of the moved mesh fail
    the plane test against the old guides and start again, the rest keep their history."""
    name, w, h = "tiny:diffuse", 48, 32
    r = _renderer(name, w, h)
    cam = camera_of(scene_by_name(name), w, h)
    rng = np.random.default_rng(9)
    imgs = [rng.random((h, w, 3)).astype(np.float32) for _ in range(3)]
    st = None
    for img in imgs[:2]:
        out, st = temporal_ref(st, img, oracle_gbuffer(name, w, h), cam)
        assert same_bits(r.denoise_temporal(img), out)
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = [0.2, 0.1, -0.15]
    r.set_mesh_transform(0, m.T.ravel())
    r.commit_geometry("refit")
    got = r.denoise_temporal(imgs[2])
    out, st = temporal_ref(st, imgs[2], oracle_gbuffer_of(r.model, w, h), cam)
    assert same_bits(got, out) and _state_equals(r, st) == []
    info = r.temporal_info()
    assert info["reset_pixels"] == st["reset"] > 0 and info["reprojected_pixels"] == st["reprojected"] > 0
    assert r.denoise_info()["gbuffer_renders"] == 2
    r.close()


PAN = ((0.0, 0.05, 0.0), (0.0, 0.0, 0.5))  # added to the scene camera's Blender position and rotation


def test_temporal_filter_denoises():
    """Eight calls from one camera, each on a fresh 1-spp accumulation (frame ids 1..8), against 512
    spp.  Derived on the CPU with the oracle's images and the two restatements: after the 8th call
    m(temporal) = 0.00009138 against m(pt_denoise on the 8th frame alone) = 0.00031998, ratio 0.2856;
    the cap is its square root, 0.5344 (halfway, in log scale, to no gain).  The per-call temporal MSEs
    were 0.000163, 0.000126, 0.000106, 0.0000903, 0.0000903, 0.0000879, 0.0000910, 0.0000914.  After a
    small pan on the 9th call (6125 pixels reprojected, 19 reset), against 512 spp of the new view:
    m(temporal) = 0.00010265, m(pt_denoise) = 0.00026936."""
    name, w, h = "tiny:diffuse", 96, 64
    sc = scene_by_name(name)
    r = _renderer(name, w, h, depth=4)
    r.set_material_mode(1)
    ref = r.render_accumulate(512, 1000)
    for k in range(1, 9):
        r.render_accumulate(1, k)
        temporal = r.denoise_temporal("accum")
    spatial = r.denoise("accum")
    m_t, m_s = image_mse(temporal, ref), image_mse(spatial, ref)
    pos = tuple(float(a + b) for a, b in zip(sc.camera_blender_pos, PAN[0]))
    rot = tuple(float(a + b) for a, b in zip(sc.camera_blender_rot, PAN[1]))
    r.SetCameraBlender(pos, rot, sc.fov_deg)
    ref_pan = r.render_accumulate(512, 1000)
    r.render_accumulate(1, 9)
    temporal_pan = r.denoise_temporal("accum")
    info = r.temporal_info()
    spatial_pan = r.denoise("accum")
    r.close()
    p_t, p_s = image_mse(temporal_pan, ref_pan), image_mse(spatial_pan, ref_pan)
    print(f"mse temporal={m_t:.8f} spatial={m_s:.8f} ratio={m_t / m_s:.4f}; after the pan temporal={p_t:.8f} "
          f"spatial={p_s:.8f} reprojected={info['reprojected_pixels']} reset={info['reset_pixels']}")
    assert m_t < m_s
    assert m_t / m_s <= 0.5344
    assert p_t < p_s
    # the CPU figures, digit for digit
    assert (m_t, m_s) == pytest.approx((0.00009138, 0.00031998), rel=1e-3)
    assert (p_t, p_s) == pytest.approx((0.00010265, 0.00026936), rel=1e-3)
    assert (info["reprojected_pixels"], info["reset_pixels"]) == (6125, 19)


def test_errors():
    import ctypes as C

    from optixpathtracer_amd import capi
    from optixpathtracer_amd.renderer import OptixRenderer

    name, w, h = "tiny:diffuse", 48, 32
    sc = scene_by_name(name)
    r = OptixRenderer(None, sc)
    lib = r.lib
    img = np.ones((h, w, 3), np.float32)
    out = np.empty_like(img)

    def call(source=capi.PT_DENOISE_SRC_HOST, **kw):
        t = capi.pt_temporal_options()
        t.struct_size = C.sizeof(t)
        assert lib.pt_temporal_options_default(C.byref(t)) == 0
        for k, v in kw.items():
            setattr(t, k, v)
        return lib.pt_denoise_temporal(r.h, source, capi.fptr(img), 1.0, C.byref(t), None, capi.fptr(out))

    assert call() == capi.PT_ERR_STATE and b"pt_resize" in lib.pt_last_error()
    r.Resize((w, h))
    r.SetCameraBlender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg)
    bad = [("alpha", 0.0), ("alpha", 1.5), ("alpha", float("nan")), ("alpha_moments", -0.1), ("max_history", 0),
           ("normal_cos", 1.5), ("normal_cos", -2.0), ("plane_distance", 0.0), ("sigma_luminance", -1.0),
           ("variance_history", -1)]
    for k, v in bad:
        assert call(**{k: v}) == capi.PT_ERR_INVALID, (k, v)
        assert k.split("_m")[0].encode() in lib.pt_last_error(), (k, lib.pt_last_error())
    assert call(source=3) == capi.PT_ERR_INVALID and b"source" in lib.pt_last_error()
    assert lib.pt_denoise_temporal(r.h, capi.PT_DENOISE_SRC_HOST, None, 1.0, None, None, capi.fptr(out)) == capi.PT_ERR_INVALID
    assert call(source=capi.PT_DENOISE_SRC_DISPLAY) == capi.PT_ERR_STATE and b"pt_display_reset" in lib.pt_last_error()
    with pytest.raises(capi.PTError):
        r.denoise_temporal(img, no_such_option=1)
    with pytest.raises(capi.PTError):
        r.denoise_temporal(img, iterations=9)
    assert r.temporal_info()["calls"] == 0 and r.denoise_info()["gbuffer_renders"] == 0
    # all options NULL = the defaults; alpha = 1 and variance_history = 0 are valid; the byte count is checked
    g, cam = oracle_gbuffer(name, w, h), camera_of(sc, w, h)
    assert lib.pt_denoise_temporal(r.h, capi.PT_DENOISE_SRC_HOST, capi.fptr(img), 1.0, None, None, capi.fptr(out)) == capi.PT_OK
    ref, st = temporal_ref(None, img, g, cam)
    assert same_bits(out, ref)
    got = r.denoise_temporal(img, alpha=1.0, variance_history=0, sigma_color=123.0)
    ref, st = temporal_ref(st, img, g, cam, alpha=1.0, variance_history=0)
    assert same_bits(got, ref) and _state_equals(r, st) == []
    buf = np.zeros((h, w), np.float32)
    assert lib.pt_temporal_download(r.h, capi.PT_TEMPORAL_MOMENTS, buf.ctypes.data, buf.nbytes) == capi.PT_ERR_INVALID
    assert lib.pt_temporal_download(r.h, 4, buf.ctypes.data, buf.nbytes) == capi.PT_ERR_INVALID
    r.close()
