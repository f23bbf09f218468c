"""The a-trous denoiser (pt_denoise): the filter equals its numpy restatement (denoise_ref.atrous_ref,
guided by the CPU oracle's first-hit records, not by the GPU's) bit for bit, from all three sources;
it keeps what it must keep; and it denoises."""
import numpy as np
import pytest
from denoise_ref import atrous_ref, oracle_gbuffer, oracle_gbuffer_of, same_bits, scene_by_name
from helpers import image_mse

pytestmark = pytest.mark.gpu

OPTIONS = [
    {},  # 5 iterations at the defaults
    {"iterations": 1},
    {"iterations": 8},
    {"demodulate": 0},
]


def _renderer(name, w, h, depth=4):
    from optixpathtracer_amd.renderer import setup_renderer

    return setup_renderer(scene_by_name(name), w, h, depth)


def _noise_with_specials(g, seed):
    """Uniform random in [0, 2) plus one +inf, one NaN and one 1e30 pixel, all three at hits.  The inf
    pixel turns every pixel that taps it into NaN (inf * 0 in the specification), at offsets of 0, 1,
    2, 4, ... pixels per axis; the NaN pixel sits 11 columns away, so none of its neighbours does."""
    h, w = g["prim"].shape
    rng = np.random.default_rng(seed)
    img = (rng.random((h, w, 3)) * 2.0).astype(np.float32)
    hit = g["prim"] >= 0
    spots = [(y, x) for y in range(1, h - 1) for x in range(1, w - 12) if hit[y, x] and hit[y, x + 11] and hit[y + 1, x + 5]]
    if not spots:  # an image too small for all three: the NaN pixel alone
        y, x = np.argwhere(hit)[0]
        img[y, x, 1] = np.nan
        return img, None
    y, x = spots[len(spots) // 2]
    img[y, x] = np.inf
    img[y, x + 11, 1] = np.nan
    img[y + 1, x + 5] = np.float32(1e30)
    return img, (y, x + 11)


@pytest.mark.parametrize("lds", [0, 2, 4, 16], ids=["plain", "lds2", "lds4", "lds16"])
@pytest.mark.parametrize("size", [(48, 32), (33, 17), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_matches_restatement(size, lds, monkeypatch):
    """Host source on the textured scene (hits and misses).  33x17 and 5x3: ragged tiles, and steps
    wider than the image.  Every build of the small-step iterations gives the same bits: all taps
    from global memory, or the steps up to 2, 4 or 16 staged in LDS (PTAMD_DENOISE_LDS)."""
    monkeypatch.setenv("PTAMD_DENOISE_LDS", str(lds))
    w, h = size
    g = oracle_gbuffer("textured:diffuse", w, h)
    assert (g["prim"] >= 0).any()
    img, nan_at = _noise_with_specials(g, seed=w * 100 + h)
    if size == (48, 32):
        assert nan_at is not None and (g["prim"] < 0).any()
    r = _renderer("textured:diffuse", w, h)
    for opt in OPTIONS:
        got = r.denoise(img, **opt)
        ref = atrous_ref(img, g, **opt)
        assert same_bits(got, ref), (opt, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
        assert r.denoise_info()["iterations"] == opt.get("iterations", 5)
        if nan_at is not None:
            y, x = nan_at
            assert np.isnan(got[y, x, 1])  # a NaN pixel stays NaN ...
            around = got[y - 1:y + 2, x - 1:x + 2].copy()
            around[1, 1] = 0.0
            assert np.isfinite(around).all(), opt  # ... and keeps to itself
    assert r.denoise_info()["gbuffer_renders"] == 1
    r.close()


def test_three_sources_agree():
    name, w, h = "tiny:diffuse", 96, 64
    g = oracle_gbuffer(name, w, h)
    r = _renderer(name, w, h, depth=4)
    r.set_material_mode(1)
    r.accum_clear()
    r.render_frames(1, 4)
    acc = r.accum(0.25)
    got = r.denoise("accum", scale=0.25)
    assert same_bits(got, atrous_ref(acc, g))
    # the device result is what the call returned (read back through the accumulator's download)
    ptr = r.lib.pt_denoised_device_ptr(r.h)
    assert ptr
    r.set_accum_device_buffer(ptr)
    dev = r.accum()
    r.set_accum_device_buffer(None)
    assert same_bits(dev, got)

    r.display_reset(-1)
    for _ in range(4):
        r.display_add_frame()
    shown = r.display()
    assert same_bits(r.denoise("display"), atrous_ref(shown, g))
    # a host copy of the same image gives the same result
    assert same_bits(r.denoise(shown), atrous_ref(shown, g))
    assert r.denoise_info()["gbuffer_renders"] == 1
    r.close()


def test_invariants():
    """Without demodulation the weights sum to wsum exactly, so a constant image is a fixed point bit
    for bit.  With it the colour filtered is image / albedo, which is constant only where the image is
    the (floored) albedo itself: that image comes back unchanged, and zeros stay zeros.  Miss pixels
    come back as they went in, whatever they hold."""
    w, h = 48, 32
    g = oracle_gbuffer("textured:diffuse", w, h)
    miss = g["prim"] < 0
    assert miss.any() and (~miss).any()
    r = _renderer("textured:diffuse", w, h)
    ones, zeros = np.ones((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    for demod in (0, 1):
        assert not r.denoise(zeros, demodulate=demod).view(np.uint32).any()
    assert same_bits(r.denoise(ones, demodulate=0), ones)
    floored = np.maximum(g["albedo"], np.float32(1e-3))
    floored[miss] = 1.0
    assert same_bits(r.denoise(floored), floored)
    rng = np.random.default_rng(5)
    img = (rng.random((h, w, 3)) * 2.0).astype(np.float32)
    img[np.argwhere(miss)[0][0], np.argwhere(miss)[0][1]] = [np.nan, np.inf, -3.0]
    for opt in OPTIONS:
        out = r.denoise(img, **opt)
        assert same_bits(out[miss], img[miss]), opt
        assert (out[~miss].view(np.uint32) != img[~miss].view(np.uint32)).any()
    r.close()


def test_filter_denoises():
    """1 spp against 512 spp, both rendered here.  Derived on the CPU with the oracle and the
    restatement, which the GPU equals bit for bit: m(noisy) = 0.003682, m(denoised) = 0.000287 (ratio
    0.078; the cap leaves a factor of 3), m(plain B3 blur) = 0.000549 (ratio 0.52)."""
    name, w, h = "tiny:diffuse", 96, 64
    r = _renderer(name, w, h, depth=4)
    r.set_material_mode(1)
    ref = r.render_accumulate(512, 1000)
    noisy = r.render_accumulate(1, 1)
    den = r.denoise("accum", scale=1.0)
    blur = r.denoise("accum", scale=1.0, sigma_color=1e9, sigma_normal=1e9, sigma_position=1e9)
    r.close()
    m_noisy, m_den, m_blur = image_mse(noisy, ref), image_mse(den, ref), image_mse(blur, ref)
    print(f"mse noisy={m_noisy:.6f} denoised={m_den:.6f} blur={m_blur:.6f}")
    assert m_den <= 0.25 * m_noisy
    assert m_den <= 0.75 * m_blur  # the edge-stopping terms act


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
        o = capi.pt_denoise_options()
        o.struct_size = C.sizeof(o)
        assert lib.pt_denoise_options_default(C.byref(o)) == 0
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.pt_denoise(r.h, source, capi.fptr(img), 1.0, C.byref(o), capi.fptr(out))

    assert call() == capi.PT_ERR_STATE and b"pt_resize" in lib.pt_last_error()  # before the first pt_resize
    r.Resize((w, h))
    r.SetCameraBlender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg)
    for bad in ({"iterations": 0}, {"iterations": 9}):
        assert call(**bad) == capi.PT_ERR_INVALID and b"iterations" in lib.pt_last_error()
    for bad in ({"sigma_color": -1.0}, {"sigma_normal": 0.0}, {"sigma_position": float("nan")}):
        assert call(**bad) == capi.PT_ERR_INVALID and b"sigma" in lib.pt_last_error(), bad
    assert call(albedo_floor=0.0) == capi.PT_ERR_INVALID and b"albedo_floor" in lib.pt_last_error()
    assert call(source=3) == capi.PT_ERR_INVALID and b"source" in lib.pt_last_error()
    assert lib.pt_denoise(r.h, capi.PT_DENOISE_SRC_HOST, None, 1.0, None, capi.fptr(out)) == capi.PT_ERR_INVALID
    assert call(source=capi.PT_DENOISE_SRC_DISPLAY) == capi.PT_ERR_STATE and b"pt_display_reset" in lib.pt_last_error()
    buf = np.zeros((h, w, 3), np.float32)
    assert lib.pt_aov_download(r.h, capi.PT_AOV_NORMAL, buf.ctypes.data, buf.nbytes + 12) == capi.PT_ERR_INVALID  # byte count
    with pytest.raises(capi.PTError):
        r.denoise(img[:-1])
    with pytest.raises(capi.PTError):
        r.denoise("nowhere")
    assert r.denoise_info()["gbuffer_renders"] == 0  # nothing above got as far as the G-buffer
    # a valid call afterwards still works, options NULL = the defaults
    assert lib.pt_denoise(r.h, capi.PT_DENOISE_SRC_HOST, capi.fptr(img), 1.0, None, capi.fptr(out)) == capi.PT_OK
    assert same_bits(out, atrous_ref(img, oracle_gbuffer(name, w, h)))
    # a caller compiled against a shorter options struct: the cut-off fields take their defaults
    short = capi.pt_denoise_options(capi.pt_denoise_options.sigma_color.offset, 2, 0, -5.0, -5.0, -5.0, -5.0)
    assert lib.pt_denoise(r.h, capi.PT_DENOISE_SRC_HOST, capi.fptr(img), 1.0, C.byref(short), capi.fptr(out)) == capi.PT_OK
    assert same_bits(out, atrous_ref(img, oracle_gbuffer(name, w, h), iterations=2, demodulate=0))
    r.close()


def test_denoise_follows_a_mesh_move():
    """The filter's guides follow a geometry commit: after it the result equals the restatement
    guided by the oracle's records of the moved scene."""
    name, w, h = "tiny:diffuse", 48, 32
    r = _renderer(name, w, h)
    rng = np.random.default_rng(9)
    img = rng.random((h, w, 3)).astype(np.float32)
    assert same_bits(r.denoise(img), atrous_ref(img, oracle_gbuffer(name, w, h)))
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = [0.2, 0.1, -0.15]
    r.set_mesh_transform(0, m.T.ravel())
    r.commit_geometry("refit")
    got = r.denoise(img)
    assert r.denoise_info()["gbuffer_renders"] == 2
    assert same_bits(got, atrous_ref(img, oracle_gbuffer_of(r.model, w, h)))
    r.close()
