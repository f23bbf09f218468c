"""The CPU oracle against the reference's OWN BSDF, RNG and camera code, bit for bit.  CPU only.

Every GPU result is judged against oracle/pt_oracle.c, a restatement by hand of the reference's
device code.  This module pins that restatement to the code it restates: oracle/Makefile
host-compiles the reference's PBRT/*.h, random.h and Camera.cpp behind our C wrapper
(oracle/ptref_capi.cpp) into oracle/_ref/, and the oracle has to give the same BITS.

Two tiers over one seeded input set (`build_cases`):

* live   - needs oracle/_ref/libptref_om.so (the reference's headers with the oracle's sin/cos/exp
           polynomials behind sinf/cosf/expf, so that everything around the transcendentals is
           compared exactly).  Skips where the reference tree was not there to build from.
* golden - tests/golden/reference_bsdf.npz, the outputs of that library for a deterministic
           subset of the same inputs (tests/golden/make_reference_golden.py).  Never skips.

No case is filtered out after generation.  The one exclusion is by construction, the Layered
seed-cast rule: GlossyDiffuse.h:215-217 (f) and :417 (Sample_f) seed a private RNG with
`tea<16>(wo.x * 1000, wo.y * 1000)` (and wi likewise in f), a float -> unsigned conversion that
saturates negatives to 0 in PTX (restated and tested as orc_f2u_sat) but is undefined on the
host.  After the two-sided flip (:162-165, :389-392) the casts are in range exactly when the x
and y of wo (and of wi, for f) carry the sign of wo.z or are zero, so every Layered direction is
built that way (`_fold`).  The negative-seed cast itself stays pinned by PTX only.
"""
from __future__ import annotations

import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
REF_DIR = ROOT / "oracle" / "_ref"
REF_OM = REF_DIR / "libptref_om.so"   # oracle polynomials behind sinf / cosf / expf
REF_LIBM = REF_DIR / "libptref.so"    # libm's
GOLDEN = ROOT / "tests" / "golden" / "reference_bsdf.npz"

MODELS = ["lambert", "conductor", "dielectric", "layered"]
# 0.0316^2 < 1e-3 <= 0.0317^2: the pair straddles Surface::IsEffectifvelySmooth (Surface.h:22-24)
ROUGHNESS = [0.0, 0.02, 0.0316, 0.0317, 0.05, 0.3, 0.7, 1.0]
TWO_SIDED = ("dielectric", "layered")  # Lambert and Conductor are used with wo above the surface
N_RANDOM = 256
GOLDEN_STRIDE = 8  # the golden file keeps every edge case and every 8th random case
N_WI = 6           # sampled direction, random above, random below, mirror, -wo, zero half-vector xy

_FP = C.POINTER(C.c_float)
_UP = C.POINTER(C.c_uint32)
_IP = C.POINTER(C.c_int32)


# ----------------------------------------------------------------------------------------------
# the two sides behind one interface
# ----------------------------------------------------------------------------------------------
class _Side:
    """sample / eval / pdf over arrays of independent cases, through the batched C entry points."""

    def __init__(self, lib, names):
        self.lib = lib
        self._sample, self._eval, self._pdf = (getattr(lib, n) for n in names)
        self._sample.restype = self._eval.restype = self._pdf.restype = None
        self._sample.argtypes = [C.c_int32, C.c_int32, _UP, _FP, _FP, _FP, _FP, _IP]
        self._eval.argtypes = [C.c_int32, C.c_int32, _UP, _FP, _FP, _FP, _FP, _FP]
        self._pdf.argtypes = [C.c_int32, C.c_int32, _FP, _FP, _FP, _FP]

    def sample(self, model, seeds, albedo, rough, wo):
        n = len(seeds)
        s = np.array(seeds, dtype=np.uint32)
        out = np.zeros((n, 8), np.float32)
        ok = np.zeros(n, np.int32)
        self._sample(O.BSDF[model], n, s.ctypes.data_as(_UP), O.fp(albedo), O.fp(rough), O.fp(wo), O.fp(out),
                     ok.ctypes.data_as(_IP))
        return ok, out.view(np.uint32), s

    def eval(self, model, seeds, albedo, rough, wo, wi):
        n = len(seeds)
        s = np.array(seeds, dtype=np.uint32)
        out = np.zeros((n, 3), np.float32)
        self._eval(O.BSDF[model], n, s.ctypes.data_as(_UP), O.fp(albedo), O.fp(rough), O.fp(wo), O.fp(wi), O.fp(out))
        return out.view(np.uint32), s

    def pdf(self, model, rough, wo, wi):
        n = len(rough)
        out = np.zeros(n, np.float32)
        self._pdf(O.BSDF[model], n, O.fp(rough), O.fp(wo), O.fp(wi), O.fp(out))
        return out.view(np.uint32)


def oracle_side() -> _Side:
    return _Side(O.load(), ("orc_bsdf_sample_cases", "orc_bsdf_eval_cases", "orc_bsdf_pdf_cases"))


def load_reference(path: Path) -> C.CDLL:
    """ctypes' default mode is RTLD_LOCAL: nothing the library defines reaches numpy or the oracle."""
    O.load()
    lib = C.CDLL(str(path))
    lib.ref_tea16.restype = C.c_uint32
    lib.ref_tea16.argtypes = [C.c_uint32, C.c_uint32]
    lib.ref_rnd_seq.restype = None
    lib.ref_rnd_seq.argtypes = [C.c_uint32, C.c_int32, _FP, _UP]
    lib.ref_disk_concentric.restype = None
    lib.ref_disk_concentric.argtypes = [_UP, _FP]
    lib.ref_camera_from_blender.restype = None
    lib.ref_camera_from_blender.argtypes = [_FP, _FP, C.c_float, C.c_int32, C.c_int32, _FP, _FP, _FP]
    return lib


def reference_side(lib: C.CDLL) -> _Side:
    return _Side(lib, ("ref_bsdf_sample_n", "ref_bsdf_eval_n", "ref_bsdf_pdf_n"))


# ----------------------------------------------------------------------------------------------
# the input set
# ----------------------------------------------------------------------------------------------
def _fold(v: np.ndarray, s: np.ndarray) -> np.ndarray:
    """The Layered seed-cast rule: x and y take the sign of wo.z (zeros, -0.0 too, stay)."""
    v = v.copy()
    for a in (0, 1):
        nz = v[:, a] != 0.0
        v[nz, a] = (s * np.abs(v[:, a]))[nz]
    return v


def _sphere(rng, n, z):
    phi = rng.uniform(0.0, 2.0 * math.pi, n)
    st = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([st * np.cos(phi), st * np.sin(phi), z], axis=1).astype(np.float32)


def build_cases(model: str, ri: int) -> dict:
    """Inputs of one (model, roughness): N_RANDOM random cases, then the edges.  Deterministic."""
    rng = np.random.default_rng([20241021, MODELS.index(model), ri])
    two = model in TWO_SIDED
    n = N_RANDOM
    # |z| from 1e-3 to 1: half of the cases log-uniform (grazing), half uniform
    z = np.where(np.arange(n) % 2 == 0, 10.0 ** rng.uniform(-3.0, 0.0, n), rng.uniform(1e-3, 1.0, n))
    if two:
        z = z * rng.choice([-1.0, 1.0], n)
    wo = _sphere(rng, n, z)
    albedo = rng.uniform(0.05, 1.0, (n, 3)).astype(np.float32)

    edges = [(0.0, 0.0, 1.0), (math.sqrt(1.0 - 1e-12), 0.0, 1e-6), (-0.0, -0.0, 1.0)]
    if two:
        edges += [(x, y, -zz) for x, y, zz in edges]
    e_wo, e_al = [], []
    for e in edges:
        for al in (tuple(rng.uniform(0.05, 1.0, 3)), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
            e_wo.append(e)
            e_al.append(al)
    for al in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):  # the two albedo edges at a random direction as well
        e_wo.append(tuple(_sphere(rng, 1, np.array([-0.6 if two and al[0] == 0.0 else 0.6]))[0]))
        e_al.append(al)
    wo = np.concatenate([wo, np.array(e_wo, np.float32)])
    albedo = np.concatenate([albedo, np.array(e_al, np.float32)])
    m = len(wo)
    s = np.where(np.signbit(wo[:, 2]), np.float32(-1.0), np.float32(1.0))
    if model == "layered":
        wo = _fold(wo, s)

    # wi for f and pdf; slot 0 is the reference's own sampled direction, filled in by `with_sampled`
    wi = np.zeros((m, N_WI, 3), np.float32)
    wi[:, 1] = _sphere(rng, m, rng.uniform(1e-3, 1.0, m))
    wi[:, 2] = _sphere(rng, m, -rng.uniform(1e-3, 1.0, m))
    wi[:, 3] = wo * np.float32([-1, -1, 1])      # mirror direction
    wi[:, 4] = -wo                               # wo + wi == 0
    wi[:, 5] = wo * np.float32([-1, -1, 0.5])    # wo + wi exactly zero in x and y, z not
    return {
        "model": model, "n_random": n, "wo": np.ascontiguousarray(wo), "albedo": np.ascontiguousarray(albedo),
        "rough": np.full(m, ROUGHNESS[ri], np.float32), "sign": s,
        "seed": rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32),
        "eval_seed": rng.integers(0, 2 ** 32, (m, N_WI), dtype=np.uint64).astype(np.uint32),
        "wi": wi,
    }


def with_sampled(c: dict, sample_out_bits: np.ndarray) -> dict:
    """Fill wi slot 0 with the reference's sampled direction.  For Layered every wi is then folded
    into the cast rule: z, and so the lobe, stays; the mirror direction, -wo and the zero-xy half
    vector keep their exact form only where wo.x = wo.y = 0 (the (0, 0, +-1) and -0.0 edges)."""
    c = dict(c)
    wi = c["wi"].copy()
    wi[:, 0] = sample_out_bits.view(np.float32)[:, 4:7]
    if c["model"] == "layered":
        for k in range(N_WI):
            wi[:, k] = _fold(wi[:, k], c["sign"])
    c["wi"] = wi
    return c


def subset(c: dict, idx: np.ndarray) -> dict:
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def golden_index(c: dict) -> np.ndarray:
    m = len(c["wo"])
    return np.concatenate([np.arange(0, c["n_random"], GOLDEN_STRIDE), np.arange(c["n_random"], m)])


def run_sample(side: _Side, c: dict):
    return side.sample(c["model"], c["seed"], c["albedo"], c["rough"], c["wo"])


def run_eval_pdf(side: _Side, c: dict):
    """f (with the seed after it) and pdf at every wi of every case: (m, N_WI, 3), (m, N_WI), (m, N_WI)."""
    m = len(c["wo"])
    rep = lambda a: np.ascontiguousarray(np.repeat(a, N_WI, axis=0))  # noqa: E731
    wi = np.ascontiguousarray(c["wi"].reshape(m * N_WI, 3))
    f, s = side.eval(c["model"], c["eval_seed"].reshape(-1), rep(c["albedo"]), rep(c["rough"]), rep(c["wo"]), wi)
    p = side.pdf(c["model"], rep(c["rough"]), rep(c["wo"]), wi)
    return f.reshape(m, N_WI, 3), s.reshape(m, N_WI), p.reshape(m, N_WI)


PAIRS = [(m, ri) for m in MODELS for ri in range(len(ROUGHNESS))]
PAIR_IDS = [f"{m}-r{ROUGHNESS[ri]}" for m, ri in PAIRS]


def _first_diff(name, a, b, c):
    """Message for the first case whose bits differ."""
    bad = np.argwhere(np.atleast_1d(a != b))
    k = int(bad[0][0])
    return (f"{name}: {len(np.unique(bad[:, 0]))} of {len(a)} cases differ; first case {k}: wo={c['wo'][k].tolist()} "
            f"albedo={c['albedo'][k].tolist()} seed={int(c['seed'][k])} oracle={np.atleast_1d(a[k]).tolist()} "
            f"reference={np.atleast_1d(b[k]).tolist()}")


def assert_same_bits(name, got, want, c):
    assert got.shape == want.shape
    assert np.array_equal(got, want), _first_diff(name, got, want, c)


def check_pair(orc: _Side, c: dict, ref_sample, ref_eval_pdf):
    """The oracle reproduces the reference's bits: return value, the eight floats, seed, f, pdf."""
    r_ok, r_out, r_seed = ref_sample
    c = with_sampled(c, r_out)
    ok, out, seed = run_sample(orc, c)
    assert_same_bits("Sample_f return value", ok, r_ok.astype(np.int32), c)
    assert_same_bits("Sample_f colour/pdf/direction/flags", out, r_out, c)
    assert_same_bits("seed after Sample_f", seed, r_seed, c)
    f, fs, p = run_eval_pdf(orc, c)
    r_f, r_fs, r_p = ref_eval_pdf
    assert_same_bits("f", f, r_f, c)
    assert_same_bits("seed after f", fs, r_fs, c)
    assert_same_bits("pdf", p, r_p, c)


# ----------------------------------------------------------------------------------------------
# live tier
# ----------------------------------------------------------------------------------------------
def _lcg_draws(seed, n):
    out = []
    for _ in range(n):
        seed = (1664525 * seed + 1013904223) & 0xFFFFFFFF
        out.append((seed & 0x00FFFFFF) / float(0x01000000))
    return out


def check_draw_order(lib):
    """Build self-check.  SampleUniformDiskConcentric (LambertDiffuse.h:35-55) takes its two draws
    inside one constructor call; the reference's PTX draws x first.  A library built by a compiler
    that evaluates arguments right to left returns the point mirrored in the diagonal, and every
    comparison in this module would be against the wrong sequence.  Tolerance 1e-6: a handful of
    float32 roundings (2^-24 each) on values of at most 1."""
    for seed in (1, 12345, 2730713777, 0xDEADBEEF):
        u0, u1 = _lcg_draws(seed, 2)
        ox, oy = 2.0 * u0 - 1.0, 2.0 * u1 - 1.0
        if abs(ox) > abs(oy):
            r, th = ox, math.pi / 4 * (oy / ox)
        else:
            r, th = oy, math.pi / 2 - math.pi / 4 * (ox / oy)
        want = (r * math.cos(th), r * math.sin(th))
        assert abs(want[0] - want[1]) > 1e-3  # the mirrored answer is told apart
        s = C.c_uint32(seed)
        got = np.zeros(2, np.float32)
        lib.ref_disk_concentric(C.byref(s), O.fp(got))
        assert abs(got[0] - want[0]) < 1e-6 and abs(got[1] - want[1]) < 1e-6, (
            f"reference library built wrongly (seed {seed}: got {got.tolist()}, want {want}); the mirrored point "
            f"means right-to-left argument evaluation: build oracle/_ref with the ROCm clang++, never g++")


def _live(path):
    """A reference library that passed the build self-check; every live test goes through here,
    so a library from the wrong compiler is an error in each of them and is never compared."""
    if not path.exists():
        pytest.skip(f"{path.relative_to(ROOT)} not built (no reference tree on this machine)")
    lib = load_reference(path)
    check_draw_order(lib)
    return lib


@pytest.fixture(scope="module")
def ref_om():
    return _live(REF_OM)


@pytest.fixture(scope="module")
def ref_libm():
    return _live(REF_LIBM)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_reference_build_draws_left_to_right(ref_om, ref_libm):
    check_draw_order(ref_om)
    check_draw_order(ref_libm)


def test_smoothness_threshold_is_never_met_exactly():
    """Why 0.0316 / 0.0317 are the sharpest pair there is: alpha = r * r in float32 never EQUALS
    1e-3f (the squares of the two float32 neighbours of sqrt(1e-3) fall either side of it, and
    r * r is monotonic), so `alpha < 1e-3f` and `alpha <= 1e-3f` are the same function of the
    roughness and no input tells them apart; a threshold moved by half a percent is caught."""
    t = np.float32(1e-3)
    hi = np.float32(math.sqrt(float(t)))
    if hi * hi < t:
        hi = np.nextafter(hi, np.float32(1))
    lo = np.nextafter(hi, np.float32(0))
    assert lo * lo < t < hi * hi
    a, b = np.float32(0.0316), np.float32(0.0317)
    assert a * a < t < b * b and b * b < np.float32(1.005e-3)


def test_interposed_math_stays_inside_the_library(ref_om, golden_inputs):
    """libptref_om.so defines sinf/cosf/expf for itself only: asked for by name it hands out
    libm's, and the oracle's camera, which calls libm's sinf/cosf/tanf, still gives its golden
    bits with the library loaded."""
    from optixpathtracer_amd import scenes

    libm = C.CDLL("libm.so.6")
    for name in ("sinf", "cosf", "expf"):
        assert C.cast(getattr(ref_om, name), C.c_void_p).value == C.cast(getattr(libm, name), C.c_void_p).value
    cam = np.concatenate(O.camera_from_blender(*scenes.SCENE2_CAMERA, 40.0, 1920, 1080))
    assert np.array_equal(cam.view(np.uint32), golden_inputs["camera"][2].view(np.uint32))


def test_live_rng(ref_om, golden_inputs):
    """tea<16> and rnd of random.h on the inputs of tests/golden/golden.npz."""
    for a, b in golden_inputs["tea_in"]:
        assert ref_om.ref_tea16(int(a), int(b)) == O.tea16(int(a), int(b))
    for seed in golden_inputs["rnd_seeds"]:
        out = np.zeros(16, np.float32)
        s = C.c_uint32()
        ref_om.ref_rnd_seq(int(seed), 16, O.fp(out), C.byref(s))
        want, want_seed = O.rnd_seq(int(seed), 16)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and s.value == want_seed


@pytest.fixture(scope="module")
def golden_inputs():
    return np.load(ROOT / "tests" / "golden" / "golden.npz")


@pytest.mark.parametrize("model,ri", PAIRS, ids=PAIR_IDS)
def test_live_bsdf_bits(ref_om, model, ri):
    """Every case of the input set, oracle against libptref_om.so: all bits equal."""
    ref = reference_side(ref_om)
    c = build_cases(model, ri)
    assert c["n_random"] >= 256
    rs = run_sample(ref, c)
    check_pair(oracle_side(), c, rs, run_eval_pdf(ref, with_sampled(c, rs[1])))


@pytest.mark.parametrize("model,ri", PAIRS, ids=PAIR_IDS)
def test_live_libm_leg(ref_libm, model, ri):
    """What is exact without the polynomials, against libptref.so (libm's sinf/cosf/expf): it is
    not the interposition that makes the two sides agree.  Return values, flags and seeds are
    equal everywhere; f and pdf of Lambert, Conductor and Dielectric call no transcendental and
    match bit for bit, and so do the specular samples of Conductor and Dielectric (Layered's
    pass through Transmittance's exp, GlossyDiffuse.h:97-105, Lambert's through sin/cos).
    Layered's f is left out whole, seed included: its random walk branches on values that carry
    exp and sin/cos (Russian roulette at GlossyDiffuse.h:254-257), so an ulp can change how many
    numbers it draws; with this libm that happens in 1 of the 13,248 Layered evaluations."""
    ref, orc = reference_side(ref_libm), oracle_side()
    c = build_cases(model, ri)
    r_ok, r_out, r_seed = run_sample(ref, c)
    ok, out, seed = run_sample(orc, c)
    assert_same_bits("Sample_f return value", ok, r_ok.astype(np.int32), c)
    assert_same_bits("flags", out[:, 7], r_out[:, 7], c)
    assert_same_bits("seed after Sample_f", seed, r_seed, c)
    if model in ("conductor", "dielectric"):
        spec = (out[:, 7].view(np.float32).astype(np.int32) & 4) != 0
        assert spec.any() == (ROUGHNESS[ri] ** 2 < 1e-3)
        assert_same_bits("specular sample", out[spec], r_out[spec], subset(c, spec))
    c = with_sampled(c, r_out)
    f, fs, p = run_eval_pdf(orc, c)
    r_f, r_fs, r_p = run_eval_pdf(ref, c)
    if model != "layered":
        assert_same_bits("f", f, r_f, c)
        assert_same_bits("seed after f", fs, r_fs, c)
        assert_same_bits("pdf", p, r_p, c)


def test_live_golden_is_current(ref_om, golden):
    """The committed golden file is what libptref_om.so gives today."""
    import sys

    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    try:
        import make_reference_golden as G
    finally:
        sys.path.pop(0)
    fresh = G.make(ref_om)
    assert sorted(fresh) == sorted(golden.files)
    for k in fresh:
        assert np.array_equal(fresh[k], golden[k]), k


# --- camera -----------------------------------------------------------------------------------
def camera_poses():
    """(blender position, blender rotation in degrees, fov, width, height): the two cameras of the
    five timed scenes at 1920x1080, 0/90/180 degrees on each axis in turn, and random poses with FOV
    10..120 at aspect 1:1, 16:9 and 1:4."""
    from optixpathtracer_amd import scenes

    poses = [(*scenes.SCENE1_CAMERA, 40.0, 1920, 1080), (*scenes.SCENE2_CAMERA, 40.0, 1920, 1080)]
    sizes = [(512, 512), (1920, 1080), (256, 1024)]
    rng = np.random.default_rng(77)
    k = 0
    for axis in range(3):
        for deg in (0.0, 90.0, 180.0):
            rot = list(rng.uniform(20.0, 70.0, 3))
            rot[axis] = deg
            poses.append((tuple(rng.uniform(-5, 5, 3)), tuple(rot), 40.0, *sizes[k % 3]))
            k += 1
    while len(poses) < 64:
        rot = rng.uniform(-180.0, 180.0, 3)
        if k % 4 == 0:  # right angles mixed into a random pose
            rot[rng.integers(3)] = rng.choice([0.0, 90.0, 180.0, -90.0])
        poses.append((tuple(rng.uniform(-10, 10, 3)), tuple(rot), float(rng.uniform(10.0, 120.0)), *sizes[k % 3]))
        k += 1
    return poses


def test_live_camera_bits(ref_libm):
    """Camera.cpp + GlmHelperMethods.cpp as they are, composed as OptixRenderer::SetCamera does
    (OptixRenderer.cpp:662-668), against orc_camera_from_blender: position, inverse view and
    inverse projection bit for bit over 64 poses.  Both sides call the same libm (libptref.so,
    not the interposed library: the oracle's camera uses libm's sinf/cosf/tanf).

    A camera looking exactly along world up (Blender x rotation 0 or 180) has a singular view
    matrix on both sides and its inverse is NaN on both sides; IEEE 754 leaves a NaN's sign and
    payload open, so a NaN has to meet a NaN and every other value its exact bits."""
    def bits(a):
        a = np.concatenate(a)
        return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))

    n_nan = 0
    poses = camera_poses()
    assert len(poses) == 64
    for pos, rot, fov, w, h in poses:
        p, iv, ip = np.zeros(3, np.float32), np.zeros(16, np.float32), np.zeros(16, np.float32)
        ref_libm.ref_camera_from_blender(O.fp(O._f(pos)), O.fp(O._f(rot)), float(fov), w, h, O.fp(p), O.fp(iv),
                                         O.fp(ip))
        got = bits(O.camera_from_blender(pos, rot, fov, w, h))
        want = bits([p, iv, ip])
        n_nan += bool(np.isnan(iv).any())
        assert np.array_equal(got, want), (
            f"pose {pos} {rot} fov {fov} {w}x{h}: oracle {got.view(np.float32).tolist()} "
            f"reference {want.view(np.float32).tolist()}")
    assert n_nan <= sum(1 for _, rot, *_ in poses if rot[0] in (0.0, 180.0))  # only looking along world up


# ----------------------------------------------------------------------------------------------
# golden tier (never skips)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,ri", PAIRS, ids=PAIR_IDS)
def test_golden_bsdf_bits(golden, model, ri):
    """The oracle reproduces the recorded bits of libptref_om.so on the golden subset."""
    full = build_cases(model, ri)
    c = subset(full, golden_index(full))
    k = PAIRS.index((model, ri))
    lo, hi = int(golden["offset"][k]), int(golden["offset"][k + 1])
    assert hi - lo == len(c["wo"]) and hi - lo >= N_RANDOM // GOLDEN_STRIDE
    rs = (golden["sample_ok"][lo:hi].astype(np.int32), golden["sample_out"][lo:hi], golden["sample_seed"][lo:hi])
    check_pair(oracle_side(), c, rs, (golden["eval_f"][lo:hi], golden["eval_seed"][lo:hi], golden["pdf"][lo:hi]))


def test_golden_holds_results_only(golden):
    assert sorted(golden.files) == ["eval_f", "eval_seed", "offset", "pdf", "sample_ok", "sample_out", "sample_seed"]
    assert all(golden[k].dtype.kind in "ui" for k in golden.files)
    assert GOLDEN.stat().st_size < 200 * 1024
    # the input set exercises both outcomes and all four lobe kinds somewhere
    flags = golden["sample_out"][:, 7].view(np.float32).astype(np.int32)
    assert set(np.unique(golden["sample_ok"])) == {0, 1}
    assert {1 | 4, 2 | 4, 1 | 8, 2 | 8, 1} <= set(np.unique(flags[golden["sample_ok"] == 1]))
