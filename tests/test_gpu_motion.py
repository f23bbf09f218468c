"""Motion vectors (pt_temporal_options.motion_vectors, pt_motion_*; DESIGN.md §11 "Motion vectors"):
the G-buffer's barycentrics are the oracle trace's; after committed mesh moves a call with the option
on equals the numpy restatement with the previous positions (motion_ref.motion_ref) bit for bit,
output, state, previous positions, screen motion and counters; the state rule holds (when the motion
kernel runs, when it falls back); and following the moved spheres denoises them better."""
import functools

import numpy as np
import pytest
from denoise_ref import AOVS, oracle_gbuffer, same_bits, scene_by_name
from motion_ref import (inflated, left_multiplied, mesh_of_triangle, motion_ref, oracle_guides, prev_position, translation,
                        wall_matrix, world_triangles)
from temporal_ref import camera_of, with_camera
from test_gpu_temporal import CAMERAS, SUBPIXEL_PAN

pytestmark = pytest.mark.gpu

SIZES = [(48, 32), (33, 17), (5, 3)]  # one tile and more than one, partial tiles, a few pixels
KINDS = ["history_length", "moments", "variance", "color"]
WALL = 4
CASES = ["wall", "rebuild", "deform", "two_commits", "move_and_pan"]


def _renderer(scene, w, h, depth=4):
    from optixpathtracer_amd.renderer import setup_renderer

    return setup_renderer(scene, w, h, depth)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def _guides(name, w, h):
    return oracle_guides(scene_by_name(name), w, h)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["tiny:diffuse", "textured:diffuse"])
def test_barycentrics(name, size):
    """motion("barycentric") is u, v of the oracle's trace of the camera rays (0, 0 at a miss), and
    the seven AOVs are what they were."""
    w, h = size
    g = _guides(name, w, h)
    r = _renderer(scene_by_name(name), w, h)
    b = r.motion("barycentric")
    got = {k: r.aov(k) for k in AOVS}
    assert r.denoise_info()["gbuffer_renders"] == 1
    r.close()
    assert b.shape == (h, w, 2) and b.dtype == np.float32
    assert same_bits(b[..., 0], g["u"]) and same_bits(b[..., 1], g["v"])
    ref = oracle_gbuffer(name, w, h)
    for k in AOVS:
        np.testing.assert_array_equal(_bits(got[k]), _bits(ref[k]), err_msg=k)
    if size == (48, 32):
        hit = g["prim"] >= 0
        assert hit.any() and (b[hit] != 0).any()
        if name.startswith("textured"):
            assert (~hit).any() and (b[~hit] == 0).all()


def _case(case):
    """(scene name, cameras of the three calls, [(how, [(mesh, scene after this change)])] commits)."""
    name = "tiny:diffuse"  # (the pan's cameras are inside the box that both scenes share)
    sc = scene_by_name(name)
    cams = [None, None, None]
    if case in ("wall", "rebuild"):
        commits = [("rebuild" if case == "rebuild" else "refit", [(WALL, left_multiplied(sc, WALL, wall_matrix()))])]
    elif case == "deform":
        commits = [("refit", [(3, inflated(sc, 3, 0.03))])]
    elif case == "two_commits":
        first = left_multiplied(sc, WALL, wall_matrix())
        commits = [("refit", [(WALL, first)]), ("refit", [(0, left_multiplied(first, 0, translation(0.05, 0.02, 0.0)))])]
    else:
        cams = [CAMERAS[SUBPIXEL_PAN - 1], CAMERAS[SUBPIXEL_PAN - 1], CAMERAS[SUBPIXEL_PAN]]
        commits = [("refit", [(WALL, left_multiplied(sc, WALL, wall_matrix()))])]
    return name, sc, cams, commits


def _apply(r, before, mesh, after):
    """Stages on the renderer what turns mesh `mesh` of scene `before` into that of `after`."""
    a, b = before.meshes[mesh], after.meshes[mesh]
    if not np.array_equal(np.asarray(a.model), np.asarray(b.model)):
        r.set_mesh_transform(mesh, b.model)
    if not np.array_equal(np.asarray(a.vertices), np.asarray(b.vertices)):
        r.set_mesh_vertices(mesh, b.vertices)


def _images(case, w, h):
    rng = np.random.default_rng(100 * CASES.index(case) + 10 * w + h)
    return [(rng.random((h, w, 3)) * 2.0).astype(np.float32) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _reference(case, w, h):
    """[(out, state)] of the three calls: two static ones, then the moved scene with the previous positions."""
    name, sc, cams, commits = _case(case)
    final = commits[-1][1][-1][1]
    view = lambda scene, k: scene if cams[k] is None else with_camera(scene, *cams[k])
    imgs = _images(case, w, h)
    seq, st = [], None
    for k in range(2):
        g = oracle_guides(view(sc, k), w, h) if k == 0 or cams[k] != cams[k - 1] else g
        out, st = motion_ref(st, imgs[k], g, camera_of(view(sc, k), w, h))
        seq.append((out, st))
    g = oracle_guides(view(final, 2), w, h)
    pp = prev_position(world_triangles(sc), g["prim"], g["u"], g["v"])
    seq.append(motion_ref(st, imgs[2], g, camera_of(view(final, 2), w, h), prev_pos=pp))
    return seq, g, final


def _check(r, out, st, got, k):
    assert same_bits(got, out), (k, int((got.view(np.uint32) != out.view(np.uint32)).sum()))
    want = {"history_length": st["length"], "moments": st["moments"], "variance": st["variance"], "color": st["color"]}
    assert [q for q in KINDS if not same_bits(r.temporal_state(q), want[q])] == [], k
    assert same_bits(r.motion("prev_position"), st["prev_position"]), k
    assert same_bits(r.motion("screen"), st["screen"]), k
    info = r.temporal_info()
    assert (info["reprojected_pixels"], info["reset_pixels"]) == (st["reprojected"], st["reset"]), k
    return info


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES)
def test_sequence_matches_restatement(case, size):
    """Two static calls, then the committed change(s) and a call with the option on: output, the four
    state kinds, the previous positions, the screen motion and the three counters are the
    restatement's, and the motion kernel ran.  This is the test that fails without the feature."""
    w, h = size
    name, sc, cams, commits = _case(case)
    seq, g, final = _reference(case, w, h)
    imgs = _images(case, w, h)
    if size == (48, 32):  # the case is what it is meant to be: pixels moved, and most of them are followed
        last = seq[2][1]
        assert last["moved"] > 0 and last["accepted"][(last["prev_position"] != g["position"]).any(-1)].mean() > 0.5
    r = _renderer(sc, w, h)
    for k in range(2):
        if cams[k] is not None:
            r.SetCameraBlender(*cams[k], sc.fov_deg)
        info = _check(r, *seq[k], r.denoise_temporal(imgs[k], motion_vectors=1), k)
        assert (info["motion_used"], info["moved_pixels"]) == (0, 0), k
        assert (info["snapshot_ms"] > 0) == (k == 0), k  # one copy of the vertices: nothing was committed since
    before = sc
    for how, changes in commits:
        for mesh, after in changes:
            _apply(r, before, mesh, after)
            before = after
        r.commit_geometry(how)
    if cams[2] is not None:
        r.SetCameraBlender(*cams[2], sc.fov_deg)
    info = _check(r, *seq[2], r.denoise_temporal(imgs[2], motion_vectors=1), 2)
    assert info["motion_used"] == 1
    assert info["moved_pixels"] == seq[2][1]["moved"]
    assert info["snapshot_ms"] > 0 and info["calls"] == 3 and info["history_valid"] == 1
    r.close()


def test_invariants():
    """Off the moved mesh the previous position is the position; no commit, no motion kernel and the
    option-off results; off -> on falls back for one call, then follows; so do a reset and a resize;
    and the two kinds of the last call are refused after a call with the option off."""
    from optixpathtracer_amd import capi

    w, h = 48, 32
    sc = scene_by_name("tiny:diffuse")
    tri_mesh = mesh_of_triangle(sc)
    rng = np.random.default_rng(5)
    imgs = [(rng.random((h, w, 3)) * 2.0).astype(np.float32) for _ in range(4)]
    r = _renderer(sc, w, h)
    moves = iter(range(1, 100))

    def move(mesh):
        """One more committed translation of `mesh`, different each time."""
        k = next(moves)
        r.set_mesh_transform(mesh, translation(0.01 * k, 0.0, -0.01 * k).T.reshape(16))
        r.commit_geometry("refit")

    def state():
        return [r.temporal_state(q) for q in KINDS]

    # the option off throughout, as the comparison for what follows
    off = []
    for img in imgs[:3]:
        off.append((r.denoise_temporal(img), state()))
    for kind in ("prev_position", "screen"):
        with pytest.raises(capi.PTError) as e:
            r.motion(kind)
        assert e.value.status == capi.PT_ERR_STATE and "motion_vectors" in str(e.value)
    assert r.motion("barycentric").shape == (h, w, 2)  # the G-buffer's own: always there
    # the same inputs with the option on and no commit: the plain kernel, the same bits
    r.temporal_reset()
    for k, img in enumerate(imgs[:3]):
        got = r.denoise_temporal(img, motion_vectors=1)
        info = r.temporal_info()
        assert info["motion_used"] == 0 and info["moved_pixels"] == 0, k
        assert same_bits(got, off[k][0]) and all(same_bits(a, b) for a, b in zip(state(), off[k][1])), k
        assert same_bits(r.motion("prev_position"), r.aov("position")), k
        assert (r.motion("screen")[..., 2] == (1.0 if k else 0.0))[r.aov("prim") >= 0].all(), k
    # a move of mesh k: the motion kernel, and off k the previous position is the position
    move(1)
    r.denoise_temporal(imgs[3], motion_vectors=1)
    info = r.temporal_info()
    prim, pos, pp = r.aov("prim"), r.aov("position"), r.motion("prev_position")
    on_mesh = (prim >= 0) & (tri_mesh[np.clip(prim, 0, None)] == 1)
    assert info["motion_used"] == 1 and info["moved_pixels"] == int(on_mesh.sum()) > 0
    assert same_bits(pp[~on_mesh], pos[~on_mesh]) and (pp[on_mesh] != pos[on_mesh]).any(-1).all()
    # off -> on: the snapshot is not the previous call's, so one call falls back, the next follows
    r.denoise_temporal(imgs[0])
    assert r.temporal_info()["motion_used"] == 0
    move(1)
    r.denoise_temporal(imgs[1], motion_vectors=1)
    info = r.temporal_info()
    assert info["motion_used"] == 0 and info["moved_pixels"] == 0 and info["reprojected_pixels"] > 0 and info["snapshot_ms"] > 0
    assert same_bits(r.motion("prev_position"), r.aov("position"))
    move(1)
    r.denoise_temporal(imgs[2], motion_vectors=1)
    info = r.temporal_info()
    assert info["motion_used"] == 1 and info["moved_pixels"] > 0

    # a reset and a resize: no history in the next call, the one after follows
    def starts_again_then_follows():
        r.denoise_temporal(imgs[0], motion_vectors=1)
        info = r.temporal_info()
        assert info["motion_used"] == 0 and info["reprojected_pixels"] == 0 and info["reset_pixels"] == int((r.aov("prim") >= 0).sum())
        assert (r.motion("screen") == 0).all()
        move(2)
        r.denoise_temporal(imgs[1], motion_vectors=1)
        info = r.temporal_info()
        assert info["motion_used"] == 1 and info["moved_pixels"] > 0 and info["reprojected_pixels"] > 0

    move(2)
    r.temporal_reset()
    starts_again_then_follows()
    r.Resize((w, h))
    with pytest.raises(capi.PTError):
        r.motion("prev_position")
    starts_again_then_follows()
    r.close()


CPU_MSE = (0.00048013, 0.00108700)  # option on, option off: the docstring of the quality test says how they were derived
CAP = 0.6646  # the square root of their ratio


def _sphere_mse(img, ref, sph):
    d = (np.nan_to_num(np.asarray(img, np.float64)) - np.asarray(ref, np.float64))[sph]
    return float(np.mean(d ** 2))


def test_following_the_spheres_denoises_them():
    """Eight static 1-spp calls (frame ids 1..8) on tiny:diffuse at 96 x 64, Lambert, depth 4; then the
    four sphere meshes move by (0, 0, 0.1) and frame 9 is filtered, against 512 spp of the moved scene,
    over the pixels that show a sphere.  Derived on the CPU with the oracle's images and the
    restatement: 262 pixels show a sphere; with the option on 260 of them take up history and
    m(on) = 0.00048013, with it off none does and m(off) = 0.00108700; ratio 0.4417, and the cap is its
    square root, 0.6646 (halfway, in log scale, to no gain).  Whole image, on: 6060 pixels reprojected,
    84 reset, 262 moved; off: 5800 and 344."""
    name, w, h = "tiny:diffuse", 96, 64
    sc = scene_by_name(name)
    tri_mesh = mesh_of_triangle(sc)
    res = {}
    for option in (1, 0):
        r = _renderer(sc, w, h, depth=4)
        r.set_material_mode(1)
        for k in range(1, 9):
            r.render_accumulate(1, k)
            r.denoise_temporal("accum", motion_vectors=option)
        for mesh in range(4):
            r.set_mesh_transform(mesh, translation(0.0, 0.0, 0.1).T.reshape(16))
        r.commit_geometry("refit")
        ref = r.render_accumulate(512, 1000)
        r.render_accumulate(1, 9)
        img = r.denoise_temporal("accum", motion_vectors=option)
        prim = r.aov("prim")
        sph = (prim >= 0) & (tri_mesh[np.clip(prim, 0, None)] < 4)
        accepted = int((r.temporal_state("history_length")[sph] > 1).sum())
        res[option] = (_sphere_mse(img, ref, sph), int(sph.sum()), accepted, r.temporal_info())
        r.close()
    (m_on, n, a_on, i_on), (m_off, n_off, a_off, i_off) = res[1], res[0]
    print(f"sphere pixels={n} accepted on={a_on} off={a_off} mse on={m_on:.8f} off={m_off:.8f} ratio={m_on / m_off:.4f} "
          f"moved={i_on['moved_pixels']}")
    assert n == n_off >= 200
    assert a_on >= 0.95 * n and a_off == 0
    assert i_on["motion_used"] == 1 and i_off["motion_used"] == 0 and i_on["moved_pixels"] == n
    assert (i_on["reprojected_pixels"], i_on["reset_pixels"]) == (6060, 84)
    assert (i_off["reprojected_pixels"], i_off["reset_pixels"]) == (5800, 344)
    assert m_on < m_off
    assert m_on / m_off <= CAP
    assert (m_on, m_off) == pytest.approx(CPU_MSE, rel=1e-3)  # the CPU figures


