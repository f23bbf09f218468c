"""First-hit feature buffers (pt_aov_*): every AOV of every pixel equals the CPU oracle's record of
the path's first bounce bit for bit, misses included, and the G-buffer is rendered again only when
the size, the camera or the committed geometry changed."""
import dataclasses

import numpy as np
import pytest
from denoise_ref import AOVS, oracle_gbuffer, scene_by_name

pytestmark = pytest.mark.gpu

W, H = 48, 32


def _aovs(r):
    return {k: r.aov(k) for k in AOVS}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["tiny:diffuse", "textured:diffuse", "sphere_box_diffuse"])
def test_aovs_match_oracle(name):
    from optixpathtracer_amd.renderer import setup_renderer

    ref = oracle_gbuffer(name, W, H)
    r = setup_renderer(scene_by_name(name), W, H, 4)
    got = _aovs(r)
    info = r.denoise_info()
    r.close()
    hit = ref["prim"] >= 0
    print(f"{name}: {int(hit.sum())} hits, {int((~hit).sum())} misses")
    if name.startswith("textured"):
        assert hit.any() and (~hit).any()  # both branches run
    # the oracle's closest-hit trace and its path agree on what the camera ray hits
    np.testing.assert_array_equal(ref["trace_prim"], ref["prim"])
    for k in AOVS:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        np.testing.assert_array_equal(_bits(got[k]), _bits(ref[k]), err_msg=k)
    for k in AOVS:  # a miss is prim -1 and zeros
        if k != "prim":
            assert not _bits(got[k][~hit]).any(), k
    assert info["hit_pixels"] == int(hit.sum()) and info["gbuffer_renders"] == 1 and info["gbuffer_ms"] > 0.0


def test_aov_does_not_depend_on_frame_mode_or_kernel():
    from optixpathtracer_amd.renderer import setup_renderer

    r = setup_renderer(scene_by_name("textured:diffuse"), W, H, 4)
    a = _aovs(r)
    r.set_material_mode(3)
    r.set_kernel(0)
    r.render_frames(7, 2)
    b = _aovs(r)
    assert r.denoise_info()["gbuffer_renders"] == 1
    r.close()
    for k in AOVS:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)


def test_gbuffer_is_cached_until_the_view_changes():
    from optixpathtracer_amd import capi
    from optixpathtracer_amd.renderer import setup_renderer

    sc = scene_by_name("tiny:diffuse")
    r = setup_renderer(sc, W, H, 4)
    assert r.lib.pt_aov_device_ptr(r.h, capi.PT_AOV_DEPTH) is None  # NULL until rendered
    first = _aovs(r)
    r.aov("depth")
    assert r.denoise_info()["gbuffer_renders"] == 1
    assert r.lib.pt_aov_device_ptr(r.h, capi.PT_AOV_DEPTH) is not None
    r.SetLights(sc.lights)  # the first hit does not depend on the lights
    r.aov("prim")
    assert r.denoise_info()["gbuffer_renders"] == 1

    pos = np.asarray(sc.camera_blender_pos, np.float32) + np.float32([0.25, 0.0, 0.1])
    r.SetCameraBlender(pos, sc.camera_blender_rot, sc.fov_deg)
    moved_cam = r.aov("position")
    assert r.denoise_info()["gbuffer_renders"] == 2
    assert (_bits(moved_cam) != _bits(first["position"])).any()

    r.Resize((33, 17))
    r.SetCameraBlender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg)
    small = r.aov("depth")
    assert small.shape == (17, 33) and r.denoise_info()["gbuffer_renders"] == 3
    r.Resize((W, H))
    r.SetCameraBlender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg)
    back = _aovs(r)
    assert r.denoise_info()["gbuffer_renders"] == 4
    for k in AOVS:
        np.testing.assert_array_equal(_bits(back[k]), _bits(first[k]), err_msg=k)

    # a staged move changes nothing; the commit does
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = [0.2, 0.1, -0.15]
    mesh = 0  # one of the spheres
    r.set_mesh_transform(mesh, m.T.ravel())
    r.aov("prim")
    assert r.denoise_info()["gbuffer_renders"] == 4
    r.commit_geometry("refit")
    after = _aovs(r)
    assert r.denoise_info()["gbuffer_renders"] == 5
    r.aov("albedo")
    assert r.denoise_info()["gbuffer_renders"] == 5
    r.close()
    assert any((_bits(after[k]) != _bits(first[k])).any() for k in AOVS)

    moved = dataclasses.replace(sc, meshes=[dataclasses.replace(me, model=np.ascontiguousarray(m.T.ravel()))
                                            if i == mesh else me for i, me in enumerate(sc.meshes)])
    f = setup_renderer(moved, W, H, 4)
    fresh = _aovs(f)
    f.close()
    for k in AOVS:
        np.testing.assert_array_equal(_bits(after[k]), _bits(fresh[k]), err_msg=k)


def test_aov_errors():
    from optixpathtracer_amd import capi
    from optixpathtracer_amd.renderer import OptixRenderer

    sc = scene_by_name("tiny:diffuse")
    r = OptixRenderer(None, sc)
    buf = np.zeros((H, W), np.float32)
    assert r.lib.pt_aov_download(r.h, capi.PT_AOV_DEPTH, buf.ctypes.data, buf.nbytes) == capi.PT_ERR_STATE  # no size yet
    assert b"pt_resize" in r.lib.pt_last_error()
    r.Resize((W, H))
    r.SetCameraBlender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg)
    assert r.lib.pt_aov_download(r.h, 7, buf.ctypes.data, buf.nbytes) == capi.PT_ERR_INVALID
    assert b"kind" in r.lib.pt_last_error()
    assert r.lib.pt_aov_download(r.h, capi.PT_AOV_DEPTH, buf.ctypes.data, buf.nbytes - 4) == capi.PT_ERR_INVALID
    assert b"bytes" in r.lib.pt_last_error()
    assert r.lib.pt_aov_download(r.h, capi.PT_AOV_ALBEDO, buf.ctypes.data, buf.nbytes) == capi.PT_ERR_INVALID
    assert r.lib.pt_aov_device_ptr(r.h, 9) is None
    assert r.aov("depth").shape == (H, W)  # a valid call afterwards still works
    r.close()
