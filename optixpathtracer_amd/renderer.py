"""Host-side mirror of the reference's render interface, over the C ABI.

`OptixRenderer` keeps the method names and semantics of
`Renderer/OptiX/OptixRenderer.h:63-76` (Resize, Render, SetCamera, SetLights,
SetMaxBounces) so caller code reads like the reference's `OptixView`/`main`; the extra
methods expose the device-resident accumulation that replaces the per-spp download + GL
blend (`Renderer/OptixView.cpp:201-255`).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi
from .capi import check, fptr, load
from .scenes import Scene


def _f32(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


class _SceneBinding:
    """Owns the ctypes `pt_scene` and keeps every numpy buffer it points to alive."""

    def __init__(self, scene: Scene):
        self.keep = []
        meshes = (capi.pt_mesh * max(1, len(scene.meshes)))()
        for i, m in enumerate(scene.meshes):
            v = _f32(m.vertices)
            idx = np.ascontiguousarray(m.indices, dtype=np.int32)
            self.keep += [v, idx]
            pm = meshes[i]
            pm.vertices = fptr(v)
            pm.indices = idx.ctypes.data_as(C.POINTER(C.c_int32))
            if m.normals is not None:
                n = _f32(m.normals)
                self.keep.append(n)
                pm.normals = fptr(n)
            if m.texcoords is not None:
                t = _f32(m.texcoords)
                self.keep.append(t)
                pm.texcoords = fptr(t)
            pm.n_vertices = int(v.shape[0])
            pm.n_triangles = int(idx.shape[0])
            pm.model_matrix[:] = [float(x) for x in _f32(m.model).ravel()]
            pm.albedo[:] = [float(x) for x in m.albedo]
            pm.metallic = float(m.metallic)
            pm.roughness = float(m.roughness)
            pm.albedo_tex = int(getattr(m, "albedo_tex", -1))
            pm.normal_tex = int(getattr(m, "normal_tex", -1))
            pm.metal_rough_tex = int(getattr(m, "metal_rough_tex", -1))
        texs = list(getattr(scene, "textures", []) or [])
        tarr = (capi.pt_texture * max(1, len(texs)))()
        for i, t in enumerate(texs):
            px = np.ascontiguousarray(t, dtype=np.uint32)
            self.keep.append(px)
            tarr[i].rgba8 = px.ctypes.data_as(C.POINTER(C.c_uint32))
            tarr[i].height, tarr[i].width = int(px.shape[0]), int(px.shape[1])
        self.meshes = meshes
        self.textures = tarr
        self.scene = capi.pt_scene()
        self.scene.meshes = C.cast(meshes, C.POINTER(capi.pt_mesh))
        self.scene.n_meshes = len(scene.meshes)
        self.scene.textures = C.cast(tarr, C.POINTER(capi.pt_texture))
        self.scene.n_textures = len(texs)


def camera_from_blender(pos, rot, fov_deg: float, width: int, height: int):
    """Camera.cpp:6-70 + OptixRenderer::SetCamera: (position, inverse view, inverse projection)."""
    lib = load()
    p = np.empty(3, np.float32)
    iv = np.empty(16, np.float32)
    ip = np.empty(16, np.float32)
    check(lib.pt_camera_from_blender(fptr(_f32(pos)), fptr(_f32(rot)), float(fov_deg), int(width), int(height),
                                     fptr(p), fptr(iv), fptr(ip)), "pt_camera_from_blender")
    return p, iv, ip


class OptixRenderer:
    """Drop-in for `OptixRenderer` (OptixRenderer.h:8-110) backed by libptamd.so."""

    def __init__(self, ptx_path_or_none, model: Scene, device: int = 0, material_mode: int | None = None,
                 kernel: int = capi.PT_KERNEL_AUTO, bvh_builder: int = capi.PT_BVH_AUTO, devices=None):
        """devices: None = the single `device`; a list of ordinals = one renderer over all of them
        (frame ids of render_frames split across the devices, RCCL-summed onto devices[0])."""
        # ptxPath is accepted for signature compatibility and ignored (no PTX on gfx950).
        self.lib = load()
        self.model = model
        self._caller_model = model
        self._binding = _SceneBinding(model)
        opts = capi.pt_options()
        opts.device = int(device)
        opts.material_mode = int(model.material_mode if material_mode is None else material_mode)
        opts.kernel = int(kernel)
        opts.bvh_builder = int(bvh_builder)
        if devices is not None:
            self._devlist = (C.c_int32 * max(1, len(devices)))(*[int(d) for d in devices])
            opts.n_devices = len(devices)
            opts.device_list = self._devlist
        h = C.c_void_p()
        check(self.lib.pt_create(C.byref(self._binding.scene), C.byref(opts), C.byref(h)), "pt_create")
        self.h = h
        self.size = (0, 0)

    # ---- reference API --------------------------------------------------------------
    def Resize(self, new_size) -> None:  # OptixRenderer.cpp:649-660
        w, h = int(new_size[0]), int(new_size[1])
        check(self.lib.pt_resize(self.h, w, h), "pt_resize")
        if w and h:
            self.size = (w, h)

    def Render(self, h_pixels: np.ndarray | None = None) -> np.ndarray:  # :617-647
        w, h = self.size
        out = h_pixels if h_pixels is not None else np.zeros((h, w, 3), np.float32)
        if w == 0:
            return out
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == w * h * 3
        check(self.lib.pt_render(self.h, fptr(out)), "pt_render")
        return out

    def launch(self, color_buffer_ptr: int, size, frame_id: int, position, inverse_view, inverse_projection,
               lights_device_ptr: int, n_lights: int, max_bounces: int) -> None:
        """optixLaunch with a LaunchParams block (pt_launch): writes frame `frame_id`'s 1-spp
        radiance into the device buffer at color_buffer_ptr (W*H*3 fp32, row 0 = bottom).
        Asynchronous; call synchronize().  Device pointers, as in the reference."""
        lp = capi.pt_launch_params()
        lp.frame.color_buffer = C.c_void_p(int(color_buffer_ptr))
        lp.frame.size[0], lp.frame.size[1] = int(size[0]), int(size[1])
        lp.frame.id = int(frame_id)
        for dst, src in ((lp.camera.position, position), (lp.camera.inverse_view_matrix, inverse_view),
                         (lp.camera.inverse_projection_matrix, inverse_projection)):
            vals = _f32(src).ravel()
            for i, v in enumerate(vals):
                dst[i] = float(v)
        lp.point_lights = C.c_void_p(int(lights_device_ptr)) if lights_device_ptr else None
        lp.point_light_count = int(n_lights)
        lp.max_bounces = int(max_bounces)
        check(self.lib.pt_launch(self.h, C.byref(lp)), "pt_launch")

    def SetCamera(self, position, inverse_view, inverse_projection) -> None:  # :662-668
        check(self.lib.pt_set_camera(self.h, fptr(_f32(position)), fptr(_f32(inverse_view)),
                                     fptr(_f32(inverse_projection))), "pt_set_camera")

    def SetCameraBlender(self, pos, rot, fov_deg: float = 40.0) -> None:
        w, h = self.size
        p, iv, ip = camera_from_blender(pos, rot, fov_deg, w, h)
        self.SetCamera(p, iv, ip)

    def SetLights(self, lights) -> None:  # :670-675
        L = _f32(lights).reshape(-1, 6)
        arr = (capi.pt_point_light * max(1, len(L)))()
        for i, row in enumerate(L):
            arr[i].position[:] = [float(x) for x in row[:3]]
            arr[i].color[:] = [float(x) for x in row[3:]]
        check(self.lib.pt_set_lights(self.h, arr, len(L)), "pt_set_lights")

    def SetMaxBounces(self, n: int) -> None:  # :677-679
        check(self.lib.pt_set_max_bounces(self.h, int(n)), "pt_set_max_bounces")

    # ---- device-resident accumulation -------------------------------------------------
    def set_material_mode(self, mode: int) -> None:
        check(self.lib.pt_set_material_mode(self.h, int(mode)), "pt_set_material_mode")

    def set_kernel(self, kernel: int) -> None:
        check(self.lib.pt_set_kernel(self.h, int(kernel)), "pt_set_kernel")

    def set_render_ahead(self, frames: int) -> None:
        """pt_set_render_ahead: frames Render() may render ahead of the caller (1 = off)."""
        check(self.lib.pt_set_render_ahead(self.h, int(frames)), "pt_set_render_ahead")

    def set_render_ahead_budget(self, max_ms: float) -> None:
        """pt_set_render_ahead_budget: bound (ms of GPU time) on one render-ahead batch, 0 = none."""
        check(self.lib.pt_set_render_ahead_budget(self.h, float(max_ms)), "pt_set_render_ahead_budget")

    def set_frames_per_launch(self, frames: int) -> None:
        check(self.lib.pt_set_frames_per_launch(self.h, int(frames)), "pt_set_frames_per_launch")

    def set_queue_budget(self, nbytes: int) -> None:
        """pt_set_queue_budget: bytes for all streams' wavefront queues (0 = default, a quarter of the
        device memory; < 0 = none)."""
        check(self.lib.pt_set_queue_budget(self.h, int(nbytes)), "pt_set_queue_budget")

    def trace_coherence(self) -> dict:
        """pt_get_trace_coherence: wave steps of the trace kernels by the number of distinct global
        BVH nodes their lanes load (counted while traversal stats are on)."""
        h = (C.c_uint64 * 8)()
        check(self.lib.pt_get_trace_coherence(self.h, h), "pt_get_trace_coherence")
        keys = ["d1", "d2", "d3_4", "d5_8", "d9_16", "d17_64", "steps", "lanes"]
        return {k: int(v) for k, v in zip(keys, h)}

    def set_debug_hold(self, on: bool) -> None:
        """pt_set_debug_hold (tests): speculative look-ahead batches wait until cancelled or released."""
        check(self.lib.pt_set_debug_hold(self.h, 1 if on else 0), "pt_set_debug_hold")

    def set_traversal_stats(self, enable: bool) -> None:
        check(self.lib.pt_set_traversal_stats(self.h, 1 if enable else 0), "pt_set_traversal_stats")

    def set_kernel_timing(self, enable: bool = True) -> None:
        """Time every wavefront trace launch and every launch of the bounce's dominant shading
        kernel with its own HIP event pair (pt_stats trace_kernel_* / shade_kernel_*)."""
        check(self.lib.pt_set_kernel_timing(self.h, 1 if enable else 0), "pt_set_kernel_timing")

    # -- geometry updates (staged, then committed) ----------------------------------------------
    def _mesh_index(self, mesh: int, what: str) -> int:
        mesh = int(mesh)
        if not 0 <= mesh < len(self.model.meshes):
            raise capi.PTError(f"{what}: mesh {mesh} out of range", capi.PT_ERR_INVALID)
        return mesh

    def _replace_mesh(self, mesh: int, **kw) -> None:
        # self.model follows with copies: the caller's Scene, Mesh and arrays are left alone
        if self.model is self._caller_model:
            self.model = dataclasses.replace(self.model, meshes=list(self.model.meshes))
        self.model.meshes[mesh] = dataclasses.replace(self.model.meshes[mesh], **kw)

    def set_mesh_transform(self, mesh: int, model) -> None:
        """pt_set_mesh_transform: stage a new column-major model matrix (16 floats) for a mesh; it
        takes effect at commit_geometry().  self.model follows, so OracleScene(r.model) renders
        the geometry that the next commit puts in force."""
        mesh = self._mesh_index(mesh, "set_mesh_transform")
        m = _f32(model).reshape(16).copy()
        check(self.lib.pt_set_mesh_transform(self.h, mesh, fptr(m)), "pt_set_mesh_transform")
        self._replace_mesh(mesh, model=m)

    def set_mesh_vertices(self, mesh: int, vertices, normals=None) -> None:
        """pt_set_mesh_vertices: stage new object-space vertices (V, 3) and, unless None, normals
        (V, 3; None keeps the current ones) for a mesh; topology and texcoords stay."""
        mesh = self._mesh_index(mesh, "set_mesh_vertices")
        cur = self.model.meshes[mesh]
        v = _f32(vertices).reshape(-1, 3).copy()
        if v.shape != np.asarray(cur.vertices).shape:
            raise capi.PTError("set_mesh_vertices: the vertex count cannot change", capi.PT_ERR_INVALID)
        n = None
        if normals is not None:
            n = _f32(normals).reshape(-1, 3).copy()
            if n.shape != v.shape:
                raise capi.PTError("set_mesh_vertices: normals must match the vertices", capi.PT_ERR_INVALID)
        check(self.lib.pt_set_mesh_vertices(self.h, mesh, fptr(v), fptr(n) if n is not None else None),
              "pt_set_mesh_vertices")
        self._replace_mesh(mesh, vertices=v, **({} if n is None else {"normals": n}))

    def commit_geometry(self, how: str = "refit") -> None:
        """pt_commit_geometry: put the staged mesh changes in force, by a BVH refit ("refit") or a
        rebuild with the renderer's builder ("rebuild").  Synchronous; nothing staged is a no-op."""
        modes = {"refit": capi.PT_GEOM_REFIT, "rebuild": capi.PT_GEOM_REBUILD}
        if how not in modes:
            raise capi.PTError(f"commit_geometry: how must be 'refit' or 'rebuild', not {how!r}", capi.PT_ERR_INVALID)
        check(self.lib.pt_commit_geometry(self.h, modes[how]), "pt_commit_geometry")

    # -- headless progressive view (OptixView accumulation on the device) -------------------
    def display_reset(self, max_samples: int = -1) -> None:
        check(self.lib.pt_display_reset(self.h, int(max_samples)), "pt_display_reset")

    def display_add_frame(self) -> int:
        n = C.c_int32(0)
        check(self.lib.pt_display_add_frame(self.h, C.byref(n)), "pt_display_add_frame")
        return n.value

    def display(self) -> np.ndarray:
        w, h = self.size
        out = np.empty((h, w, 3), dtype=np.float32)
        check(self.lib.pt_display_download(self.h, fptr(out)), "pt_display_download")
        return out

    # -- first-hit feature buffers and the denoiser ----------------------------------------------
    def aov(self, kind) -> np.ndarray:
        """pt_aov_download: one first-hit feature buffer of the present size, camera and geometry,
        by name (capi.AOV_KINDS) or PT_AOV_* value: (H, W, channels) float32, (H, W) for depth, and
        (H, W) int32 for prim (-1 = miss).  Row 0 = bottom.  The G-buffer is rendered only when the
        size, camera or committed geometry changed since the cached one."""
        k = capi.AOV_KINDS[kind] if isinstance(kind, str) else int(kind)
        ch = int(self.lib.pt_aov_channels(k))
        if ch < 0:
            raise capi.PTError(f"aov: no such kind {kind!r}", capi.PT_ERR_INVALID)
        w, h = self.size
        out = np.empty((h, w) if ch == 1 else (h, w, ch), np.int32 if k == capi.PT_AOV_PRIM else np.float32)
        check(self.lib.pt_aov_download(self.h, k, out.ctypes.data, out.nbytes), "pt_aov_download")
        return out

    def denoise(self, source="accum", scale: float = 1.0, download: bool = True, **options):
        """pt_denoise: the a-trous filter over source * scale, guided by the G-buffer.  source:
        "accum" (the sum buffer; scale = 1 / spp gives the mean), "display" (the progressive view),
        "adaptive" (the per-pixel mean of the last render_adaptive()) or an (H, W, 3) array.  options: fields of pt_denoise_options (iterations, demodulate,
        sigma_color, sigma_normal, sigma_position, albedo_floor); the rest keep their defaults.
        Returns the (H, W, 3) result; download=False leaves it on the device (pt_denoised_device_ptr,
        asynchronous) and returns None."""
        o = capi.pt_denoise_options()
        o.struct_size = C.sizeof(o)
        check(self.lib.pt_denoise_options_default(C.byref(o)), "pt_denoise_options_default")
        for k, v in options.items():
            if k == "struct_size" or k not in dict(capi.pt_denoise_options._fields_):
                raise capi.PTError(f"denoise: no such option {k!r}", capi.PT_ERR_INVALID)
            setattr(o, k, v)
        w, h = self.size
        host = None
        if isinstance(source, str):
            srcs = {"accum": capi.PT_DENOISE_SRC_ACCUM, "display": capi.PT_DENOISE_SRC_DISPLAY,
                    "adaptive": capi.PT_DENOISE_SRC_ADAPTIVE}
            if source not in srcs:
                raise capi.PTError(f"denoise: source must be 'accum', 'display', 'adaptive' or an array, not {source!r}",
                                   capi.PT_ERR_INVALID)
            src = srcs[source]
        else:
            host = _f32(source)
            if host.size != w * h * 3:
                raise capi.PTError("denoise: the source array must hold H * W * 3 floats", capi.PT_ERR_INVALID)
            src = capi.PT_DENOISE_SRC_HOST
        out = np.empty((h, w, 3), np.float32) if download else None
        check(self.lib.pt_denoise(self.h, src, fptr(host) if host is not None else None, float(scale), C.byref(o),
                                  fptr(out) if download else None), "pt_denoise")
        return out

    def denoise_info(self) -> dict:
        """pt_get_denoise_info: iterations and filter_ms of the last denoise(), gbuffer_renders since
        the renderer was created, hit_pixels and gbuffer_ms of the G-buffer in force."""
        s = capi.pt_denoise_info()
        s.struct_size = C.sizeof(s)
        check(self.lib.pt_get_denoise_info(self.h, C.byref(s)), "pt_get_denoise_info")
        return {k: getattr(s, k) for k, _ in capi.pt_denoise_info._fields_ if k != "struct_size"}

    def denoise_temporal(self, source="accum", scale: float = 1.0, download: bool = True, **options):
        """pt_denoise_temporal: denoise() with the previous call's filtered colour, luminance moments
        and history length reprojected through the previous call's camera, and a colour term scaled
        by the estimated variance.  options: fields of pt_temporal_options (alpha,
        alpha_moments, max_history, normal_cos, plane_distance, sigma_luminance, variance_history,
        motion_vectors) or of pt_denoise_options (sigma_color is not used).  This call's view and state
        become the history of the next one."""
        t, o = capi.pt_temporal_options(), capi.pt_denoise_options()
        t.struct_size, o.struct_size = C.sizeof(t), C.sizeof(o)
        check(self.lib.pt_temporal_options_default(C.byref(t)), "pt_temporal_options_default")
        check(self.lib.pt_denoise_options_default(C.byref(o)), "pt_denoise_options_default")
        for k, v in options.items():
            if k != "struct_size" and k in dict(capi.pt_temporal_options._fields_):
                setattr(t, k, v)
            elif k != "struct_size" and k in dict(capi.pt_denoise_options._fields_):
                setattr(o, k, v)
            else:
                raise capi.PTError(f"denoise_temporal: no such option {k!r}", capi.PT_ERR_INVALID)
        w, h = self.size
        host = None
        if isinstance(source, str):
            srcs = {"accum": capi.PT_DENOISE_SRC_ACCUM, "display": capi.PT_DENOISE_SRC_DISPLAY,
                    "adaptive": capi.PT_DENOISE_SRC_ADAPTIVE}
            if source not in srcs:
                raise capi.PTError(f"denoise_temporal: source must be 'accum', 'display', 'adaptive' or an array, not {source!r}",
                                   capi.PT_ERR_INVALID)
            src = srcs[source]
        else:
            host = _f32(source)
            if host.size != w * h * 3:
                raise capi.PTError("denoise_temporal: the source array must hold H * W * 3 floats", capi.PT_ERR_INVALID)
            src = capi.PT_DENOISE_SRC_HOST
        out = np.empty((h, w, 3), np.float32) if download else None
        check(self.lib.pt_denoise_temporal(self.h, src, fptr(host) if host is not None else None, float(scale),
                                           C.byref(t), C.byref(o), fptr(out) if download else None), "pt_denoise_temporal")
        return out

    def temporal_reset(self) -> None:
        """pt_temporal_reset: the next denoise_temporal() starts every pixel again."""
        check(self.lib.pt_temporal_reset(self.h), "pt_temporal_reset")

    def temporal_state(self, kind) -> np.ndarray:
        """pt_temporal_download: state of the last denoise_temporal(), by name (capi.TEMPORAL_KINDS)
        or PT_TEMPORAL_* value: (H, W) for history_length and variance, (H, W, 2) moments, (H, W, 3)
        color."""
        k = capi.TEMPORAL_KINDS[kind] if isinstance(kind, str) else int(kind)
        ch = int(self.lib.pt_temporal_channels(k))
        if ch < 0:
            raise capi.PTError(f"temporal_state: no such kind {kind!r}", capi.PT_ERR_INVALID)
        w, h = self.size
        out = np.empty((h, w) if ch == 1 else (h, w, ch), np.float32)
        check(self.lib.pt_temporal_download(self.h, k, out.ctypes.data, out.nbytes), "pt_temporal_download")
        return out

    def motion(self, kind) -> np.ndarray:
        """pt_motion_download, by name (capi.MOTION_KINDS) or PT_MOTION_* value: (H, W, 2) barycentric
        (u, v of the G-buffer in force), and of the last denoise_temporal(motion_vectors=1) the
        (H, W, 3) prev_position and screen (the reprojected point's offset in pixels | 1)."""
        k = capi.MOTION_KINDS[kind] if isinstance(kind, str) else int(kind)
        ch = int(self.lib.pt_motion_channels(k))
        if ch < 0:
            raise capi.PTError(f"motion: no such kind {kind!r}", capi.PT_ERR_INVALID)
        w, h = self.size
        out = np.empty((h, w, ch), np.float32)
        check(self.lib.pt_motion_download(self.h, k, out.ctypes.data, out.nbytes), "pt_motion_download")
        return out

    def temporal_info(self) -> dict:
        """pt_get_temporal_info: calls, history_valid, and of the last denoise_temporal() the
        reprojected, reset and moved hit pixels, whether the motion kernel ran, and the device times
        of its three stages and of its vertex snapshot."""
        s = capi.pt_temporal_info()
        s.struct_size = C.sizeof(s)
        check(self.lib.pt_get_temporal_info(self.h, C.byref(s)), "pt_get_temporal_info")
        return {k: getattr(s, k) for k, _ in capi.pt_temporal_info._fields_ if k != "struct_size"}

    # -- adaptive sampling ------------------------------------------------------------------------
    def render_adaptive(self, first_frame_id: int = 1, download: bool = True, **options):
        """pt_render_adaptive: clears the sum, then renders rounds of round_frames frames from
        first_frame_id on, each only for the pixels of the 8x8 tiles whose mean relative standard
        error is still above threshold.  options: fields of pt_adaptive_options
        (threshold, min_samples, max_samples, round_frames, luminance_floor); the rest keep their
        defaults.  Returns the (H, W, 3) per-pixel mean; download=False leaves it on the device
        (pt_adaptive_mean_device_ptr) and returns None.  Synchronous."""
        o = capi.pt_adaptive_options()
        o.struct_size = C.sizeof(o)
        check(self.lib.pt_adaptive_options_default(C.byref(o)), "pt_adaptive_options_default")
        for k, v in options.items():
            if k == "struct_size" or k not in dict(capi.pt_adaptive_options._fields_):
                raise capi.PTError(f"render_adaptive: no such option {k!r}", capi.PT_ERR_INVALID)
            setattr(o, k, v)
        w, h = self.size
        out = np.empty((h, w, 3), np.float32) if download else None
        check(self.lib.pt_render_adaptive(self.h, int(first_frame_id), C.byref(o), fptr(out) if download else None),
              "pt_render_adaptive")
        return out

    def adaptive_state(self, kind) -> np.ndarray:
        """pt_adaptive_download: state of the last render_adaptive(), by name (capi.ADAPTIVE_KINDS) or
        PT_ADAPTIVE_* value: (H, W) uint32 samples, (H, W) float32 error, (H, W, 2) float64 moments
        (S1, S2), and per tile (rows of tiles from the bottom) float32 tile_error and int32
        tile_rounds."""
        k = capi.ADAPTIVE_KINDS[kind] if isinstance(kind, str) else int(kind)
        ch = int(self.lib.pt_adaptive_channels(k))
        if ch < 0:
            raise capi.PTError(f"adaptive_state: no such kind {kind!r}", capi.PT_ERR_INVALID)
        w, h = self.size
        t = capi.PT_ADAPTIVE_TILE
        shape, dtype = {
            capi.PT_ADAPTIVE_SAMPLES: ((h, w), np.uint32),
            capi.PT_ADAPTIVE_ERROR: ((h, w), np.float32),
            capi.PT_ADAPTIVE_MOMENTS: ((h, w, 2), np.float64),
            capi.PT_ADAPTIVE_TILE_ERROR: (((h + t - 1) // t, (w + t - 1) // t), np.float32),
            capi.PT_ADAPTIVE_TILE_ROUNDS: (((h + t - 1) // t, (w + t - 1) // t), np.int32),
        }[k]
        out = np.empty(shape, dtype)
        check(self.lib.pt_adaptive_download(self.h, k, out.ctypes.data, out.nbytes), "pt_adaptive_download")
        return out

    def adaptive_info(self) -> dict:
        """pt_get_adaptive_info: of the last render_adaptive() the rounds, tiles and tiles_stopped (by
        the threshold), the samples spent and what the largest count costs on every pixel
        (samples_uniform), the wall time of the rounds and the device time of the estimates."""
        s = capi.pt_adaptive_info()
        s.struct_size = C.sizeof(s)
        check(self.lib.pt_get_adaptive_info(self.h, C.byref(s)), "pt_get_adaptive_info")
        return {k: getattr(s, k) for k, _ in capi.pt_adaptive_info._fields_ if k != "struct_size"}

    # -- anti-aliasing ------------------------------------------------------------------------------
    def set_pixel_filter(self, supersample: int = 1, kind="box", radius: float = 0.0, param: float = 0.0) -> None:
        """pt_set_pixel_filter: frame F samples sub-pixel cell F mod supersample^2 of
        every pixel (supersample 1, 2, 4 or 8), and the frames are accumulated through the pixel
        filter `kind` ("box", "tent", "gaussian", "mitchell" or a PT_FILTER_* value); radius and
        param 0 take the kind's defaults.  Without arguments: the default, pixel centres and the box.
        The sum is not cleared."""
        f = _pixel_filter(supersample, kind, radius, param, "set_pixel_filter")
        check(self.lib.pt_set_pixel_filter(self.h, C.byref(f)), "pt_set_pixel_filter")

    def pixel_filter(self) -> dict:
        """pt_get_pixel_filter: supersample, kind (by name), and the radius and param in use."""
        f = capi.pt_pixel_filter()
        f.struct_size = C.sizeof(f)
        check(self.lib.pt_get_pixel_filter(self.h, C.byref(f)), "pt_get_pixel_filter")
        names = {v: k for k, v in capi.FILTER_KINDS.items()}
        return {"supersample": f.supersample, "kind": names[f.kind], "radius": f.radius, "param": f.param}

    def accum_clear(self) -> None:
        check(self.lib.pt_accum_clear(self.h), "pt_accum_clear")

    def render_frames(self, first_frame_id: int, n_frames: int) -> None:
        check(self.lib.pt_render_frames(self.h, int(first_frame_id), int(n_frames)), "pt_render_frames")

    def set_primary_dedup(self, enable: bool) -> None:
        check(self.lib.pt_set_primary_dedup(self.h, 1 if enable else 0), "pt_set_primary_dedup")

    def set_wavefront_streams(self, streams: int) -> None:
        check(self.lib.pt_set_wavefront_streams(self.h, int(streams)), "pt_set_wavefront_streams")

    def set_band_split(self, enable: bool) -> None:
        """One-frame calls: two row bands on two wavefront streams (pt_set_band_split, default on)."""
        check(self.lib.pt_set_band_split(self.h, 1 if enable else 0), "pt_set_band_split")

    def set_lit_table(self, enable: bool | None) -> None:
        """pt_set_lit_table: NEE answers from the (light, cell) lit table instead of shadow rays where
        the table proves the light unoccluded; None = auto (the default), images bit-identical."""
        check(self.lib.pt_set_lit_table(self.h, -1 if enable is None else (1 if enable else 0)), "pt_set_lit_table")

    def lit_table(self):
        """(info dict, tri_words (triangles,) uint32, bits (lights, words_per_light) uint32) of the lit
        table for the current lights (pt_lit_table_download); (info, None, None) while it is off."""
        info = capi.pt_lit_table_info()
        check(self.lib.pt_lit_table_download(self.h, C.byref(info), None, 0, None, 0), "pt_lit_table_download")
        d = {k: getattr(info, k) for k, _ in capi.pt_lit_table_info._fields_}
        if not info.active:
            return d, None, None
        tri = np.zeros(info.triangles, np.uint32)
        bits = np.zeros((info.lights, info.words_per_light), np.uint32)
        check(self.lib.pt_lit_table_download(self.h, C.byref(info), tri.ctypes.data, tri.nbytes, bits.ctypes.data,
                                             bits.nbytes), "pt_lit_table_download")
        return d, tri, bits

    def set_occluder_table(self, enable: bool | None) -> None:
        """pt_set_occluder_table: before a shadow ray is emitted, test the cell's occluder candidate
        with the tracer's arithmetic and drop the ray on a hit; None = auto (the default), images
        bit-identical.  Needs the lit table in use."""
        check(self.lib.pt_set_occluder_table(self.h, -1 if enable is None else (1 if enable else 0)),
              "pt_set_occluder_table")

    def occluder_table(self):
        """The occluder candidates for the current lights, (lights * cells,) int32 laid out
        light * cells + cell: -1 or a leaf-order triangle (pt_occluder_table_download); None while the
        table is not in use."""
        n = C.c_int64(0)
        check(self.lib.pt_occluder_table_download(self.h, C.byref(n), None, 0), "pt_occluder_table_download")
        if n.value == 0:
            return None
        e = np.zeros(n.value, np.int32)
        check(self.lib.pt_occluder_table_download(self.h, C.byref(n), e.ctypes.data, e.nbytes), "pt_occluder_table_download")
        return e

    def set_skip_table(self, enable: bool | None) -> None:
        """pt_set_skip_table: extension rays drop the BVH subtree that lies behind the surface they
        leave (bit-identical images).  None = automatic (the default), False / True force it."""
        check(self.lib.pt_set_skip_table(self.h, -1 if enable is None else (1 if enable else 0)), "pt_set_skip_table")

    def skip_table(self):
        """Tests: the skip words, shape (triangles, 2): 0 or a BVH4 child link per side of the stored
        winding (pt_skip_table_download); None while the table is not in use."""
        n = C.c_int64(0)
        check(self.lib.pt_skip_table_download(self.h, C.byref(n), None, 0), "pt_skip_table_download")
        if n.value == 0:
            return None
        w = np.empty(n.value, np.uint32)
        check(self.lib.pt_skip_table_download(self.h, C.byref(n), w.ctypes.data, w.nbytes), "pt_skip_table_download")
        return w.reshape(-1, 2)

    def upload_occluder_table(self, entries) -> None:
        """pt_occluder_table_upload: replace the candidates until the next rebuild; every entry must be
        -1 or a triangle index of the scene."""
        e = np.ascontiguousarray(entries, np.int32)
        check(self.lib.pt_occluder_table_upload(self.h, e.ctypes.data, e.nbytes), "pt_occluder_table_upload")

    def render_accumulate(self, spp: int, first_frame_id: int = 1) -> np.ndarray:
        """Clear, render frame ids first_frame_id .. +spp-1 and return the mean image
        (pt_render_accumulate); the sum stays in the device accumulator."""
        w, h = self.size
        out = np.empty((h, w, 3), np.float32)
        check(self.lib.pt_render_accumulate(self.h, int(spp), int(first_frame_id), fptr(out)),
              "pt_render_accumulate")
        return out

    def set_accum_device_buffer(self, ptr: int | None) -> None:
        check(self.lib.pt_set_accum_device_buffer(self.h, C.c_void_p(ptr) if ptr else None),
              "pt_set_accum_device_buffer")

    def accum(self, scale: float = 1.0) -> np.ndarray:
        w, h = self.size
        out = np.empty((h, w, 3), np.float32)
        check(self.lib.pt_accum_download(self.h, fptr(out), float(scale)), "pt_accum_download")
        return out

    def set_accum_fp64(self, enable: bool) -> None:
        """pt_set_accum_fp64: add the samples in fp64 (accum() then returns the fp64 sum rounded
        to fp32, accum64() the fp64 sum); off by default (the reference sums in fp32)."""
        check(self.lib.pt_set_accum_fp64(self.h, 1 if enable else 0), "pt_set_accum_fp64")

    def accum64(self) -> np.ndarray:
        w, h = self.size
        out = np.empty((h, w, 3), np.float64)
        check(self.lib.pt_accum_download64(self.h, out.ctypes.data_as(C.POINTER(C.c_double))), "pt_accum_download64")
        return out

    def synchronize(self) -> None:
        check(self.lib.pt_synchronize(self.h), "pt_synchronize")

    def stream(self) -> int:
        return int(self.lib.pt_stream(self.h) or 0)

    @property
    def frame_id(self) -> int:
        return int(self.lib.pt_frame_id(self.h))

    @frame_id.setter
    def frame_id(self, v: int) -> None:
        check(self.lib.pt_set_frame_id(self.h, int(v)), "pt_set_frame_id")

    def stats(self) -> dict:
        s = capi.pt_stats()
        check(self.lib.pt_get_stats(self.h, C.byref(s)), "pt_get_stats")
        return {k: getattr(s, k) for k, _ in capi.pt_stats._fields_}

    def stats_reset(self) -> None:
        check(self.lib.pt_stats_reset(self.h), "pt_stats_reset")

    def trace_rays(self, rays: np.ndarray, any_hit: bool = False):
        """rays: (n, 8) float32 = origin, dir, tmin, tmax -> (prim, t, u, v, backface)."""
        r = _f32(rays).reshape(-1, 8)
        n = len(r)
        prim = np.empty(n, np.int32)
        t, u, v = (np.empty(n, np.float32) for _ in range(3))
        back = np.empty(n, np.int32)
        check(self.lib.pt_trace_rays(self.h, fptr(r), n, prim.ctypes.data_as(C.POINTER(C.c_int32)), fptr(t),
                                     fptr(u), fptr(v), back.ctypes.data_as(C.POINTER(C.c_int32)),
                                     1 if any_hit else 0), "pt_trace_rays")
        return prim, t, u, v, back

    def set_debug_pixel(self, x: int, y: int, frame_id: int) -> None:
        """Record the per-bounce surface of pixel (x, y)'s path at frame_id (pt_set_debug_pixel;
        the reference's isDebugRay, devicePrograms.cu:637-644).  x < 0 turns it off."""
        check(self.lib.pt_set_debug_pixel(self.h, int(x), int(y), int(frame_id)), "pt_set_debug_pixel")

    def debug_path(self) -> list:
        """The recorded bounces as dicts of pt_debug_bounce fields."""
        recs = (capi.pt_debug_bounce * 64)()
        n = C.c_int32()
        check(self.lib.pt_get_debug_path(self.h, recs, 64, C.byref(n)), "pt_get_debug_path")
        out = []
        for k in range(n.value):
            r = recs[k]
            out.append({f: (list(getattr(r, f)) if isinstance(getattr(r, f), C.Array) else getattr(r, f))
                        for f, _ in capi.pt_debug_bounce._fields_})
        return out

    def devices(self) -> list:
        """Device ordinals this renderer drives (pt_devices)."""
        n = int(self.lib.pt_device_count(self.h))
        out = (C.c_int32 * max(1, n))()
        check(self.lib.pt_devices(self.h, out, n), "pt_devices")
        return [int(out[i]) for i in range(n)]

    def bvh_arrays(self):
        """(nodes, triangles): the BVH4 node array as (bvh_nodes, 32) uint32 words and the
        leaf-ordered triangle records as (triangles, 12) uint32 words (pt_bvh_download)."""
        st = self.stats()
        nodes = np.zeros((st["bvh_nodes"], 32), np.uint32)
        tris = np.zeros((st["triangles"], 12), np.uint32)
        check(self.lib.pt_bvh_download(self.h, nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes),
              "pt_bvh_download")
        return nodes, tris

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.pt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pixel_filter(supersample, kind, radius, param, what: str) -> "capi.pt_pixel_filter":
    if isinstance(kind, str) and kind not in capi.FILTER_KINDS:
        raise capi.PTError(f"{what}: kind must be one of {sorted(capi.FILTER_KINDS)}, not {kind!r}", capi.PT_ERR_INVALID)
    f = capi.pt_pixel_filter()
    f.struct_size = C.sizeof(f)
    f.supersample = int(supersample)
    f.kind = capi.FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
    f.radius = float(radius)
    f.param = float(param)
    return f


def pixel_filter_cells(supersample: int) -> np.ndarray:
    """pt_pixel_filter_cells: (supersample^2, 2) int32, the sub-pixel cell (sx, sy) of every cell
    index c = frame id mod supersample^2.  Host only."""
    s = int(supersample)
    out = np.zeros((max(1, s * s), 2), np.int32)
    check(capi.load().pt_pixel_filter_cells(s, capi.iptr(out)), "pt_pixel_filter_cells")
    return out


def pixel_filter_taps(supersample: int = 1, kind="box", radius: float = 0.0, param: float = 0.0, cell: int = 0):
    """pt_pixel_filter_taps: (R, wx, wy) of one cell index, the 2 R + 1 float32 weights along x and
    along y exactly as the device reads them.  Host only."""
    f = _pixel_filter(supersample, kind, radius, param, "pixel_filter_taps")
    R = C.c_int32(0)
    wx, wy = np.zeros(5, np.float32), np.zeros(5, np.float32)
    check(capi.load().pt_pixel_filter_taps(C.byref(f), int(cell), C.byref(R), fptr(wx), fptr(wy)), "pt_pixel_filter_taps")
    k = 2 * R.value + 1
    return R.value, wx[:k].copy(), wy[:k].copy()


def setup_renderer(scene: Scene, width: int, height: int, max_bounces: int, device: int = 0,
                   kernel: int = capi.PT_KERNEL_AUTO, bvh_builder: int = capi.PT_BVH_AUTO,
                   devices=None) -> OptixRenderer:
    """The reference's main.cpp:95-113 sequence: construct, Resize, SetLights, SetMaxBounces, SetCamera."""
    r = OptixRenderer(None, scene, device=device, kernel=kernel, bvh_builder=bvh_builder, devices=devices)
    r.Resize((width, height))
    r.SetLights(scene.lights)
    r.SetMaxBounces(max_bounces)
    r.SetCameraBlender(scene.camera_blender_pos, scene.camera_blender_rot, scene.fov_deg)
    return r
