"""Lit-table probe (DESIGN.md §4 "The lit table"): counters, kernel times and the one-frame pt_launch loop.

    python tools/lit_table_probe.py counters sphere_box_diffuse sponza_class > profiles/lit_table_counters.jsonl
    python tools/lit_table_probe.py launch sphere_box_diffuse > profiles/lit_table_launch_loop.jsonl

counters: per scene and table setting (off, lit table on, lit and occluder table on) at 1920x1080, depth 8, one 128-frame launch: a
  pass with per-kernel event timing and a pass with the traversal counters, as one JSON line.
  bvh_build_ms is each renderer's own pt_create; the first renderer of a process also pays the
  runtime's first-launch costs there, so later rows show the shorter, steady figure.
launch: ms per call of a loop of one-frame pt_launch calls (device colour buffer and device light
  array, as the reference's optixLaunch loop) with the table off, auto and forced on.
PTAMD_LIB selects another build of the library (a parent build without the table reports "n/a").
"""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from optixpathtracer_amd import scenes  # noqa: E402
from optixpathtracer_amd.renderer import camera_from_blender, setup_renderer  # noqa: E402

W, H, DEPTH = 1920, 1080, 8
KEYS = ["segments", "shadow_rays", "pair_kernel_shadow_rays", "nee_unoccluded", "lit_table_answers", "lit_table_cells",
        "lit_table_bits_set", "lit_table_bytes", "lit_table_build_ms", "bvh_build_ms", "pair_kernel_ms",
        "pair_kernel_launches", "shade_kernel_ms", "shade_kernel_launches", "trace_kernel_ms", "trace_kernel_launches",
        "total_render_ms", "triangles", "occluder_table_answers", "occluder_table_candidates", "occluder_table_bytes",
        "occluder_table_build_ms"]


def has_table(r) -> bool:
    return hasattr(r.lib, "pt_set_lit_table")


def counters(names):
    for name in names:
        sc = scenes.make_scene(name)
        for lit, occ in ((False, False), (True, False), (True, True)):
            r = setup_renderer(sc, W, H, DEPTH)
            r.set_lit_table(lit)
            if hasattr(r.lib, "pt_set_occluder_table"):
                r.set_occluder_table(occ)
            elif occ:
                continue
            r.accum_clear()
            r.render_frames(1, 128)  # warm-up (allocations)
            r.synchronize()
            out = {"scene": name, "lit_table": lit, "occluder_table": occ}
            for what in ("timing", "counts"):
                r.stats_reset()
                r.set_kernel_timing(what == "timing")
                r.set_traversal_stats(what == "counts")
                r.render_frames(129, 128)
                st = r.stats()
                out[what] = {k: st[k] for k in KEYS if k in st}
            r.close()
            print(json.dumps(out), flush=True)


def launch_loop(names, calls=200):
    hip = C.CDLL("libamdhip64.so.7")
    for name in names:
        sc = scenes.make_scene(name)
        r = setup_renderer(sc, W, H, DEPTH)
        p, iv, ip = camera_from_blender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg, W, H)
        lights = np.ascontiguousarray(sc.lights, np.float32)
        d_lights, d_img = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_lights), C.c_size_t(lights.nbytes)) == 0
        assert hip.hipMalloc(C.byref(d_img), C.c_size_t(W * H * 3 * 4)) == 0
        assert hip.hipMemcpy(d_lights, lights.ctypes.data_as(C.c_void_p), C.c_size_t(lights.nbytes), 1) == 0
        for setting in ("off", "auto", "on"):
            if has_table(r):
                r.set_lit_table({"off": False, "auto": None, "on": True}[setting])
            elif setting != "off":
                continue
            ms = []
            for rep in range(4):  # the first repetition warms up
                r.synchronize()
                t0 = time.perf_counter()
                for k in range(calls):
                    r.launch(d_img.value, (W, H), 1 + k, p, iv, ip, d_lights.value, len(lights), DEPTH)
                r.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / calls)
            print(json.dumps({"scene": name, "lit_table": setting if has_table(r) else "n/a", "calls": calls,
                              "ms_per_pt_launch": [round(x, 4) for x in ms[1:]]}), flush=True)
        hip.hipFree(d_lights)
        hip.hipFree(d_img)
        r.close()


if __name__ == "__main__":
    {"counters": counters, "launch": launch_loop}[sys.argv[1]](sys.argv[2:])
