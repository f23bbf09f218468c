"""What the first-hit G-buffer and the a-trous denoiser cost, beside one frame of path tracing.

For the sphere box (about 35k triangles) and sponza_class (about 250k) at 1920x1080, a 4-spp sum is
accumulated once and one JSON line per scene is printed (each figure the median of `--reps` calls
after a warm-up call, with min and max):

  gbuffer_ms            pt_denoise_info.gbuffer_ms (HIP events around k_gbuffer) of a call after a
                        camera nudge, which makes the cached G-buffer stale
  filter_ms             pt_denoise_info.filter_ms (HIP events around the pack pass and the iterations)
                        at 1 .. `--iterations` iterations, for the plain global-load build of the
                        iterations (plain) and with the iterations of a step up to 2 (lds2), 4
                        (lds4) or 16 (lds16) staging their tile in LDS (PTAMD_DENOISE_LDS = 0, 2,
                        4, 16), the variants alternating call by call
  per_iteration_ms      differences of those medians: iteration i alone (iteration 0 with the pack pass)
  floor_ms_per_iteration  64 B per pixel (48 B of colour and guide records read, 16 B written) at the
                        6.29 TB/s a float4 copy reaches on this GPU
  denoise_wall_ms       wall time of one pt_denoise from the accumulator at the defaults, left on
                        the device (then pt_synchronize) and downloaded to the host
  render_wall_ms        wall time of one one-frame pt_render in the same process, for scale
  temporal              pt_denoise_temporal at the defaults: temporal_ms, variance_ms,
                        filter_ms (pt_temporal_info) and the wall time of a call left on the device, for
                        the first call after a reset, a call from the same view as the one before (the
                        fifth in a row: every history is past variance_history), and a call after a
                        camera nudge; beside them pt_denoise's filter_ms, measured in the same rounds
                        (each round: pt_denoise, reset + call, four static calls, nudge + call)
  motion                motion vectors (pt_temporal_options.motion_vectors): a call after a committed
                        move of mesh 0 with the option on and with it off -- temporal_ms, the wall time
                        of the call left on the device (with the G-buffer render the commit causes),
                        moved_pixels, and for the option on snapshot_ms, the copy of the scene's
                        vertices that ends the call (each round, per setting: reset, two static calls,
                        move + commit + call; the settings alternate)

No pass/fail bar.  The lines also go to `--out` (default profiles/denoise_bench.json).

With `--ab-lib OTHER.so` a first line compares pt_denoise's filter_ms, the G-buffer's gbuffer_ms and
the device time of a static pt_denoise_temporal call (temporal_ms + variance_ms + filter_ms, the
options at their defaults) on the sphere box between this build and another build of the library,
e.g. the parent commit's: `--ab-rounds` rounds, in each a fresh process per build, one after the
other on the same GPU.

  python tools/denoise_bench.py [--reps 9] [--iterations 5] [--size 1920x1080] [--out FILE]
                                [--ab-lib OTHER.so] [--ab-rounds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from optixpathtracer_amd import scenes  # noqa: E402
from optixpathtracer_amd.renderer import setup_renderer  # noqa: E402

COPY_TBS = 6.29  # measured float4 copy rate of the MI355X's HBM
FLOOR_BYTES = 64  # per pixel and iteration: three 16-byte records read, one written


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def filter_ms(r, lds: int, iterations: int) -> float:
    os.environ["PTAMD_DENOISE_LDS"] = str(lds)
    r.denoise("accum", 0.25, download=False, iterations=iterations)
    return r.denoise_info()["filter_ms"]


def temporal_rows(r, sc, reps):
    """The temporal filter's three cases and pt_denoise, alternating round by round."""
    base = np.asarray(sc.camera_blender_pos, np.float32)
    keys = ("temporal_ms", "variance_ms", "filter_ms")
    rows = {c: {k: [] for k in keys + ("wall_ms",)} for c in ("after_reset", "static", "after_nudge")}
    spatial, counts = [], {}

    def call(case, keep):
        wall = wall_ms(lambda: (r.denoise_temporal("accum", 0.25, download=False), r.synchronize()))
        info = r.temporal_info()
        if keep:
            for k in keys:
                rows[case][k].append(info[k])
            rows[case]["wall_ms"].append(wall)
            counts[case] = {"reprojected_pixels": info["reprojected_pixels"], "reset_pixels": info["reset_pixels"]}

    for k in range(reps + 1):
        r.denoise("accum", 0.25, download=False)
        if k:
            spatial.append(r.denoise_info()["filter_ms"])
        r.temporal_reset()
        call("after_reset", k)
        for j in range(4):
            call("static", k and j == 3)
        r.SetCameraBlender(base + np.float32([1e-3 * (1 - k % 2), 0.0, 0.0]), sc.camera_blender_rot, sc.fov_deg)
        call("after_nudge", k)
    out = {c: {k: spread(v) for k, v in rows[c].items()} | counts[c] for c in rows}
    out["denoise_filter_ms"] = spread(spatial)
    return out


def motion_rows(r, reps):
    """A call after a committed mesh move, with motion vectors on and off, alternating round by round."""
    keys = ("temporal_ms", "snapshot_ms")
    rows = {c: {k: [] for k in keys + ("wall_ms",)} for c in ("on", "off")}
    counts = {}
    model = np.eye(4, dtype=np.float32)
    for k in range(reps + 1):
        for case in ("on", "off"):
            opt = 1 if case == "on" else 0
            r.temporal_reset()
            for _ in range(2):
                r.denoise_temporal("accum", 0.25, download=False, motion_vectors=opt)
            model[0, 3] = 1e-3 * (1 + k % 2)
            r.set_mesh_transform(0, model.T.ravel())
            r.commit_geometry("refit")
            wall = wall_ms(lambda: (r.denoise_temporal("accum", 0.25, download=False, motion_vectors=opt), r.synchronize()))
            info = r.temporal_info()
            assert info["motion_used"] == opt
            if k:
                for key in keys:
                    rows[case][key].append(info[key])
                rows[case]["wall_ms"].append(wall)
                counts[case] = {q: info[q] for q in ("moved_pixels", "reprojected_pixels", "reset_pixels", "motion_used")}
    return {c: {k: spread(v) for k, v in rows[c].items()} | counts[c] for c in rows}


AB_KEYS = ("filter_ms", "gbuffer_ms", "temporal_total_ms")


def filter_only(w, h, depth, reps):
    """One process of the A/B, on the sphere box at the defaults: pt_denoise's filter_ms, gbuffer_ms of
    a call after a camera nudge, and the device time of a static pt_denoise_temporal call."""
    sc = scenes.sphere_in_box("diffuse")
    r = setup_renderer(sc, w, h, depth)
    r.accum_clear()
    r.render_frames(1, 4)
    base = np.asarray(sc.camera_blender_pos, np.float32)
    ms = {k: [] for k in AB_KEYS}
    for k in range(reps + 1):
        r.SetCameraBlender(base + np.float32([1e-3 * (k % 2), 0.0, 0.0]), sc.camera_blender_rot, sc.fov_deg)
        r.denoise("accum", 0.25, download=False)
        info = r.denoise_info()
        ms["filter_ms"].append(info["filter_ms"])
        ms["gbuffer_ms"].append(info["gbuffer_ms"])
        for _ in range(3):
            r.denoise_temporal("accum", 0.25, download=False)
        t = r.temporal_info()
        ms["temporal_total_ms"].append(t["temporal_ms"] + t["variance_ms"] + t["filter_ms"])
    r.close()
    print(json.dumps({k: spread(v[1:]) for k, v in ms.items()}), flush=True)


def ab(other, a):
    """pt_denoise's filter_ms of this build (a) against `other` (b), a fresh process each, alternating."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--filter-only", "--size", a.size, "--reps", str(a.reps),
           "--depth", str(a.depth)]
    res = {"a": [], "b": []}
    for _ in range(a.ab_rounds):
        for side in ("a", "b"):
            env = dict(os.environ)
            env.pop("PTAMD_LIB", None)
            if side == "b":
                env["PTAMD_LIB"] = str(other)
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True)
            res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
    out = {"ab": "pt_denoise filter_ms, gbuffer_ms and a static pt_denoise_temporal call, sphere_box_diffuse, defaults",
           "size": a.size, "reps": a.reps, "rounds": a.ab_rounds, "a": "this build", "b": Path(other).name + " (the other build)"}
    for side in ("a", "b"):
        out[f"{side}_rounds"] = res[side]
    for key in AB_KEYS:
        med = {side: statistics.median(x[key]["median"] for x in res[side]) for side in ("a", "b")}
        out[key] = {"a_median_of_medians": med["a"], "b_median_of_medians": med["b"], "a_over_b": med["a"] / med["b"]}
    line = json.dumps(out)
    print(line, flush=True)
    return line


def run(name, sc, w, h, depth, reps, iterations):
    r = setup_renderer(sc, w, h, depth)
    r.accum_clear()
    r.render_frames(1, 4)
    r.synchronize()
    out = {"scene": name, "size": f"{w}x{h}", "triangles": r.stats()["triangles"], "reps": reps}

    # the G-buffer: every call after a camera nudge renders it again
    base = np.asarray(sc.camera_blender_pos, np.float32)
    g = []
    for k in range(reps + 1):
        r.SetCameraBlender(base + np.float32([1e-3 * (k % 2), 0.0, 0.0]), sc.camera_blender_rot, sc.fov_deg)
        r.denoise("accum", 0.25, download=False)
        g.append(r.denoise_info()["gbuffer_ms"])
    info = r.denoise_info()
    assert info["gbuffer_renders"] == reps + 1
    out["gbuffer_ms"] = spread(g[1:])
    out["hit_pixels"] = info["hit_pixels"]

    # the filter, plain against LDS-staged small steps (up to step 2, 4 or 16), alternating
    variants = {"plain": 0, "lds2": 2, "lds4": 4, "lds16": 16}
    ms = {v: {n: [] for n in range(1, iterations + 1)} for v in variants}
    for n in range(1, iterations + 1):
        for k in range(reps + 1):
            for v, lds in variants.items():
                t = filter_ms(r, lds, n)
                if k:
                    ms[v][n].append(t)
    same = {}
    for v, lds in variants.items():
        os.environ["PTAMD_DENOISE_LDS"] = str(lds)
        same[v] = r.denoise("accum", 0.25, iterations=iterations)
    out["variants_identical"] = all(bool((same["plain"].view(np.uint32) == same[v].view(np.uint32)).all()) for v in variants)
    floor = w * h * FLOOR_BYTES / (COPY_TBS * 1e12) * 1e3
    out["floor_ms_per_iteration"] = floor
    for v in variants:
        med = [statistics.median(ms[v][n]) for n in range(1, iterations + 1)]
        per = [med[0]] + [med[n] - med[n - 1] for n in range(1, iterations)]
        out[f"filter_ms_{v}"] = {str(n): spread(ms[v][n]) for n in range(1, iterations + 1)}
        out[f"per_iteration_ms_{v}"] = per
    os.environ.pop("PTAMD_DENOISE_LDS", None)  # the library's default build from here on

    dev, host = [], []
    for k in range(reps + 1):
        dev.append(wall_ms(lambda: (r.denoise("accum", 0.25, download=False), r.synchronize())))
        host.append(wall_ms(lambda: r.denoise("accum", 0.25)))
    out["denoise_wall_ms"] = {"device": spread(dev[1:]), "downloaded": spread(host[1:])}
    out["filter_ms_default"] = r.denoise_info()["filter_ms"]

    out["temporal"] = temporal_rows(r, sc, reps)
    r.SetCameraBlender(sc.camera_blender_pos, sc.camera_blender_rot, sc.fov_deg)
    out["motion"] = motion_rows(r, reps)

    r.set_render_ahead(1)  # every call renders its own frame
    img = np.empty((h, w, 3), np.float32)
    rw = [wall_ms(lambda: r.Render(img)) for _ in range(reps + 1)]
    out["render_wall_ms"] = spread(rw[1:])
    r.close()
    line = json.dumps(out)
    print(line, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise_bench.json"))
    ap.add_argument("--ab-lib", default=None, help="another build of libptamd.so to compare pt_denoise's filter_ms with")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--filter-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    if a.filter_only:
        return filter_only(w, h, a.depth, a.reps)
    head = [ab(a.ab_lib, a)] if a.ab_lib else []  # first: this process has not touched the GPU yet
    lines = head + [run("sphere_box_diffuse", scenes.sphere_in_box("diffuse"), w, h, a.depth, a.reps, a.iterations),
                    run("sponza_class", scenes.sponza_class(), w, h, a.depth, a.reps, a.iterations)]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
