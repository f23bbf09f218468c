#!/usr/bin/env python3
"""What adaptive sampling (pt_render_adaptive) buys over a uniform sample count.

    python tools/adaptive_bench.py [--scene sphere_box_diffuse] [--thresholds 0.1,0.05,0.03]

For one scene at 1920x1080 a reference of `--ref-spp` samples per pixel is rendered once (frame ids
far from the ones compared), then a uniform render is stepped up round by round to max_samples with
its MSE against the reference after every step, and for every threshold one JSON line is printed:

  samples / samples_uniform   what the adaptive call spent, against W * H * its largest count
  mse                         of its mean against the reference
  wall_ms                     of the call left on the device (best of `--reps`)
  equal_mse_spp               the smallest uniform count (a multiple of the round) whose MSE is no larger
  uniform_wall_ms             pt_render_accumulate at that count, left on the device (best of `--reps`)
  estimate_ms_per_round       HIP-event time of the error, compaction and resolve kernels per round
  active_fraction             per round, the share of the image's pixels it rendered
  round_ms                    wall_ms / rounds

No pass/fail bar.  The lines also go to `--out` (default profiles/adaptive_bench.json).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
TILE = 8


def mse(a, ref):
    d = np.nan_to_num(a.astype(np.float64) - ref, nan=0.0)
    return float(np.mean(d * d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sphere_box_diffuse")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--thresholds", default="0.1,0.05,0.03")
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--max-samples", type=int, default=256)
    ap.add_argument("--round-frames", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adaptive_bench.json"))
    a = ap.parse_args()
    import torch  # before libptamd holds the device

    dev = torch.cuda.get_device_properties(0).name
    from optixpathtracer_amd import scenes
    from optixpathtracer_amd.renderer import setup_renderer

    sc = scenes.make_scene(a.scene)
    w, h, R = a.width, a.height, a.round_frames
    r = setup_renderer(sc, w, h, a.depth)
    t0 = time.perf_counter()
    ref = r.render_accumulate(a.ref_spp, first_frame_id=1_000_001).astype(np.float64)
    ref_s = time.perf_counter() - t0
    # the uniform render, stepped: MSE after every round's worth of frames
    r.accum_clear()
    uniform = []
    for k in range(a.max_samples // R):
        r.render_frames(1 + k * R, R)
        uniform.append(((k + 1) * R, mse(r.accum(1.0 / ((k + 1) * R)), ref)))

    def timed(call):
        best = None
        for _ in range(a.reps):
            r.synchronize()
            t = time.perf_counter()
            call()
            r.synchronize()
            ms = (time.perf_counter() - t) * 1e3
            best = ms if best is None else min(best, ms)
        return best

    uniform_ms = {}
    tiles_y, tiles_x = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    ys = np.minimum(TILE, h - TILE * np.arange(tiles_y))
    xs = np.minimum(TILE, w - TILE * np.arange(tiles_x))
    tile_pixels = ys[:, None] * xs[None, :]
    lines = [{"device": dev, "scene": a.scene, "tris": sc.n_triangles, "size": [w, h], "depth": a.depth,
              "round_frames": R, "min_samples": a.min_samples, "max_samples": a.max_samples, "ref_spp": a.ref_spp,
              "ref_s": round(ref_s, 2), "uniform_mse": {str(s): m for s, m in uniform}}]
    print(json.dumps(lines[0]), flush=True)
    for thr in [float(t) for t in a.thresholds.split(",")]:
        opt = dict(threshold=thr, min_samples=a.min_samples, max_samples=a.max_samples, round_frames=R)
        wall = timed(lambda: r.render_adaptive(1, download=False, **opt))
        mean = r.render_adaptive(1, **opt)
        info = r.adaptive_info()
        rounds = r.adaptive_state("tile_rounds")
        m = mse(mean, ref)
        equal = next((s for s, um in uniform if um <= m), None)
        if equal is not None and equal not in uniform_ms:
            uniform_ms[equal] = timed(lambda: (r.accum_clear(), r.render_frames(1, equal)))
        active = [float((tile_pixels * (rounds > k)).sum()) / (w * h) for k in range(info["rounds"])]
        line = {"scene": a.scene, "threshold": thr, "samples": info["samples"], "samples_uniform": info["samples_uniform"],
                "samples_share": round(info["samples"] / max(1, info["samples_uniform"]), 4), "mse": m,
                "wall_ms": round(wall, 2), "equal_mse_spp": equal,
                "uniform_wall_ms": round(uniform_ms[equal], 2) if equal is not None else None,
                "rounds": info["rounds"], "tiles_stopped": info["tiles_stopped"], "tiles": info["tiles"],
                "estimate_ms_per_round": round(info["estimate_ms"] / max(1, info["rounds"]), 4),
                "round_ms": round(wall / max(1, info["rounds"]), 3), "active_fraction": [round(x, 4) for x in active]}
        lines.append(line)
        print(json.dumps(line), flush=True)
    r.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
