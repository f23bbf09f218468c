#!/usr/bin/env python3
"""What anti-aliasing (pt_set_pixel_filter) costs and buys.

    python tools/pixel_filter_bench.py [--scene sphere_box_diffuse] [--frames 128] [--spp 16,64]

For one scene at 1920x1080 it prints JSON lines:

  (a) "cost"     one call of `--frames` frames (best of `--reps`, left on the device) with the filter
                 off and under supersample 4 with the box: the second gives up the primary dedup and
                 the bounce-0 visibility table, so the ratio is what sub-pixel sampling costs
  (b) "accum"    the same call at 0 bounces, where a batch is only k_camera and the accumulate kernel,
                 for the box and each wider filter at supersample 4: ms per batch, and what the
                 filtered accumulate adds over the plain one
  (c) "quality"  MSE and FLIP (pt_image_mse, pt_image_flip) of the mean after `--spp` frames against a
                 supersample 8, `--ref-spp` reference, for off, supersample 4 box and supersample 4 tent

No pass/fail bar.  The lines also go to `--out` (default profiles/pixel_filter_bench.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sphere_box_diffuse")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--spp", default="16,64")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pixel_filter_bench.json"))
    a = ap.parse_args()
    import torch  # before libptamd holds the device

    dev = torch.cuda.get_device_properties(0).name
    from optixpathtracer_amd import capi, scenes
    from optixpathtracer_amd.capi import fptr
    from optixpathtracer_amd.renderer import setup_renderer

    lib = capi.load()
    sc = scenes.make_scene(a.scene)
    w, h, n = a.width, a.height, a.frames
    r = setup_renderer(sc, w, h, a.depth)
    lines = [{"device": dev, "scene": a.scene, "tris": sc.n_triangles, "size": [w, h], "depth": a.depth, "frames": n,
              "ref_spp": a.ref_spp}]
    print(json.dumps(lines[0]), flush=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    def timed(first):
        r.accum_clear()
        r.render_frames(first, n)  # warm: queues allocated, tables built
        best = None
        for k in range(a.reps):
            r.accum_clear()
            r.synchronize()
            t = time.perf_counter()
            r.render_frames(first, n)
            r.synchronize()
            ms = (time.perf_counter() - t) * 1e3
            best = ms if best is None else min(best, ms)
        return best

    settings = [("off", 1, "box"), ("box4", 4, "box"), ("tent4", 4, "tent"), ("gaussian4", 4, "gaussian"),
                ("mitchell4", 4, "mitchell")]
    # (a) the dedup given up
    cost = {}
    for name, s, kind in settings[:2]:
        r.set_pixel_filter(s, kind)
        cost[name] = timed(1)
    emit({"what": "cost", "ms": {k: round(v, 2) for k, v in cost.items()},
          "msamples_per_s": {k: round(w * h * n / v / 1e3, 1) for k, v in cost.items()},
          "box4_over_off": round(cost["box4"] / cost["off"], 4)})
    # (b) the accumulate kernels alone: no bounces, so a batch is k_camera and the accumulate
    r.SetMaxBounces(0)
    acc = {}
    for name, s, kind in settings:
        r.set_pixel_filter(s, kind)
        acc[name] = timed(1)
    r.SetMaxBounces(a.depth)
    batches = -(-n // max(1, r.stats()["last_batch_frames"]))
    emit({"what": "accum", "ms_per_call_at_0_bounces": {k: round(v, 3) for k, v in acc.items()},
          "filtered_minus_box4_ms": {k: round(acc[k] - acc["box4"], 3) for k in ("tent4", "gaussian4", "mitchell4")},
          "batches_per_call": batches})
    # (c) quality at equal spp
    r.set_pixel_filter(8, "box")
    t0 = time.perf_counter()
    ref = np.ascontiguousarray(r.render_accumulate(a.ref_spp, first_frame_id=1_000_001), np.float32)
    ref_s = time.perf_counter() - t0
    for spp in [int(v) for v in a.spp.split(",")]:
        for name, s, kind in (settings[0], settings[1], settings[2]):
            r.set_pixel_filter(s, kind)
            img = np.ascontiguousarray(r.render_accumulate(spp, first_frame_id=1), np.float32)
            mse = float(lib.pt_image_mse(fptr(img), fptr(ref), w * h))
            flip = float(lib.pt_image_flip(fptr(ref), fptr(img), w, h, C.c_float(0.0), None))
            emit({"what": "quality", "setting": name, "spp": spp, "mse": mse, "flip": round(flip, 5),
                  "ref_s": round(ref_s, 2)})
    r.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
