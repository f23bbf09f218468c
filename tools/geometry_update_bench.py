"""What a geometry commit costs, beside the path it replaces (pt_destroy + pt_create).

For the sphere box (about 35k triangles) and sponza_class (about 250k) one mesh is moved and one
JSON line per scene is printed:

  refit_ms / rebuild_ms   pt_stats.geometry_commit_ms of pt_commit_geometry (device time), median of
                          `--reps` commits, with min and max, and the commit's wall time
  create_build_ms         pt_stats.bvh_build_ms of a fresh pt_create on the moved scene
  destroy_create_wall_ms  wall time of close() + a new renderer set up the same way
  sah_ratio_refit         bvh_sah_cost / bvh_sah_cost_built after the refit (1.0 after a rebuild)
  msamples_refit / _rebuilt   a render (`--frames` frames, one pt_render_frames call after a warm-up
                          call) on the tree refitted from the unmoved scene's build and on the tree
                          rebuilt for the moved scene, alternating `--render-reps` times: median, min, max

No pass/fail bar: the numbers are what a caller needs to choose between refit and rebuild.

  python tools/geometry_update_bench.py [--reps 5] [--render-reps 3] [--frames 64] [--size 1920x1080]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from optixpathtracer_amd import scenes  # noqa: E402
from optixpathtracer_amd.renderer import setup_renderer  # noqa: E402


def translation(t) -> np.ndarray:
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = t
    return np.ascontiguousarray(m.T.ravel())  # column-major


def msamples(r, w, h, frames, depth):
    r.accum_clear()
    r.render_frames(1, frames)  # warm-up: queues, lit table
    r.synchronize()
    r.stats_reset()
    r.accum_clear()
    t0 = time.perf_counter()
    r.render_frames(1, frames)
    r.synchronize()
    wall = time.perf_counter() - t0
    return w * h * frames / wall / 1e6, r.accum()


def commits(r, mesh, moves, how, reps):
    dev, wall = [], []
    for k in range(reps):
        r.set_mesh_transform(mesh, moves[k % len(moves)])
        t0 = time.perf_counter()
        r.commit_geometry(how)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(r.stats()["geometry_commit_ms"])
    return {"median": statistics.median(dev), "min": min(dev), "max": max(dev), "wall_median": statistics.median(wall)}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, sc, mesh, w, h, frames, depth, reps, render_reps):
    # the commits alternate between the two positions and end on the moved one
    moves = [translation([0.0, 0.0, 0.0]), translation([0.3, 0.15, -0.2])]
    if reps % 2:
        moves.reverse()
    final = moves[(reps - 1) % 2]
    moved = dataclasses.replace(sc, meshes=[dataclasses.replace(m, model=final) if i == mesh else m
                                            for i, m in enumerate(sc.meshes)])
    r = setup_renderer(sc, w, h, depth)
    st0 = r.stats()
    refit = commits(r, mesh, moves, "refit", reps)
    st = r.stats()
    rebuild = commits(r, mesh, moves, "rebuild", reps)
    ms_refit, ms_rebuilt = [], []
    for _ in range(render_reps):  # the two trees in turn, on the same renderer
        r.set_mesh_transform(mesh, translation([0.0, 0.0, 0.0]))
        r.commit_geometry("rebuild")  # the unmoved scene's tree ...
        r.set_mesh_transform(mesh, final)
        r.commit_geometry("refit")  # ... refitted to the move
        v, img_refit = msamples(r, w, h, frames, depth)
        ms_refit.append(v)
        r.set_mesh_transform(mesh, final)
        r.commit_geometry("rebuild")
        v, img_rebuilt = msamples(r, w, h, frames, depth)
        ms_rebuilt.append(v)
    t0 = time.perf_counter()
    r.close()
    f = setup_renderer(moved, w, h, depth)
    f.synchronize()
    recreate = (time.perf_counter() - t0) * 1e3
    stf = f.stats()
    _, img_fresh = msamples(f, w, h, frames, depth)
    f.close()
    print(json.dumps({
        "scene": name, "triangles": st0["triangles"], "bvh_nodes": st0["bvh_nodes"], "bvh_depth": st0["bvh_depth"],
        "moved_mesh": sc.meshes[mesh].name or mesh, "moved_triangles": sc.meshes[mesh].n_triangles,
        "refit_ms": refit, "rebuild_ms": rebuild, "create_build_ms": stf["bvh_build_ms"],
        "destroy_create_wall_ms": recreate,
        "sah_ratio_refit": st["bvh_sah_cost"] / st["bvh_sah_cost_built"], "sah_cost_built": st["bvh_sah_cost_built"],
        "msamples_refit": spread(ms_refit), "msamples_rebuilt": spread(ms_rebuilt), "render": f"{w}x{h} x{frames} depth {depth}",
        "images_identical": bool((img_refit == img_fresh).all() and (img_rebuilt == img_fresh).all()),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--render-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--depth", type=int, default=8)
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    box = scenes.sphere_in_box("diffuse")
    run("sphere_box_diffuse", box, 14, w, h, a.frames, a.depth, a.reps, a.render_reps)  # one of the 36 spheres
    sp = scenes.sponza_class()
    order = sorted(range(len(sp.meshes)), key=lambda i: sp.meshes[i].n_triangles)
    run("sponza_class", sp, order[len(order) // 2], w, h, a.frames, a.depth, a.reps, a.render_reps)  # a mesh of median size


if __name__ == "__main__":
    main()
