"""Skip-table probe (DESIGN.md §4 "The skip table"): traversal counters, kernel times, the table's size and
build time, and a digest of the accumulator per setting.

    python tools/skip_table_probe.py sphere_box_diffuse sponza_class:1 > profiles/skip_table_counters.jsonl

"scene:mode" renders a scene in another material mode than its own (the atrium's Default mode has no skip
code; mode 1 = Lambert builds and uses the table on its geometry).  Per scene and table setting (off, on; "n/a" for a library without the table) at 1920x1080, depth 8, one
128-frame batch: a pass with per-kernel event timing and a pass with the traversal counters, as one JSON
line.  nodes_per_ray / tri_tests_per_ray are the counters over the rays the statistics kernels traced;
accum_sha256 is the digest of the accumulator after the counted batch, equal across the settings when the
table changes no sample.  PTAMD_LIB selects another build of the library; run from a checkout of the
parent commit the script reports that tree's figures as "n/a" rows.
"""
import hashlib
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from optixpathtracer_amd import scenes  # noqa: E402
from optixpathtracer_amd.renderer import OptixRenderer, setup_renderer  # noqa: E402

W, H, DEPTH, FRAMES = 1920, 1080, 8, 128
KEYS = ["segments", "rays", "nodes_visited", "tri_tests", "shadow_rays", "skip_table_rays", "skip_table_bytes",
        "skip_table_build_ms", "lit_table_build_ms", "occluder_table_build_ms", "bvh_build_ms", "pair_kernel_ms",
        "pair_kernel_launches", "shade_kernel_ms", "shade_kernel_launches", "trace_kernel_ms", "total_render_ms",
        "triangles", "bvh_nodes"]


def probe(names):
    for arg in names:
        name, _, mode = arg.partition(":")  # "scene:mode" renders the scene in that material mode
        sc = scenes.make_scene(name)
        has = hasattr(OptixRenderer, "set_skip_table")
        for setting in (("off", "on") if has else ("n/a",)):
            r = setup_renderer(sc, W, H, DEPTH)
            if mode:
                r.set_material_mode(int(mode))
            if has:
                r.set_skip_table(setting == "on")
            r.accum_clear()
            r.render_frames(1, FRAMES)  # warm-up (allocations)
            r.synchronize()
            out = {"scene": name, "skip_table": setting, "material_mode": int(mode) if mode else int(sc.material_mode)}
            for what in ("timing", "counts"):
                r.stats_reset()
                r.accum_clear()
                r.set_kernel_timing(what == "timing")
                r.set_traversal_stats(what == "counts")
                r.render_frames(1 + FRAMES, FRAMES)
                st = r.stats()
                out[what] = {k: st[k] for k in KEYS if k in st}
                out["accum_sha256_" + what] = hashlib.sha256(r.accum().tobytes()).hexdigest()
            c = out["counts"]
            out["nodes_per_ray"] = c["nodes_visited"] / max(1, c["rays"])
            out["tri_tests_per_ray"] = c["tri_tests"] / max(1, c["rays"])
            r.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    probe(sys.argv[1:])
