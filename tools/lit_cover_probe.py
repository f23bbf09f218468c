"""Coverage probe of the lit table's proofs on the host (tools/lit_cover_probe.cpp, no GPU).

    python tools/lit_cover_probe.py sphere_box_diffuse sponza_class > profiles/lit_cover_probe.json

Exports each scene's world triangles and lights, builds the probe as plain C++ and runs it for the
cell fractions 0.005, 0.0035 and 0.0025 (kLitCellFraction and the two candidates of DESIGN.md §4).
The output is one JSON object: scene -> list of per-fraction results.
"""
import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from optixpathtracer_amd import scenes  # noqa: E402

FRACTIONS = ["0.005", "0.0035", "0.0025"]


def world_tris(sc) -> np.ndarray:
    parts = []
    for m in sc.meshes:
        M = np.asarray(m.model, np.float32).reshape(4, 4, order="F")
        v = (np.c_[m.vertices, np.ones(len(m.vertices), np.float32)] @ M.T).astype(np.float32)
        parts.append(v[m.indices.reshape(-1), :3].reshape(-1, 3, 3))
    return np.concatenate(parts).astype(np.float32)


def main(names):
    cxx = next((p for p in map(shutil.which, ("c++", "g++", "clang++", "hipcc")) if p), None)
    assert cxx, "no C++ compiler found"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "lit_cover_probe"
        subprocess.run([cxx, "-O2", "-std=c++17", "-pthread", "-x", "c++", f"-I{ROOT / 'optixpathtracer_amd' / 'csrc'}",
                        str(ROOT / "tools" / "lit_cover_probe.cpp"), "-o", str(exe)], check=True)
        for name in names:
            sc = scenes.make_scene(name)
            tris = world_tris(sc)
            lights = np.ascontiguousarray(np.asarray(sc.lights, np.float32)[:, :3])
            path = Path(tmp) / f"{name}.bin"
            with open(path, "wb") as f:
                f.write(np.array([len(tris), len(lights)], np.int32).tobytes())
                f.write(tris.tobytes())
                f.write(lights.tobytes())
            rc = subprocess.run([str(exe), str(path), *FRACTIONS], capture_output=True, text=True, check=True)
            out[name] = [json.loads(line) for line in rc.stdout.splitlines()]
            print(f"{name}: done", file=sys.stderr)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:] or ["sphere_box_diffuse", "sponza_class"])
