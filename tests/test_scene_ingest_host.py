"""Host checks of the part of pt_create that reads the caller's memory (pt_capi_bake.cpp:
ingest_scene, GeomHost::normal_mode, bake_scene).  tests/scene_ingest_check.cpp is compiled
host-only with pt_capi_bake.cpp, which calls no HIP runtime function, and checks on scenes of 0, 1
and 3 meshes (a dozen triangles at most; one mesh without normals, one without vertices, one
textured):

- rejections: the status, the message, and that no output is written, for a negative count, an
  index equal to n_vertices, a texture id equal to n_textures and a mesh with triangles but no
  index array;
- normal_mode: 0 without normals; 1 for the identity, a signed axis permutation and a pure
  translation; 2 for a 45 degree rotation and a non-uniform scale with rotation;
- the bake under matrices whose products and sums are exact in fp32 (signed permutations, integer
  translations, vertices of small integers and halves): world positions, the three w tags, the
  normals (object space for a mode-2 mesh) and the centroid bounds equal the exact values.

The images these records give are checked on the GPU (test_gpu_parity.py, test_gpu_bitexact.py,
test_gpu_geometry_update.py)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "optixpathtracer_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("ingest") / "scene_ingest_check"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{CSRC}",
                    str(ROOT / "tests" / "scene_ingest_check.cpp"), str(CSRC / "pt_capi_bake.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    return exe


@pytest.mark.parametrize("what,at_least", [("rejections", 50), ("normal_mode", 30), ("bake", 150)])
def test_scene_ingest(checker, what, at_least):
    rc = subprocess.run([str(checker), what], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 0, rc.stdout + rc.stderr
    m = re.search(r"checks=(\d+) bad=(\d+)", rc.stdout)
    assert m and int(m.group(2)) == 0, rc.stdout
    assert int(m.group(1)) >= at_least  # the cases ran
