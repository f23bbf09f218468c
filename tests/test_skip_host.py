"""Host check of the skip table's builder (optixpathtracer_amd/csrc/pt_skip.h): tests/skip_host_check.cpp
is compiled host-only with the SAH builder of pt_sah.cpp, collapses its binary tree into a BVH4 in the
tracer's node layout and checks skip_word for every (triangle, side) of a tetrahedron, a cube, an 8x4
UV sphere, two such spheres 0.07 apart, a concave L-prism, one planar quad and a soup of 200 random
triangles by brute force in fp64: the named link is on the triangle's path, every triangle under it is
at or below the plane + kLitDelta and passes the predicate, no higher path link would pass, and "none"
only where nothing passes.  On the convex scenes no outward side may be "none".  The second test runs the
same stand-alone program under AddressSanitizer and UBSan.  The words the GPU builds are checked through
the images and the traversal counters (test_gpu_skip_table.py)."""
import json
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "optixpathtracer_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    rc = subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-x", "hip", "--cuda-host-only",
                         f"-I{CSRC}", str(ROOT / "tests" / "skip_host_check.cpp"), str(CSRC / "pt_sah.cpp"), "-o",
                         str(exe)], capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr
    return exe


def _run(exe):
    rc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert rc.returncode == 0, rc.stdout + rc.stderr
    out = json.loads(rc.stdout)
    print(out)
    assert out["bad"] == 0
    tris = {"tetrahedron": 4, "cube": 12, "sphere": 48, "two_spheres": 96, "l_prism": 24, "quad": 2, "soup": 200}
    assert {k: out[k]["triangles"] for k in tris} == tris
    assert out["checked"] == 2 * sum(tris.values())
    # not vacuous: the convex scenes name a link for every outward side, and most words overall are links
    for k in ("tetrahedron", "cube", "sphere"):
        assert out[k]["none_outward"] == 0
    assert out["quad"]["none"] == 0  # both sides of a planar mesh drop the whole mesh
    for k in ("tetrahedron", "cube", "sphere", "two_spheres", "l_prism"):
        assert out[k]["none"] <= tris[k]  # a closed mesh: at most the inward sides
    assert 0 < out["soup"]["none"] < 2 * tris["soup"]  # the soup has both kinds
    return out


def test_skip_words_against_brute_force(tmp_path):
    _run(_build(tmp_path, "skip_host_check", []))


def test_skip_words_under_sanitizers(tmp_path):
    _run(_build(tmp_path, "skip_host_check_san",
                ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]))
