"""Host check of the skip table's builder (optixpathtracer_amd/csrc/pt_skip.h): tests/skip_host_check.cpp
is compiled host-only with the SAH builder of pt_sah.cpp, collapses its binary tree into a BVH4 in the
tracer's node layout and checks skip_word for every (triangle, side) of a tetrahedron, a cube, an 8x4
UV sphere, two such spheres 0.07 apart, a concave L-prism, one planar quad and a soup of 200 random
triangles by brute force in fp64: the named link is on the triangle's path, every triangle under it is
at or below the plane + kLitDelta and passes the predicate, no higher path link would pass, and "none"
only where nothing passes.  On the convex scenes no outward side may be "none".  Four floor scenes -- a
planar floor of 4608 or 18432 triangles under one sphere, with and without a sliver -- take one walk past
kSkipMaxTris triangles: every word stays safe against brute force and no lower than the highest passing
link with fewer than kSkipMaxTris triangles under it, and without a sliver the floor's downward sides
name a child of the root.  The second test runs the same stand-alone program under AddressSanitizer and
UBSan.  The words the GPU builds are compared with a numpy restatement word for word
(test_gpu_skip_words.py, skip_ref.py) and held to bit-identical images (test_gpu_skip_table.py)."""
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
    # the floor scenes: 2 * quads^2 floor triangles, a 48-triangle sphere, one sliver; every stride-th checked
    floors = {"floor": (4608 + 48, 1), "floor_sliver": (4608 + 48 + 1, 1), "wide_floor": (18432 + 48, 31),
              "wide_floor_sliver": (18432 + 48 + 1, 31)}
    assert {k: out[k]["triangles"] for k in tris} == tris
    assert {k: out[k]["triangles"] for k in floors} == {k: n for k, (n, _) in floors.items()}
    for k, (n, stride) in floors.items():
        assert out[k]["checked"] == 2 * len(range(0, n, stride))
        assert out[k]["down"] > 0  # one downward side per floor triangle checked
    assert out["checked"] == 2 * sum(tris.values()) + sum(out[k]["checked"] for k in floors)
    # without a sliver box_accept spends no budget: every downward side of the floor names a child of the
    # root, although more than kSkipMaxTris = 4096 triangles lie under that side (wide_floor: under the link)
    for k in ("floor", "wide_floor"):
        assert out[k]["down_root_child"] == out[k]["down"] and out[k]["kept_low"] == 0
    assert out["floor"]["down"] == 4608
    # with one, every triangle is looked at.  4657 triangles spread over the root's children stay within the
    # budget (no link on a path has 4096 under it); 4608 under one child do not, and the words stop below
    # what brute force allows (never unsafe, never lower than the budget explains: "bad" counts both)
    assert out["floor_sliver"]["down"] == 4608
    assert out["wide_floor_sliver"]["down_root_child"] == 0
    assert out["wide_floor_sliver"]["kept_low"] >= out["wide_floor_sliver"]["down"] > 0
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
