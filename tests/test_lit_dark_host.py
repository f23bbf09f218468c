"""Host check of the lit table's single-triangle cover predicate and per-cell margin
(optixpathtracer_amd/csrc/pt_lit.h lit_tri_covers, lit_margin_cell): tests/lit_dark_check.cpp is
compiled as plain C++ (no device code) and checks that

  * wherever the predicate says "covered", every shadow ray of the cell -- thousands per case, from
    random points, the corners and border points moved one ulp outward -- is a hit for an fp32
    replica of the tracer's tri_test + tri_accept;
  * a bundle straddling an edge, a triangle behind the light, one without clearance at either end,
    grazing incidence below the |cos| bound, degenerate triangles and a light within the margin of
    the surface are refused;
  * the per-cell margin never exceeds lit_margin(diag) and never falls below the derived bound,
    cells at a box's far corners included.

The predicate is what tools/lit_cover_probe.cpp measures coverage with (profiles/lit_cover_probe.json);
the table on the GPU holds lit bits only.  The second test runs the same program under
AddressSanitizer and UBSan as a stand-alone host binary."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "optixpathtracer_amd" / "csrc"


def host_compiler():
    """Any C++17 compiler: the header is plain C++ without __HIPCC__."""
    for name in ("c++", "g++", "clang++", "hipcc", "/opt/rocm/bin/hipcc"):
        path = shutil.which(name)
        if path:
            return path
    return None


def _build(tmp_path, name, extra):
    cxx = host_compiler()
    assert cxx, "no C++ compiler found (c++, g++, clang++ or hipcc)"
    exe = tmp_path / name
    rc = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-x", "c++", f"-I{CSRC}",
                         str(ROOT / "tests" / "lit_dark_check.cpp"), "-o", str(exe)], capture_output=True, text=True,
                        timeout=300)
    return exe, rc


def _run(exe):
    rc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert rc.returncode == 0, rc.stdout + rc.stderr
    out = json.loads(rc.stdout)
    assert out["bad"] == 0
    assert out["covered"] >= 400 and out["rays"] > 400 * 2000  # not vacuous
    assert out["refusals"] == 10 and out["margins"] > 20000
    return out


def test_cover_predicate_and_cell_margin(tmp_path):
    exe, rc = _build(tmp_path, "lit_dark_check", [])
    assert rc.returncode == 0, rc.stderr
    print(_run(exe))


def test_cover_predicate_under_sanitizers(tmp_path):
    exe, rc = _build(tmp_path, "lit_dark_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if rc.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime: " + rc.stderr[-200:])
    _run(exe)
