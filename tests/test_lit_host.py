"""Host check of the lit table's cell index and plane predicates (optixpathtracer_amd/csrc/pt_lit.h):
tests/lit_host_check.cpp is compiled as plain C++ (no device code) and checks that every level has
N^2 distinct unit cells, that (u, v) on and around the cell borders lands in the exact cell or one
sharing that border, and the rejection predicates on a hand-made floor cell.  The table's bits are
checked against the tracer on the GPU (test_gpu_lit_table.py)."""
import json
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "optixpathtracer_amd" / "csrc"


def host_compiler():
    """Any C++17 compiler: the header is plain C++ without __HIPCC__."""
    for name in ("c++", "g++", "clang++", "hipcc", "/opt/rocm/bin/hipcc"):
        path = shutil.which(name)
        if path:
            return path
    return None


def test_cell_index_and_predicates(tmp_path):
    cxx = host_compiler()
    assert cxx, "no C++ compiler found (c++, g++, clang++ or hipcc)"
    exe = tmp_path / "lit_host_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-x", "c++", f"-I{CSRC}", str(ROOT / "tests" / "lit_host_check.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    rc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert rc.returncode == 0, rc.stdout + rc.stderr
    out = json.loads(rc.stdout)
    assert out["bad"] == 0
    # 4^0 + ... + 4^8 cells, and several border probes around each checked grid point
    assert out["checked"] > sum(4 ** k for k in range(9))
