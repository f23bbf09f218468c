"""The geometry-update surface without a GPU: the three entry points are declared in
include/ptamd.h and bound in capi.py, the ctypes pt_stats mirror has the size the C compiler
gives the header's struct, and the C++ facade's new methods compile and link."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "ptamd.h"
NEW = ("pt_set_mesh_transform", "pt_set_mesh_vertices", "pt_commit_geometry")


def test_entry_points_declared_and_bound(ptlib):
    from optixpathtracer_amd import capi

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(\s*pt_renderer\s*\*", text), name
        res, args = capi.SIGNATURES[name]
        fn = getattr(ptlib, name)
        assert fn.restype is res is C.c_int
        assert list(fn.argtypes) == args and args[0] is C.c_void_p
    assert re.search(r"#define\s+PT_GEOM_REFIT\s+0\b", text) and capi.PT_GEOM_REFIT == 0
    assert re.search(r"#define\s+PT_GEOM_REBUILD\s+1\b", text) and capi.PT_GEOM_REBUILD == 1
    # NULL renderers are refused, with a message
    ident = (C.c_float * 16)(*[1.0 if i % 5 == 0 else 0.0 for i in range(16)])
    assert ptlib.pt_set_mesh_transform(None, 0, ident) == capi.PT_ERR_INVALID
    assert ptlib.pt_set_mesh_vertices(None, 0, ident, None) == capi.PT_ERR_INVALID
    assert ptlib.pt_commit_geometry(None, capi.PT_GEOM_REFIT) == capi.PT_ERR_INVALID
    assert b"NULL" in ptlib.pt_last_error()


def test_stats_mirror_has_the_header_size(tmp_path):
    from optixpathtracer_amd import capi

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "ptamd.h"\nint main(void) { printf("%zu", sizeof(pt_stats)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert int(out) == C.sizeof(capi.pt_stats)
    names = [f for f, _ in capi.pt_stats._fields_]
    assert names[-6:] == ["geometry_commits", "geometry_refits", "geometry_rebuilds", "geometry_commit_ms",
                          "bvh_sah_cost", "bvh_sah_cost_built"]
    # the mirror lists the header's fields in the header's order
    body = re.search(r"typedef struct pt_stats \{(.*?)\} pt_stats;", HEADER.read_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+);", body) == names


def _build(tmp_path):
    from optixpathtracer_amd import capi

    exe = tmp_path / "facade_geometry"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "facade_geometry_check.cpp"), f"-L{capi.LIB_PATH.parent}", "-lptamd",
                    f"-Wl,-rpath,{capi.LIB_PATH.parent}", "-o", str(exe)], check=True)
    return exe


def test_cpp_facade_geometry_methods_compile_and_fail_loudly_without_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode in (0, 2), rc.stdout + rc.stderr
    if rc.returncode == 2:
        assert "no HIP device" in rc.stdout


@pytest.mark.gpu
def test_cpp_facade_geometry_methods_run_on_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout + rc.stderr
