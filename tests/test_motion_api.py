"""The motion-vector surface without a GPU: pt_motion_channels and pt_motion_download are declared
in include/ptamd.h and bound in capi.py with matching signatures, the grown structs' ctypes mirrors
have the sizes and field names the C compiler gives the header's, a caller compiled against the
shorter pt_temporal_options keeps motion_vectors at its default, NULL and unknown kinds are refused
with a message, and the C++ facade's Motion method compiles and links."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "ptamd.h"
NEW = {"pt_motion_channels": "int", "pt_motion_download": "int"}
CONSTANTS = {"PT_MOTION_BARYCENTRIC": 0, "PT_MOTION_PREV_POSITION": 1, "PT_MOTION_SCREEN": 2}
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}


def _header():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _ctype(decl: str):
    decl = decl.strip()
    if "*" in decl:
        base = decl.replace("const", "").split("*")[0].strip()
        assert base in ("pt_renderer", "void"), decl
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_entry_points_and_constants_declared_and_bound(ptlib):
    from optixpathtracer_amd import capi

    text = _header()
    for name, ret in NEW.items():
        m = re.search(rf"([\w ]+?\*?)\s*\b{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert m.group(1).strip() == ret, (name, m.group(1))
        res, args = capi.SIGNATURES[name]
        fn = getattr(ptlib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        assert res is C.c_int
        assert args == [_ctype(p) for p in m.group(2).split(",")], name
    for name, value in CONSTANTS.items():
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
        assert getattr(capi, name) == value
    assert capi.MOTION_KINDS == {"barycentric": 0, "prev_position": 1, "screen": 2}
    assert [ptlib.pt_motion_channels(k) for k in range(3)] == [2, 3, 3]
    assert ptlib.pt_motion_channels(3) < 0 and ptlib.pt_motion_channels(-1) < 0
    # a family of its own: the AOV and temporal kinds are what they were
    assert sorted(capi.AOV_KINDS.values()) == list(range(7)) and ptlib.pt_aov_channels(7) < 0
    assert sorted(capi.TEMPORAL_KINDS.values()) == list(range(4)) and ptlib.pt_temporal_channels(4) < 0


def test_struct_mirrors_have_the_header_sizes(tmp_path):
    from optixpathtracer_amd import capi

    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptamd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu", sizeof(pt_temporal_options), sizeof(pt_temporal_info),\n'
                   '    offsetof(pt_temporal_options, motion_vectors), offsetof(pt_temporal_info, filter_ms),\n'
                   '    offsetof(pt_temporal_info, moved_pixels), offsetof(pt_temporal_info, snapshot_ms),\n'
                   '    offsetof(pt_temporal_info, motion_used)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    o, i = capi.pt_temporal_options, capi.pt_temporal_info
    assert out == [C.sizeof(o), C.sizeof(i), o.motion_vectors.offset, i.filter_ms.offset, i.moved_pixels.offset,
                   i.snapshot_ms.offset, i.motion_used.offset]
    # trailing fields: what a caller compiled against the previous header has keeps its offsets
    assert o.motion_vectors.offset == o.variance_history.offset + 4 == C.sizeof(o) - 4
    assert i.moved_pixels.offset == i.filter_ms.offset + 8
    for cls in (o, i):
        body = re.search(rf"typedef struct {cls.__name__} \{{(.*?)\}} {cls.__name__};", _header(), flags=re.S).group(1)
        names = [f for f, _ in cls._fields_]
        assert re.findall(r"\b(\w+);", body) == names and names[0] == "struct_size"
    assert [f for f, _ in o._fields_][-1] == "motion_vectors"
    assert [f for f, _ in i._fields_][-4:-1] == ["moved_pixels", "snapshot_ms", "motion_used"]


def test_shorter_struct_size_leaves_motion_vectors_alone(ptlib):
    from optixpathtracer_amd import capi

    o = capi.pt_temporal_options()
    o.struct_size = C.sizeof(o)
    o.motion_vectors = 7
    assert ptlib.pt_temporal_options_default(C.byref(o)) == capi.PT_OK
    assert o.motion_vectors == 0 and o.variance_history == 4  # off by default

    class Guarded(C.Structure):
        _fields_ = [("o", capi.pt_temporal_options), ("guard", C.c_uint8 * 16)]

    # a caller compiled before the field existed: everything up to variance_history
    short = capi.pt_temporal_options.motion_vectors.offset
    g = Guarded()
    C.memset(C.byref(g), 0xAB, C.sizeof(g))
    g.o.struct_size = short
    assert ptlib.pt_temporal_options_default(C.byref(g.o)) == capi.PT_OK
    assert (g.o.struct_size, g.o.variance_history) == (short, 4)
    assert bytes(g)[short:] == b"\xab" * (C.sizeof(g) - short)  # motion_vectors and the guard are untouched
    # the info struct: a refused call writes nothing past the size field of a shorter caller's struct
    class GuardedInfo(C.Structure):
        _fields_ = [("i", capi.pt_temporal_info), ("guard", C.c_uint8 * 16)]

    gi = GuardedInfo()
    C.memset(C.byref(gi), 0xAB, C.sizeof(gi))
    gi.i.struct_size = capi.pt_temporal_info.moved_pixels.offset
    assert ptlib.pt_get_temporal_info(None, C.byref(gi.i)) == capi.PT_ERR_INVALID
    assert bytes(gi)[4:] == b"\xab" * (C.sizeof(gi) - 4)


def test_null_and_bad_kinds_are_refused_with_a_message(ptlib):
    from optixpathtracer_amd import capi

    buf = (C.c_float * 12)()
    fake = C.c_void_p(1)
    assert ptlib.pt_motion_download(None, 0, buf, C.sizeof(buf)) == capi.PT_ERR_INVALID
    assert b"pt_motion_download" in ptlib.pt_last_error() and b"NULL" in ptlib.pt_last_error()
    assert ptlib.pt_motion_download(fake, 0, None, C.sizeof(buf)) == capi.PT_ERR_INVALID
    assert b"pt_motion_download" in ptlib.pt_last_error() and b"NULL" in ptlib.pt_last_error()
    for kind in (3, -1, 7):  # checked before the renderer is read
        assert ptlib.pt_motion_download(fake, kind, buf, C.sizeof(buf)) == capi.PT_ERR_INVALID, kind
        assert b"pt_motion_download" in ptlib.pt_last_error() and b"kind" in ptlib.pt_last_error()


def _build(tmp_path):
    from optixpathtracer_amd import capi

    exe = tmp_path / "facade_motion"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "facade_motion_check.cpp"), f"-L{capi.LIB_PATH.parent}", "-lptamd",
                    f"-Wl,-rpath,{capi.LIB_PATH.parent}", "-o", str(exe)], check=True)
    return exe


def test_cpp_facade_motion_methods_compile_and_fail_loudly_without_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode in (0, 2), rc.stdout + rc.stderr
    if rc.returncode == 2:
        assert "no HIP device" in rc.stdout


@pytest.mark.gpu
def test_cpp_facade_motion_methods_run_on_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout + rc.stderr
