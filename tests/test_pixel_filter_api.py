"""The anti-aliasing surface without a GPU: the entry points and constants are declared in
include/ptamd.h and bound in capi.py with matching signatures, the versioned struct keeps to its
struct_size, NULL and invalid arguments are refused with a message, the ctypes mirror has the size
the C compiler gives the header's struct, and the C++ facade's new methods compile and link."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "ptamd.h"
NEW = ["pt_pixel_filter_default", "pt_set_pixel_filter", "pt_get_pixel_filter", "pt_pixel_filter_cells",
       "pt_pixel_filter_taps"]
CONSTANTS = {"PT_FILTER_BOX": 0, "PT_FILTER_TENT": 1, "PT_FILTER_GAUSSIAN": 2, "PT_FILTER_MITCHELL": 3}
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float}


def _header():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _ctype(decl: str):
    """The ctypes type of one parameter declaration of the header."""
    from optixpathtracer_amd import capi

    decl = decl.strip()
    if "*" in decl:
        base = decl.replace("const", "").split("*")[0].strip()
        if base == "float":
            return C.POINTER(C.c_float)
        if base == "int32_t":
            return C.POINTER(C.c_int32)
        if base in ("pt_renderer", "void"):
            return C.c_void_p
        return C.POINTER(getattr(capi, base))
    return CTYPES[decl.split()[0]]


def _filter(capi, supersample=1, kind=0, radius=0.0, param=0.0):
    f = capi.pt_pixel_filter()
    f.struct_size = C.sizeof(f)
    f.supersample, f.kind, f.radius, f.param = supersample, kind, radius, param
    return f


def test_entry_points_and_constants_declared_and_bound(ptlib):
    from optixpathtracer_amd import capi

    text = _header()
    for name in NEW:
        m = re.search(rf"([\w ]+?\*?)\s*\b{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert m.group(1).strip() == "int", (name, m.group(1))
        res, args = capi.SIGNATURES[name]
        fn = getattr(ptlib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        assert res is C.c_int
        assert args == [_ctype(p) for p in m.group(2).split(",")], name
    for name, value in CONSTANTS.items():
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
        assert getattr(capi, name) == value
    assert sorted(capi.FILTER_KINDS.values()) == list(range(4))


def test_defaults_respect_struct_size(ptlib):
    from optixpathtracer_amd import capi

    f = capi.pt_pixel_filter()
    f.struct_size = C.sizeof(f)
    f.supersample, f.kind, f.radius, f.param = 9, 9, 9.0, 9.0
    assert ptlib.pt_pixel_filter_default(C.byref(f)) == capi.PT_OK
    assert (f.struct_size, f.supersample, f.kind, f.radius, f.param) == (C.sizeof(f), 1, capi.PT_FILTER_BOX, 0.0, 0.0)
    assert "(1, PT_FILTER_BOX, 0, 0)" in HEADER.read_text()  # the header states them

    # a caller compiled against a shorter struct: size, supersample, kind
    class Guarded(C.Structure):
        _fields_ = [("f", capi.pt_pixel_filter), ("guard", C.c_uint8 * 16)]

    short = capi.pt_pixel_filter.radius.offset
    g = Guarded()
    C.memset(C.byref(g), 0xAB, C.sizeof(g))
    g.f.struct_size = short
    assert ptlib.pt_pixel_filter_default(C.byref(g.f)) == capi.PT_OK
    assert (g.f.struct_size, g.f.supersample, g.f.kind) == (short, 1, 0)
    assert bytes(g)[short:] == b"\xab" * (C.sizeof(g) - short)  # the cut-off fields and the guard are untouched
    # a larger struct_size than the library knows writes the library's own size and no more
    C.memset(C.byref(g), 0xAB, C.sizeof(g))
    g.f.struct_size = C.sizeof(g)
    assert ptlib.pt_pixel_filter_default(C.byref(g.f)) == capi.PT_OK
    assert g.f.struct_size == C.sizeof(g) and g.f.supersample == 1
    assert bytes(g.guard) == b"\xab" * 16
    g.f.struct_size = 0
    assert ptlib.pt_pixel_filter_default(C.byref(g.f)) == capi.PT_ERR_INVALID
    assert b"struct_size" in ptlib.pt_last_error()
    assert ptlib.pt_pixel_filter_default(None) == capi.PT_ERR_INVALID


def test_null_arguments_are_refused_with_a_message(ptlib):
    from optixpathtracer_amd import capi

    f = _filter(capi)
    xy = (C.c_int32 * 2)()
    calls = {
        "pt_set_pixel_filter": lambda: ptlib.pt_set_pixel_filter(None, C.byref(f)),
        "pt_get_pixel_filter": lambda: ptlib.pt_get_pixel_filter(None, C.byref(f)),
        "pt_pixel_filter_cells": lambda: ptlib.pt_pixel_filter_cells(1, None),
    }
    for name, call in calls.items():
        assert call() == capi.PT_ERR_INVALID, name
        msg = ptlib.pt_last_error()
        assert name.encode() in msg and b"NULL" in msg, msg
    assert ptlib.pt_set_pixel_filter(None, None) == capi.PT_ERR_INVALID
    assert ptlib.pt_pixel_filter_cells(1, xy) == capi.PT_OK and list(xy) == [0, 0]


def test_invalid_settings_are_refused(ptlib):
    from optixpathtracer_amd import capi

    R = C.c_int32(-1)
    w = (C.c_float * 5)()
    bad = [dict(supersample=0), dict(supersample=3), dict(supersample=16), dict(supersample=-2), dict(kind=4),
           dict(kind=-1), dict(radius=0.25), dict(radius=2.75), dict(radius=-1.0), dict(radius=float("nan")),
           dict(kind=capi.PT_FILTER_GAUSSIAN, param=float("nan"))]
    for kw in bad:
        f = _filter(capi, **kw)
        assert ptlib.pt_pixel_filter_taps(C.byref(f), 0, C.byref(R), w, w) == capi.PT_ERR_INVALID, kw
        assert b"pt_pixel_filter_taps" in ptlib.pt_last_error()
    f = _filter(capi, supersample=2, kind=capi.PT_FILTER_TENT)
    for cell in (-1, 4):
        assert ptlib.pt_pixel_filter_taps(C.byref(f), cell, C.byref(R), w, w) == capi.PT_ERR_INVALID
    f.struct_size = 0
    assert ptlib.pt_pixel_filter_taps(C.byref(f), 0, C.byref(R), w, w) == capi.PT_ERR_INVALID
    assert b"struct_size" in ptlib.pt_last_error()
    for s in (0, 3, 16):
        assert ptlib.pt_pixel_filter_cells(s, (C.c_int32 * 512)()) == capi.PT_ERR_INVALID
    # NULL = the default setting; any of the outputs may be left out
    assert ptlib.pt_pixel_filter_taps(None, 0, C.byref(R), w, None) == capi.PT_OK
    assert R.value == 0 and w[0] == 1.0
    assert ptlib.pt_pixel_filter_taps(None, 0, None, None, None) == capi.PT_OK
    assert R.value == 0


def test_python_names_are_checked():
    from optixpathtracer_amd import capi
    from optixpathtracer_amd.renderer import OptixRenderer, pixel_filter_taps

    for name in ("set_pixel_filter", "pixel_filter"):
        assert callable(getattr(OptixRenderer, name))
    with pytest.raises(capi.PTError) as e:
        pixel_filter_taps(2, "lanczos")
    assert e.value.status == capi.PT_ERR_INVALID
    R, wx, wy = pixel_filter_taps(2, "mitchell", cell=3)
    assert R == 2 and len(wx) == len(wy) == 5


def test_struct_mirror_has_the_header_size(tmp_path):
    from optixpathtracer_amd import capi

    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptamd.h"\n'
                   'int main(void) { printf("%zu %zu %zu", sizeof(pt_pixel_filter), offsetof(pt_pixel_filter, kind),\n'
                   '    offsetof(pt_pixel_filter, param)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.pt_pixel_filter), capi.pt_pixel_filter.kind.offset, capi.pt_pixel_filter.param.offset]
    body = re.search(r"typedef struct pt_pixel_filter \{(.*?)\} pt_pixel_filter;", _header(), flags=re.S).group(1)
    names = [f for f, _ in capi.pt_pixel_filter._fields_]
    assert re.findall(r"\b(\w+);", body) == names and names[0] == "struct_size"


def _build(tmp_path):
    from optixpathtracer_amd import capi

    exe = tmp_path / "facade_pixel_filter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "facade_pixel_filter_check.cpp"), f"-L{capi.LIB_PATH.parent}", "-lptamd",
                    f"-Wl,-rpath,{capi.LIB_PATH.parent}", "-o", str(exe)], check=True)
    return exe


def test_cpp_facade_pixel_filter_methods_compile_and_fail_loudly_without_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode in (0, 2), rc.stdout + rc.stderr
    if rc.returncode == 2:
        assert "no HIP device" in rc.stdout


@pytest.mark.gpu
def test_cpp_facade_pixel_filter_methods_run_on_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout + rc.stderr
