"""The adaptive-sampling surface without a GPU: the entry points and constants are declared in
include/ptamd.h and bound in capi.py with matching signatures, the versioned structs keep to their
struct_size, NULL renderers are refused with a message, the ctypes mirrors have the sizes the C
compiler gives the header's structs, and the C++ facade's new methods compile and link."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "ptamd.h"
# name -> the header's return type
NEW = {
    "pt_adaptive_options_default": "int", "pt_render_adaptive": "int", "pt_adaptive_channels": "int",
    "pt_adaptive_download": "int", "pt_adaptive_mean_device_ptr": "float*", "pt_get_adaptive_info": "int",
}
CONSTANTS = {
    "PT_ADAPTIVE_SAMPLES": 0, "PT_ADAPTIVE_ERROR": 1, "PT_ADAPTIVE_MOMENTS": 2, "PT_ADAPTIVE_TILE_ERROR": 3,
    "PT_ADAPTIVE_TILE_ROUNDS": 4, "PT_DENOISE_SRC_ADAPTIVE": 3,
    # the sources that were there keep their numbers
    "PT_DENOISE_SRC_ACCUM": 0, "PT_DENOISE_SRC_DISPLAY": 1, "PT_DENOISE_SRC_HOST": 2,
}
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float}
DEFAULTS = (0.05, 16, 1024, 16, 0.01)  # threshold, min_samples, max_samples, round_frames, luminance_floor


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
        if base in ("pt_renderer", "void"):
            return C.c_void_p
        return C.POINTER(getattr(capi, base))
    return CTYPES[decl.split()[0]]


def test_entry_points_and_constants_declared_and_bound(ptlib):
    from optixpathtracer_amd import capi

    text = _header()
    for name, ret in NEW.items():
        m = re.search(rf"([\w ]+?\*?)\s*\b{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert m.group(1).replace(" *", "*").strip() == ret, (name, m.group(1))
        res, args = capi.SIGNATURES[name]
        fn = getattr(ptlib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        assert res is (C.c_int if ret == "int" else C.c_void_p)
        assert args == [_ctype(p) for p in m.group(2).split(",")], name
    for name, value in CONSTANTS.items():
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
        assert getattr(capi, name) == value
    assert sorted(capi.ADAPTIVE_KINDS.values()) == list(range(5))


def test_adaptive_channels(ptlib):
    assert [ptlib.pt_adaptive_channels(k) for k in range(5)] == [1, 1, 2, 1, 1]
    assert ptlib.pt_adaptive_channels(5) < 0 and ptlib.pt_adaptive_channels(-1) < 0


def test_option_defaults_respect_struct_size(ptlib):
    from optixpathtracer_amd import capi

    o = capi.pt_adaptive_options()
    o.struct_size = C.sizeof(o)
    assert ptlib.pt_adaptive_options_default(C.byref(o)) == capi.PT_OK
    got = (o.threshold, o.min_samples, o.max_samples, o.round_frames, o.luminance_floor)
    assert o.struct_size == C.sizeof(o)
    assert got == (C.c_float(DEFAULTS[0]).value, *DEFAULTS[1:4], C.c_float(DEFAULTS[4]).value)
    # the header states them
    assert "(0.05, 16, 1024, 16, 0.01)" in HEADER.read_text()

    # a caller compiled against a shorter struct: size, threshold, min_samples
    class Guarded(C.Structure):
        _fields_ = [("o", capi.pt_adaptive_options), ("guard", C.c_uint8 * 16)]

    short = capi.pt_adaptive_options.max_samples.offset
    g = Guarded()
    C.memset(C.byref(g), 0xAB, C.sizeof(g))
    g.o.struct_size = short
    assert ptlib.pt_adaptive_options_default(C.byref(g.o)) == capi.PT_OK
    assert (g.o.struct_size, g.o.threshold, g.o.min_samples) == (short, C.c_float(0.05).value, 16)
    raw = bytes(g)
    assert raw[short:] == b"\xab" * (C.sizeof(g) - short)  # the cut-off fields and the guard are untouched
    # a larger struct_size than the library knows writes the library's own size and no more
    C.memset(C.byref(g), 0xAB, C.sizeof(g))
    g.o.struct_size = C.sizeof(g)
    assert ptlib.pt_adaptive_options_default(C.byref(g.o)) == capi.PT_OK
    assert g.o.struct_size == C.sizeof(g) and g.o.round_frames == 16
    assert bytes(g.guard) == b"\xab" * 16
    # no size at all
    g.o.struct_size = 0
    assert ptlib.pt_adaptive_options_default(C.byref(g.o)) == capi.PT_ERR_INVALID
    assert b"struct_size" in ptlib.pt_last_error()
    assert ptlib.pt_adaptive_options_default(None) == capi.PT_ERR_INVALID


def test_null_renderers_are_refused_with_a_message(ptlib):
    from optixpathtracer_amd import capi

    buf = (C.c_float * 12)()
    info = capi.pt_adaptive_info()
    info.struct_size = C.sizeof(info)
    calls = {
        "pt_render_adaptive": lambda: ptlib.pt_render_adaptive(None, 1, None, None),
        "pt_adaptive_download": lambda: ptlib.pt_adaptive_download(None, 0, buf, C.sizeof(buf)),
        "pt_get_adaptive_info": lambda: ptlib.pt_get_adaptive_info(None, C.byref(info)),
    }
    for name, call in calls.items():
        assert call() == capi.PT_ERR_INVALID, name
        msg = ptlib.pt_last_error()
        assert name.encode() in msg and b"NULL" in msg, msg
    assert ptlib.pt_adaptive_mean_device_ptr(None) is None
    # the new denoise source reaches the renderer check like the others
    assert ptlib.pt_denoise(None, capi.PT_DENOISE_SRC_ADAPTIVE, None, 1.0, None, None) == capi.PT_ERR_INVALID
    assert b"NULL renderer" in ptlib.pt_last_error()
    # ... and takes no host image beside it (checked before the renderer is touched)
    fake = C.c_void_p(1)
    for fn, args in ((ptlib.pt_denoise, (None, None)), (ptlib.pt_denoise_temporal, (None, None, None))):
        assert fn(fake, capi.PT_DENOISE_SRC_ADAPTIVE, buf, 1.0, *args) == capi.PT_ERR_INVALID
        assert b"host_in" in ptlib.pt_last_error() and b"source" in ptlib.pt_last_error()


def test_struct_mirrors_have_the_header_sizes(tmp_path):
    from optixpathtracer_amd import capi

    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptamd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu", sizeof(pt_adaptive_options), sizeof(pt_adaptive_info),\n'
                   '    offsetof(pt_adaptive_options, luminance_floor), offsetof(pt_adaptive_info, samples),\n'
                   '    offsetof(pt_adaptive_info, estimate_ms)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.pt_adaptive_options), C.sizeof(capi.pt_adaptive_info),
                   capi.pt_adaptive_options.luminance_floor.offset, capi.pt_adaptive_info.samples.offset,
                   capi.pt_adaptive_info.estimate_ms.offset]
    # the mirrors list the header's fields in the header's order, struct_size first
    for cls in (capi.pt_adaptive_options, capi.pt_adaptive_info):
        body = re.search(rf"typedef struct {cls.__name__} \{{(.*?)\}} {cls.__name__};", _header(), flags=re.S).group(1)
        names = [f for f, _ in cls._fields_]
        assert re.findall(r"\b(\w+);", body) == names and names[0] == "struct_size"


def test_python_facade_names_the_new_source_and_methods():
    from optixpathtracer_amd.renderer import OptixRenderer

    for name in ("render_adaptive", "adaptive_state", "adaptive_info"):
        assert callable(getattr(OptixRenderer, name))


def _build(tmp_path):
    from optixpathtracer_amd import capi

    exe = tmp_path / "facade_adaptive"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "facade_adaptive_check.cpp"), f"-L{capi.LIB_PATH.parent}", "-lptamd",
                    f"-Wl,-rpath,{capi.LIB_PATH.parent}", "-o", str(exe)], check=True)
    return exe


def test_cpp_facade_adaptive_methods_compile_and_fail_loudly_without_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode in (0, 2), rc.stdout + rc.stderr
    if rc.returncode == 2:
        assert "no HIP device" in rc.stdout


@pytest.mark.gpu
def test_cpp_facade_adaptive_methods_run_on_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout + rc.stderr
