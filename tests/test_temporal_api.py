"""The temporal-filter surface without a GPU: the entry points and constants are declared in
include/ptamd.h and bound in capi.py with matching signatures, the versioned structs keep to their
struct_size, NULL renderers are refused with a message, the option checks name what they refuse, the
ctypes mirrors have the sizes the C compiler gives the header's structs, the restatement's fp32
matrix inverse inverts the library's camera matrices, and the C++ facade's new methods compile and link."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "ptamd.h"
NEW = {
    "pt_temporal_options_default": "int", "pt_denoise_temporal": "int", "pt_temporal_reset": "int",
    "pt_temporal_channels": "int", "pt_temporal_download": "int", "pt_get_temporal_info": "int",
}
CONSTANTS = {"PT_TEMPORAL_HISTORY_LENGTH": 0, "PT_TEMPORAL_MOMENTS": 1, "PT_TEMPORAL_VARIANCE": 2, "PT_TEMPORAL_COLOR": 3}
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
DEFAULTS = {"alpha": 0.2, "alpha_moments": 0.2, "max_history": 32, "normal_cos": 0.9, "plane_distance": 0.02,
            "sigma_luminance": 4.0, "variance_history": 4}


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
        assert res is C.c_int
        assert args == [_ctype(p) for p in m.group(2).split(",")], name
    for name, value in CONSTANTS.items():
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
        assert getattr(capi, name) == value
    assert sorted(capi.TEMPORAL_KINDS.values()) == list(range(4))
    assert [ptlib.pt_temporal_channels(k) for k in range(4)] == [1, 2, 1, 3]
    assert ptlib.pt_temporal_channels(4) < 0 and ptlib.pt_temporal_channels(-1) < 0


def test_option_defaults_respect_struct_size(ptlib):
    from optixpathtracer_amd import capi

    o = capi.pt_temporal_options()
    o.struct_size = C.sizeof(o)
    assert ptlib.pt_temporal_options_default(C.byref(o)) == capi.PT_OK
    assert o.struct_size == C.sizeof(o)
    for k, v in DEFAULTS.items():
        assert getattr(o, k) == (v if isinstance(v, int) else C.c_float(v).value), k

    # a caller compiled against a shorter struct: size, alpha, alpha_moments, max_history
    class Guarded(C.Structure):
        _fields_ = [("o", capi.pt_temporal_options), ("guard", C.c_uint8 * 16)]

    short = capi.pt_temporal_options.normal_cos.offset
    g = Guarded()
    C.memset(C.byref(g), 0xAB, C.sizeof(g))
    g.o.struct_size = short
    assert ptlib.pt_temporal_options_default(C.byref(g.o)) == capi.PT_OK
    assert (g.o.struct_size, g.o.alpha, g.o.max_history) == (short, C.c_float(0.2).value, 32)
    raw = bytes(g)
    assert raw[short:] == b"\xab" * (C.sizeof(g) - short)  # the cut-off fields and the guard are untouched
    # a larger struct_size than the library knows writes the library's own size and no more
    C.memset(C.byref(g), 0xAB, C.sizeof(g))
    g.o.struct_size = C.sizeof(g)
    assert ptlib.pt_temporal_options_default(C.byref(g.o)) == capi.PT_OK
    assert g.o.struct_size == C.sizeof(g) and g.o.variance_history == 4
    assert bytes(g.guard) == b"\xab" * 16
    g.o.struct_size = 0
    assert ptlib.pt_temporal_options_default(C.byref(g.o)) == capi.PT_ERR_INVALID
    assert b"struct_size" in ptlib.pt_last_error()
    assert ptlib.pt_temporal_options_default(None) == capi.PT_ERR_INVALID


def test_null_renderers_are_refused_with_a_message(ptlib):
    from optixpathtracer_amd import capi

    buf = (C.c_float * 12)()
    info = capi.pt_temporal_info()
    info.struct_size = C.sizeof(info)
    calls = {
        "pt_denoise_temporal": lambda: ptlib.pt_denoise_temporal(None, capi.PT_DENOISE_SRC_ACCUM, None, 1.0, None, None, None),
        "pt_temporal_reset": lambda: ptlib.pt_temporal_reset(None),
        "pt_temporal_download": lambda: ptlib.pt_temporal_download(None, 0, buf, C.sizeof(buf)),
        "pt_get_temporal_info": lambda: ptlib.pt_get_temporal_info(None, C.byref(info)),
    }
    for name, call in calls.items():
        assert call() == capi.PT_ERR_INVALID, name
        msg = ptlib.pt_last_error()
        assert name.encode() in msg and b"NULL" in msg, msg


def test_option_validation_messages(ptlib):
    """The options are checked before the renderer's state: a fake non-NULL handle is never read."""
    from optixpathtracer_amd import capi

    img = (C.c_float * 3)()
    fake = C.c_void_p(1)

    def call(dopt=None, **kw):
        t = capi.pt_temporal_options()
        t.struct_size = C.sizeof(t)
        assert ptlib.pt_temporal_options_default(C.byref(t)) == 0
        for k, v in kw.items():
            setattr(t, k, v)
        return ptlib.pt_denoise_temporal(fake, capi.PT_DENOISE_SRC_HOST, img, 1.0, C.byref(t), dopt, None)

    bad = [("alpha", 0.0, b"alpha"), ("alpha", 1.0001, b"alpha"), ("alpha", float("nan"), b"alpha"),
           ("alpha_moments", -1.0, b"alpha_moments"), ("max_history", 0, b"max_history"),
           ("normal_cos", 1.01, b"normal_cos"), ("normal_cos", -1.01, b"normal_cos"),
           ("plane_distance", 0.0, b"plane_distance"), ("plane_distance", float("nan"), b"plane_distance"),
           ("sigma_luminance", 0.0, b"sigma_luminance"), ("variance_history", -1, b"variance_history")]
    for k, v, word in bad:
        assert call(**{k: v}) == capi.PT_ERR_INVALID, (k, v)
        assert word in ptlib.pt_last_error() and b"pt_denoise_temporal" in ptlib.pt_last_error(), (k, ptlib.pt_last_error())
    d = capi.pt_denoise_options()
    d.struct_size = C.sizeof(d)
    assert ptlib.pt_denoise_options_default(C.byref(d)) == 0
    d.iterations = 9
    assert call(C.byref(d)) == capi.PT_ERR_INVALID and b"iterations" in ptlib.pt_last_error()
    d.iterations, d.sigma_normal = 5, 0.0
    assert call(C.byref(d)) == capi.PT_ERR_INVALID and b"sigma" in ptlib.pt_last_error()
    d.sigma_normal, d.struct_size = 0.3, 0
    assert call(C.byref(d)) == capi.PT_ERR_INVALID and b"struct_size" in ptlib.pt_last_error()
    assert ptlib.pt_denoise_temporal(fake, 3, img, 1.0, None, None, None) == capi.PT_ERR_INVALID
    assert b"source" in ptlib.pt_last_error()
    assert ptlib.pt_denoise_temporal(fake, capi.PT_DENOISE_SRC_HOST, None, 1.0, None, None, None) == capi.PT_ERR_INVALID
    assert b"host_in" in ptlib.pt_last_error()


def test_struct_mirrors_have_the_header_sizes(tmp_path):
    from optixpathtracer_amd import capi

    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ptamd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu", sizeof(pt_temporal_options), sizeof(pt_temporal_info),\n'
                   '    offsetof(pt_temporal_options, variance_history), offsetof(pt_temporal_info, calls),\n'
                   '    offsetof(pt_temporal_info, filter_ms)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(capi.pt_temporal_options), C.sizeof(capi.pt_temporal_info),
                   capi.pt_temporal_options.variance_history.offset, capi.pt_temporal_info.calls.offset,
                   capi.pt_temporal_info.filter_ms.offset]
    for cls in (capi.pt_temporal_options, capi.pt_temporal_info):
        body = re.search(rf"typedef struct {cls.__name__} \{{(.*?)\}} {cls.__name__};", _header(), flags=re.S).group(1)
        names = [f for f, _ in cls._fields_]
        assert re.findall(r"\b(\w+);", body) == names and names[0] == "struct_size"


def test_restated_inverse_inverts():
    """The restatement's fp32 glm-style inverse inverts the matrices pt_camera_from_blender hands
    out (that it walks the library's bits is what the GPU sequence test shows)."""
    from optixpathtracer_amd.renderer import camera_from_blender
    from temporal_ref import mat4_inverse

    for pos, rot in [((3.85, 0.0, 1.0), (90.0, 0.0, 90.0)), ((1.25, 0.16, 0.3), (90.0, 0.0, 92.0)), ((0.2, 0.3, 1.0), (80.0, 0.0, -30.0))]:
        _, iv, ip = camera_from_blender(pos, rot, 40.0, 48, 32)
        for m in (iv, ip):
            back = mat4_inverse(m)
            assert back.dtype == np.float32 and np.isfinite(back).all()
            # a true inverse: back * m is the identity to fp32 rounding of entries up to 100
            prod = back.reshape(4, 4).T.astype(np.float64) @ m.reshape(4, 4).T.astype(np.float64)
            assert np.abs(prod - np.eye(4)).max() < 1e-4


def _build(tmp_path):
    from optixpathtracer_amd import capi

    exe = tmp_path / "facade_temporal"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "facade_temporal_check.cpp"), f"-L{capi.LIB_PATH.parent}", "-lptamd",
                    f"-Wl,-rpath,{capi.LIB_PATH.parent}", "-o", str(exe)], check=True)
    return exe


def test_cpp_facade_temporal_methods_compile_and_fail_loudly_without_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode in (0, 2), rc.stdout + rc.stderr
    if rc.returncode == 2:
        assert "no HIP device" in rc.stdout


@pytest.mark.gpu
def test_cpp_facade_temporal_methods_run_on_gpu(tmp_path, ptlib):
    exe = _build(tmp_path)
    rc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout + rc.stderr
