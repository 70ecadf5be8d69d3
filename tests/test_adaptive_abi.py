"""Adaptive sampling (rt3_render_path_adaptive*) without a GPU: header / binding / library coverage with the declared signatures,
the size of rt3_adaptive_params, the Python methods, the NULL context, the "no device" stubs, and the command line's --adaptive / --counts."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> the parameter types of the declaration in include/rt3.h, spaces removed
DECLARED = {
    "rt3_render_path_adaptive": ["rt3_ctx*", "constrt3_camera*", "constrt3_params*", "constrt3_adaptive_params*", "uint32_t*", "uint32_t*"],
    "rt3_render_path_adaptive_device": ["rt3_ctx*", "constrt3_camera*", "constrt3_params*", "constrt3_adaptive_params*", "void*", "void*", "void*"],
}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt3.h")).read(), flags=re.S)


def header_declarations():
    out = {}
    for res, name, args in re.findall(r"\b(int)\s+(rt3_render_path_adaptive[a-z_]*)\s*\(([^)]*)\)\s*;", header_text()):
        out[name] = [re.sub(r"\s+", "", a.strip()[:a.strip().rindex("*") + 1]) for a in args.split(",")]
    return out


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    assert header_declarations() == DECLARED
    for s, types in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p] * len(types), s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3
    assert "RT3_ABI_VERSION 3u" in open(os.path.join(ROOT, "include", "rt3.h")).read()


def test_the_wire_struct_is_16_bytes_here_in_the_header_and_in_the_library(rt3, tmp_path):
    assert C.sizeof(rt3.ADAPTIVE_PARAMS) == 16
    assert [(n, t) for n, t in rt3.ADAPTIVE_PARAMS._fields_] == [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("threshold", C.c_float),
                                                                 ("dark", C.c_float)]
    m = re.search(r"typedef struct rt3_adaptive_params \{(.*?)\} rt3_adaptive_params;", header_text(), flags=re.S)
    assert re.findall(r"(uint32_t|float)\s+(\w+);", m.group(1)) == [("uint32_t", "min_spp"), ("uint32_t", "step_spp"), ("float", "threshold"),
                                                                     ("float", "dark")]
    src = tmp_path / "size.c"
    src.write_text('#include "rt3.h"\n_Static_assert(sizeof(rt3_adaptive_params) == 16, "size");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")])
    device = open(os.path.join(ROOT, "raytracer-3_amd", "csrc", "rt3_device.hip")).read()
    assert 'static_assert(sizeof(rt3_adaptive_params) == 16, "rt3.h: rt3_adaptive_params");' in device


def test_python_methods(rt3):
    sig = inspect.signature(rt3.HipRenderer.render_adaptive)
    assert list(sig.parameters) == ["self", "camera_c", "params", "threshold", "min_spp", "step_spp", "dark"]
    assert [sig.parameters[k].default for k in ("threshold", "min_spp", "step_spp", "dark")] == [0.05, 16, 16, 0.01]
    sig = inspect.signature(rt3.HipRenderer.render_adaptive_device)
    assert list(sig.parameters)[:4] == ["self", "camera_c", "params", "d_out"]
    assert [sig.parameters[k].default for k in ("d_counts", "stream_ptr", "threshold", "min_spp", "step_spp", "dark")] == [None, None, 0.05, 16, 16, 0.01]


def calls(rt3, ctx):
    cam = rt3.weekend_camera(16, 9).c
    p = rt3.make_params(16, 9, spp=32, max_depth=4)
    ap = rt3.ADAPTIVE_PARAMS(16, 16, 0.05, 0.01)
    buf = np.zeros(256, np.uint32)
    b = buf.ctypes.data_as(C.c_void_p)
    keep = (cam, p, ap, buf)
    return keep, (("rt3_render_path_adaptive", (ctx, C.byref(cam), C.byref(p), C.byref(ap), b, b)),
                  ("rt3_render_path_adaptive", (ctx, C.byref(cam), C.byref(p), C.byref(ap), b, None)),
                  ("rt3_render_path_adaptive_device", (ctx, C.byref(cam), C.byref(p), C.byref(ap), b, b, None)),
                  ("rt3_render_path_adaptive_device", (ctx, C.byref(cam), C.byref(p), C.byref(ap), b, None, None)))


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    keep, table = calls(rt3, None)
    for name, args in table:
        assert getattr(L, name)(*args) == -1, name                    # RT3_E_ARG
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    keep, table = calls(rt3, C.c_void_p(0x10))                         # never dereferenced by a stub
    for name, args in table:
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args) == -2, name                                   # RT3_E_DEVICE


def test_no_renderer_without_a_device(rt3):
    import torch
    if torch.cuda.is_available():
        return                                                         # (the GPU suite covers the calls themselves)
    with pytest.raises(rt3.Fatal, match="no CPU fallback"):
        rt3.initialize_renderer(0).render_adaptive(rt3.weekend_camera(16, 9).c, rt3.make_params(16, 9, spp=32))


@pytest.mark.parametrize("value", ["0", "-0.05", "nan", "inf", "abc", "0.05,", "0.05,1", "0.05,16,0", "0.05,16,8,4", "0.05,x", "0.05,16,-1",
                                   "0.05 ", "0.05,4294967296", "1e-60"])
def test_cli_refuses_bad_adaptive_values(value):
    rc, out, err = run("--scene", "weekend", "--spp", "64", "--adaptive=" + value, "o.png")
    assert rc == -1 and ("Invalid adaptive '%s'" % value in err or "--adaptive has no value." in err), err


@pytest.mark.parametrize("args,message", [
    (("--adaptive", "0.05", "o.png"), "--adaptive needs the path tracer (Mode X): pass --spp, the budget."),
    (("--scene", "weekend", "--spp", "64", "--counts", "c.pfm", "o.png"), "--counts needs --adaptive"),
    (("--scene", "weekend", "--spp", "64", "--adaptive", "o.png"), "Invalid adaptive 'o.png'"),
    (("--scene", "weekend", "--spp", "64", "o.png", "--adaptive"), "--adaptive has no value."),
    (("--scene", "weekend", "--spp", "64", "--adaptive", "0.05", "o.png", "--counts"), "--counts has no value."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


@pytest.mark.parametrize("value", ["0.05", "0.1,8", "0.02,4,2", "1e-30,2,1", "5e-2,16,16"])
def test_cli_accepts_good_values_and_then_needs_a_device(value):
    """Past the parser the command line reaches for the device: without one that is the fatal convention's -1 with the backend's message,
    with one the render itself (the GPU suite)."""
    import torch
    if torch.cuda.is_available():
        return
    rc, out, err = run("--scene", "three", "--spp", "64", "-W", "32", "-H", "18", "--adaptive", value, "--counts", "c.pfm", "o.ppm", "-f", "ppm")
    assert rc == -1 and "Invalid adaptive" not in err and "fatal:" in err, err


def test_cli_help_lists_the_new_options():
    rc, out, err = run("-h")
    assert rc == 0 and "--adaptive" in out and "--counts" in out and "T[,MIN[,STEP]]" in out
