"""rt3_regroup*  without a GPU: header / binding / library coverage with the declared signatures, the Python methods, the
NULL context, the "no device" stubs, and the command line's --regroup."""
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
    "rt3_regroup": ["rt3_ctx*", "uint32_t"],
    "rt3_regroup_device": ["rt3_ctx*", "uint32_t", "void*"],
    "rt3_debug_group_order": ["rt3_ctx*", "uint32_t", "uint32_t*", "uint64_t", "uint32_t*"],
}


def header_declarations():
    text = open(os.path.join(ROOT, "include", "rt3.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int)\s+(rt3_regroup[a-z_]*|rt3_debug_group_order)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(re.sub(r"\s+", "", a[:a.rindex("*") + 1] if "*" in a else a.rsplit(None, 1)[0]))
        out[name] = types
    return out


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    assert header_declarations() == DECLARED
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    ctype = {"rt3_ctx*": vp, "void*": vp, "uint32_t*": vp, "uint32_t": u32, "uint64_t": u64}
    for s, types in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is C.c_int and list(fn.argtypes) == [ctype[t] for t in types], s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3
    text = open(os.path.join(ROOT, "include", "rt3.h")).read()
    assert "RT3_ABI_VERSION 3u" in text
    assert re.search(r"#define\s+RT3_REGROUP_SPHERES\s+1u", text) and re.search(r"#define\s+RT3_REGROUP_MESH\s+2u", text)
    assert (rt3.REGROUP_SPHERES, rt3.REGROUP_MESH) == (1, 2)


def test_python_methods(rt3):
    sig = inspect.signature(rt3.HipRenderer.regroup)
    assert list(sig.parameters) == ["self", "spheres", "mesh"]
    assert sig.parameters["spheres"].default is True and sig.parameters["mesh"].default is True
    assert list(inspect.signature(rt3.HipRenderer.group_order).parameters) == ["self", "what"]


def calls(ctx):
    buf = np.zeros(256, np.uint32)
    n = C.c_uint32(0)
    b = buf.ctypes.data_as(C.c_void_p)
    return (buf, n), (("rt3_regroup", (ctx, 1)), ("rt3_regroup", (ctx, 3)), ("rt3_regroup_device", (ctx, 2, None)),
                      ("rt3_debug_group_order", (ctx, 1, b, 256, C.byref(n))))


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    keep, table = calls(None)
    for name, args in table:
        assert getattr(L, name)(*args) == -1, name                    # RT3_E_ARG
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    keep, table = calls(C.c_void_p(0x10))                              # never dereferenced by a stub
    for name, args in table:
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args) == -2, name                                   # RT3_E_DEVICE


def test_the_cpp_mirror_declares_regroup():
    text = open(os.path.join(ROOT, "raytracer-3_amd", "host", "renderer", "Renderer.hpp")).read()
    assert re.search(r"void\s+regroup\s*\(\s*bool\s+spheres\s*=\s*true\s*,\s*bool\s+mesh\s*=\s*true\s*\)\s*;", text)


@pytest.mark.parametrize("args,message", [
    (("--scene", "weekend", "--regroup", "2", "o.png"), "--regroup needs --refit"),
    (("--scene", "weekend", "--frames", "4", "--slide", "0.1,0,0", "--regroup", "2", "o.png"), "--regroup needs --refit"),
    (("--scene", "weekend", "--frames", "4", "--slide", "0.1,0,0", "--refit", "--regroup", "0", "o.png"), "--regroup must be at least 1"),
    (("--scene", "weekend", "--frames", "4", "--slide", "0.1,0,0", "--refit", "--regroup", "x", "o.png"), "Invalid regroup"),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_help_lists_the_new_option():
    rc, out, err = run("-h")
    assert rc == 0 and "--regroup" in out
