"""Scene updates (rt3_update_spheres*, rt3_update_mesh*) without a GPU: header / binding / library coverage with the declared
signatures, the Python methods, the NULL context, the "no device" stubs, and the command line's --refit."""
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
    "rt3_update_spheres": ["rt3_ctx*", "constfloat*", "uint32_t"],
    "rt3_update_spheres_device": ["rt3_ctx*", "constvoid*", "uint32_t", "void*"],
    "rt3_update_mesh": ["rt3_ctx*", "constrt3_gface*", "constfloat*", "uint32_t"],
    "rt3_update_mesh_device": ["rt3_ctx*", "constvoid*", "constvoid*", "uint32_t", "void*"],
}


def header_declarations():
    text = open(os.path.join(ROOT, "include", "rt3.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int)\s+(rt3_update_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
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
    vp, u32 = C.c_void_p, C.c_uint32
    ctype = {"rt3_ctx*": vp, "constfloat*": vp, "constvoid*": vp, "void*": vp, "constrt3_gface*": vp, "uint32_t": u32}
    for s, types in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is C.c_int and list(fn.argtypes) == [ctype[t] for t in types], s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3
    assert "RT3_ABI_VERSION 3u" in open(os.path.join(ROOT, "include", "rt3.h")).read()


def test_python_methods(rt3):
    assert list(inspect.signature(rt3.HipRenderer.update_spheres).parameters) == ["self", "center_radius"]
    sig = inspect.signature(rt3.HipRenderer.update_mesh)
    assert list(sig.parameters) == ["self", "vertices", "faces"] and sig.parameters["faces"].default is None


def calls(ctx):
    buf = np.zeros(256, np.float32)
    b = buf.ctypes.data_as(C.c_void_p)
    return buf, (("rt3_update_spheres", (ctx, b, 4)), ("rt3_update_spheres_device", (ctx, b, 4, None)),
                 ("rt3_update_mesh", (ctx, None, b, 4)), ("rt3_update_mesh_device", (ctx, None, b, 4, None)),
                 ("rt3_update_mesh", (ctx, b, b, 4)), ("rt3_update_mesh_device", (ctx, b, b, 4, None)))


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


def test_no_renderer_without_a_device(rt3):
    import torch
    if torch.cuda.is_available():
        return                                                         # (the GPU suite covers the calls themselves)
    with pytest.raises(rt3.Fatal, match="no CPU fallback"):
        rt3.initialize_renderer(0).update_spheres(np.zeros((1, 4), np.float32))


@pytest.mark.parametrize("args,message", [
    (("--scene", "weekend", "--refit", "o.png"), "--refit needs --slide"),
    (("--scene", "weekend", "--frames", "2", "--refit", "o.png"), "--refit needs --slide"),
    (("--scene", "weekend", "--refit", "--slide", "0.1,0,0", "o.png"), "--slide needs a sequence: pass --frames N with N of at least 2."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_help_lists_the_new_option():
    rc, out, err = run("-h")
    assert rc == 0 and "--refit" in out
