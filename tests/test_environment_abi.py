"""The environment map (rt3_set_environment*) without a GPU: header / binding / library coverage with the declared signatures, the
Python surface, the refusals of the host-only lookup, the NULL context, the "no device" stubs and the command line's --env."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (result, the parameter types of the declaration in include/rt3.h, spaces removed)
DECLARED = {
    "rt3_set_environment": ("int", ["rt3_ctx*", "constfloat*", "uint32_t"]),
    "rt3_set_environment_device": ("int", ["rt3_ctx*", "constvoid*", "uint32_t", "void*"]),
    "rt3_clear_environment": ("int", ["rt3_ctx*"]),
    "rt3_environment_size": ("uint32_t", ["rt3_ctx*"]),
    "rt3_debug_environment_lookup": ("int", ["constfloat*", "uint32_t", "constfloat", "float"]),     # (d[3] and out_rgb[3]: arrays, pointers on the wire)
}


def header_declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt3.h")).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|uint32_t)\s+(rt3_[a-z_]*environment[a-z_]*)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(re.sub(r"\s+", "", a[:a.rindex("*") + 1] if "*" in a else a[:a.rindex(" ")]))
        out[name] = (res, types)
    return out


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    assert header_declarations() == DECLARED
    for s, (res, types) in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is (C.c_int if res == "int" else C.c_uint32), s
        assert list(fn.argtypes) == [C.c_uint32 if t == "uint32_t" else C.c_void_p for t in types], s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3            # additions only: every existing struct is unchanged
    header = open(os.path.join(ROOT, "include", "rt3.h")).read()
    assert "RT3_ABI_VERSION 3u" in header and "#define RT3_ENV_MAX_FACE 2048u" in header


def test_python_surface(rt3):
    H = rt3.HipRenderer
    assert list(inspect.signature(H.set_environment).parameters) == ["self", "cube"]
    assert list(inspect.signature(H.clear_environment).parameters) == ["self"]
    assert list(inspect.signature(H.environment_size).parameters) == ["self"]
    assert list(inspect.signature(H.environment_lookup).parameters) == ["cube", "d"]
    assert list(inspect.signature(rt3.cube_from_equirect).parameters) == ["image", "n"]
    for bad in (np.zeros((5, 2, 2, 4)), np.zeros((6, 2, 3, 4)), np.zeros((6, 2, 2, 2)), np.zeros((6, 2, 2)), np.zeros((6, 0, 0, 4))):
        with pytest.raises(rt3.Fatal):
            rt3.environment_lookup(bad, [0, 0, 1])


def test_the_host_lookup_refuses_bad_arguments(rt3):
    L = rt3.lib()
    rgba = np.ones((6, 2, 2, 4), np.float32)
    d = np.array([0, 0, 1], np.float32)
    out = np.full(3, 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                          # noqa: E731
    assert L.rt3_debug_environment_lookup(p(rgba), 2, p(d), p(out)) == 0 and out.tolist() == [1, 1, 1]
    out[:] = 7.0
    for args in ((None, 2, p(d), p(out)), (p(rgba), 2, None, p(out)), (p(rgba), 2, p(d), None), (p(rgba), 0, p(d), p(out)), (p(rgba), 2049, p(d), p(out))):
        assert L.rt3_debug_environment_lookup(*args) == -1, args
    assert out.tolist() == [7, 7, 7]                                    # a refused call writes nothing
    big = np.zeros((6, 2048, 2048, 4), np.float32)                      # the largest map: the last texel of the last face
    big[5, 2047, 2047, :3] = (1, 2, 3)
    corner = np.array([-1.0, -1.0, -1.0 - 2.0 ** -20], np.float32)      # face -Z, sc = +1 (x = -1), tc = +1 (y = -1)
    assert L.rt3_debug_environment_lookup(p(big), 2048, p(corner), p(out)) == 0 and out.tolist() == [1, 2, 3]


def calls(ctx):
    rgba = np.ones((6, 2, 2, 4), np.float32)
    r = rgba.ctypes.data_as(C.c_void_p)
    return rgba, (("rt3_set_environment", (ctx, r, 2)), ("rt3_set_environment", (ctx, None, 0)), ("rt3_set_environment_device", (ctx, r, 2, None)),
                  ("rt3_set_environment_device", (ctx, None, 0, None)), ("rt3_clear_environment", (ctx,)))


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    keep, table = calls(None)
    for name, args in table:
        assert getattr(L, name)(*args) == -1, name                      # RT3_E_ARG, as every entry point refuses a NULL context
    assert L.rt3_environment_size(None) == 0
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    keep, table = calls(C.c_void_p(0x10))                               # never dereferenced by a stub
    for name, args in table:
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args) == -2, name                                    # RT3_E_DEVICE
    S.rt3_environment_size.restype = C.c_uint32
    assert S.rt3_environment_size(C.c_void_p(0x10)) == 0


def test_no_renderer_without_a_device(rt3):
    import torch
    if torch.cuda.is_available():
        return                                                          # (the GPU suite covers the calls themselves)
    with pytest.raises(rt3.Fatal, match="no CPU fallback"):
        rt3.initialize_renderer(0).set_environment(np.ones((6, 1, 1, 3), np.float32))


@pytest.mark.parametrize("args,message", [
    (("--env", "e.pfm", "o.png"), "--env needs the path tracer (Mode X): pass --spp."),
    (("--scene", "three", "--spp", "4", "o.png", "--env"), "--env has no value."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_help_lists_the_option():
    rc, out, err = run("-h")
    assert rc == 0 and "--env" in out and "6N high" in out
