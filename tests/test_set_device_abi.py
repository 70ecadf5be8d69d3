"""rt3_set_spheres_device / rt3_set_mesh_device without a GPU: header / binding / library coverage with the declared
signatures, the Python methods, the NULL context and the "no device" stubs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (result, the parameter types of the declaration in include/rt3.h, spaces removed; an array parameter is a pointer)
DECLARED = {
    "rt3_set_spheres_device": ("int", ["rt3_ctx*", "constvoid*", "constvoid*", "uint32_t", "void*"]),
    "rt3_set_mesh_device": ("int", ["rt3_ctx*", "constvoid*", "uint32_t", "constvoid*", "uint32_t", "constvoid*", "void*"]),
    "rt3_debug_sphere_plan": ("uint32_t", ["constfloat*", "uint32_t", "float*", "uint32_t*"]),
    "rt3_debug_sphere_build": ("int", ["rt3_ctx*", "float*", "uint32_t*", "uint32_t*"]),
}


def header_declarations():
    text = open(os.path.join(ROOT, "include", "rt3.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|uint32_t)\s+(rt3_set_(?:spheres|mesh)_device|rt3_debug_sphere_(?:plan|build))\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = a.strip()
            if "[" in a:
                a = a[:a.index("[")].rsplit(None, 1)[0] + "*"
            types.append(re.sub(r"\s+", "", a[:a.rindex("*") + 1] if "*" in a else a.rsplit(None, 1)[0]))
        out[name] = (res, types)
    return out


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    assert header_declarations() == DECLARED
    vp, u32 = C.c_void_p, C.c_uint32
    ctype = {"rt3_ctx*": vp, "void*": vp, "constvoid*": vp, "constfloat*": vp, "float*": vp, "uint32_t*": vp, "uint32_t": u32}
    for s, (res, types) in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is (C.c_int if res == "int" else u32) and list(fn.argtypes) == [ctype[t] for t in types], s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3
    assert "RT3_ABI_VERSION 3u" in open(os.path.join(ROOT, "include", "rt3.h")).read()


def test_python_methods(rt3):
    sig = inspect.signature(rt3.HipRenderer.set_spheres)
    assert list(sig.parameters) == ["self", "center_radius", "materials"]
    sig = inspect.signature(rt3.HipRenderer.set_mesh)
    assert list(sig.parameters) == ["self", "faces", "verts", "face_materials"] and sig.parameters["face_materials"].default is None
    assert list(inspect.signature(rt3.HipRenderer.sphere_build).parameters) == ["self"]
    assert list(inspect.signature(rt3.sphere_plan).parameters) == ["center_radius"]


def calls(ctx):
    keep = (np.zeros(4, np.float32), np.zeros(4, np.uint32), C.c_uint32(0))
    c, d = (a.ctypes.data_as(C.c_void_p) for a in keep[:2])
    return keep, (("rt3_set_spheres_device", (ctx, None, None, 0, None)), ("rt3_set_spheres_device", (ctx, c, c, 1, None)),
                  ("rt3_set_mesh_device", (ctx, None, 0, None, 0, None, None)), ("rt3_debug_sphere_build", (ctx, c, d, C.byref(keep[2]))))


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
    assert not hasattr(S, "rt3_debug_sphere_plan")                     # host code: the sanitizer build links the library's own (rt3_host.cpp)


def test_the_host_probe_needs_no_device(rt3):
    centre, direct = rt3.sphere_plan(np.array([[1.0, 2.0, 3.0, 0.5], [5.0, 6.0, 7.0, 0.5], [9.0, 9.0, 9.0, 0.5]], np.float32))
    assert centre.tolist() == [5.0, 6.0, 7.0] and direct.dtype == np.uint32
    out = np.full(4, 7, np.uint32)
    cen = np.ones(3, np.float32)
    assert rt3.lib().rt3_debug_sphere_plan(None, 0, cen.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    assert not cen.any() and (out == 0xFFFFFFFF).all()
