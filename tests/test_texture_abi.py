"""Image textures (rt3_set_texture*, rt3_bind_*_textures*) without a GPU: header / binding / library coverage with the declared
signatures, the constants, the Python surface, the refusals of the host-only law functions, the NULL context, the "no device" stubs and the command
line's --texture / --bind-sphere."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (result, the parameter types of the declaration in include/rt3.h, spaces removed; an array parameter is a pointer on the wire)
DECLARED = {
    "rt3_set_texture": ("int", ["rt3_ctx*", "uint32_t", "constfloat*", "uint32_t", "uint32_t", "uint32_t"]),
    "rt3_set_texture_device": ("int", ["rt3_ctx*", "uint32_t", "constvoid*", "uint32_t", "uint32_t", "uint32_t", "void*"]),
    "rt3_clear_textures": ("int", ["rt3_ctx*"]),
    "rt3_texture_size": ("int", ["rt3_ctx*", "uint32_t", "uint32_t*", "uint32_t*", "uint32_t*"]),
    "rt3_bind_sphere_textures": ("int", ["rt3_ctx*", "constuint32_t*", "uint32_t"]),
    "rt3_bind_sphere_textures_device": ("int", ["rt3_ctx*", "constvoid*", "uint32_t", "void*"]),
    "rt3_bind_mesh_textures": ("int", ["rt3_ctx*", "constuint32_t*", "constfloat*", "uint32_t"]),
    "rt3_bind_mesh_textures_device": ("int", ["rt3_ctx*", "constvoid*", "constvoid*", "uint32_t", "void*"]),
    "rt3_debug_texture_lookup": ("int", ["constfloat*", "uint32_t", "uint32_t", "uint32_t", "constfloat", "float"]),
    "rt3_debug_texture_sphere_uv": ("int", ["constfloat", "float"]),
    "rt3_debug_texture_face_uv": ("int", ["constfloat", "constfloat", "constfloat", "constfloat", "constfloat", "float"]),
}


def header_declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt3.h")).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|uint32_t)\s+(rt3_[a-z_]*texture[a-z_]*)\s*\(([^)]*)\)\s*;", text):
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
        assert fn.restype is C.c_int, s
        assert list(fn.argtypes) == [C.c_uint32 if t == "uint32_t" else C.c_void_p for t in types], s       # struct-free: words and pointers only
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3            # additions only: every existing struct is unchanged
    header = open(os.path.join(ROOT, "include", "rt3.h")).read()
    for line in ("RT3_ABI_VERSION 3u", "#define RT3_TEX_MAX_TEXTURES 256u", "#define RT3_TEX_MAX_SIDE     8192u", "#define RT3_TEX_NONE         0xFFFFFFFFu",
                 "#define RT3_TEX_REPEAT       0u", "#define RT3_TEX_CLAMP        1u"):
        assert line in header, line
    assert (rt3.TEX_MAX_TEXTURES, rt3.TEX_MAX_SIDE, rt3.TEX_NONE, rt3.TEX_REPEAT, rt3.TEX_CLAMP) == (256, 8192, 0xFFFFFFFF, 0, 1)
    for phrase in ("mip levels", "8-bit or compressed texels", "normal, roughness and emission-only maps", "`vt` from OBJ", "SceneLang syntax",
                   "textures under the two sampling flags", "a per-axis wrap mode"):
        assert phrase in header, phrase                                 # the header says what is out of scope


def test_python_surface(rt3):
    H = rt3.HipRenderer
    assert list(inspect.signature(H.set_texture).parameters) == ["self", "slot", "image", "wrap"]
    assert inspect.signature(H.set_texture).parameters["wrap"].default == "repeat"
    assert list(inspect.signature(H.clear_textures).parameters) == ["self"]
    assert list(inspect.signature(H.texture_size).parameters) == ["self", "slot"]
    assert list(inspect.signature(H.bind_sphere_textures).parameters) == ["self", "slots"]
    assert list(inspect.signature(H.bind_mesh_textures).parameters) == ["self", "slots", "uv"]
    assert list(inspect.signature(rt3.texture_lookup).parameters) == ["image", "uv", "wrap"]
    assert list(inspect.signature(rt3.texture_sphere_uv).parameters) == ["n"]
    assert list(inspect.signature(rt3.texture_face_uv).parameters) == ["p1", "p2", "p3", "uv6", "p"]
    for bad in (np.zeros((2, 2)), np.zeros((2, 2, 2)), np.zeros((0, 2, 4)), np.zeros((2, 2, 2, 4))):
        with pytest.raises(rt3.Fatal):
            rt3.texture_lookup(bad, [0.5, 0.5])
    with pytest.raises(rt3.Fatal, match="repeat"):
        rt3.texture_lookup(np.ones((2, 2, 3)), [0.5, 0.5], wrap="mirror")


def test_the_host_law_refuses_bad_arguments(rt3):
    L = rt3.lib()
    rgba = np.ones((2, 2, 4), np.float32)
    uv = np.array([0.5, 0.5], np.float32)
    out = np.full(3, 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                          # noqa: E731
    assert L.rt3_debug_texture_lookup(p(rgba), 2, 2, 0, p(uv), p(out)) == 0 and out.tolist() == [1, 1, 1]
    out[:] = 7.0
    for args in ((None, 2, 2, 0, p(uv), p(out)), (p(rgba), 2, 2, 0, None, p(out)), (p(rgba), 2, 2, 0, p(uv), None), (p(rgba), 0, 2, 0, p(uv), p(out)),
                 (p(rgba), 2, 0, 0, p(uv), p(out)), (p(rgba), 8193, 1, 0, p(uv), p(out)), (p(rgba), 1, 8193, 0, p(uv), p(out)),
                 (p(rgba), 8192, 8193, 0, p(uv), p(out)), (p(rgba), 8192, 8192 + 1, 1, p(uv), p(out)), (p(rgba), 2, 2, 2, p(uv), p(out))):
        assert L.rt3_debug_texture_lookup(*args) == -1, args
    assert L.rt3_debug_texture_lookup(p(rgba), 8200, 8192, 0, p(uv), p(out)) == -1     # (a side over the limit; 8192 x 8192 = 2^26 is the largest area)
    assert out.tolist() == [7, 7, 7]                                    # a refused call writes nothing
    n = np.array([0, 1, 0], np.float32)
    two = np.zeros(2, np.float32)
    assert L.rt3_debug_texture_sphere_uv(None, p(two)) == -1 and L.rt3_debug_texture_sphere_uv(p(n), None) == -1
    six = np.zeros(6, np.float32)
    good = [p(n), p(n), p(n), p(six), p(n), p(two)]
    assert L.rt3_debug_texture_face_uv(*good) == 0
    for k in range(6):
        args = list(good)
        args[k] = None
        assert L.rt3_debug_texture_face_uv(*args) == -1, k


def test_the_largest_texture_reads_its_last_texel(rt3):
    """8192 x 8192 texels = 2^26, the largest area: the index arithmetic reaches the last texel, whose byte offset is just below 2^30."""
    w = h = 8192
    fn = rt3.lib().rt3_debug_texture_lookup
    big = np.zeros((h, w, 4), np.float32)                               # (zero pages until written: one texel is)
    big[h - 1, w - 1, :3] = (1, 2, 3)
    out = np.zeros(3, np.float32)
    uv = np.array([1.0, 1.0], np.float32)
    assert fn(big.ctypes.data_as(C.c_void_p), w, h, 1, uv.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0 and out.tolist() == [1, 2, 3]


def calls(ctx):
    rgba = np.ones((2, 2, 4), np.float32)
    slots = np.zeros(4, np.uint32)
    uv6 = np.zeros(24, np.float32)
    r, s, u = (a.ctypes.data_as(C.c_void_p) for a in (rgba, slots, uv6))
    w = C.c_uint32(0)
    return (rgba, slots, uv6, w), (
        ("rt3_set_texture", (ctx, 0, r, 2, 2, 0)), ("rt3_set_texture", (ctx, 0, None, 0, 0, 0)), ("rt3_set_texture_device", (ctx, 0, r, 2, 2, 0, None)),
        ("rt3_clear_textures", (ctx,)), ("rt3_texture_size", (ctx, 0, C.byref(w), C.byref(w), C.byref(w))),
        ("rt3_bind_sphere_textures", (ctx, s, 4)), ("rt3_bind_sphere_textures", (ctx, None, 0)), ("rt3_bind_sphere_textures_device", (ctx, s, 4, None)),
        ("rt3_bind_mesh_textures", (ctx, s, u, 4)), ("rt3_bind_mesh_textures", (ctx, None, None, 0)), ("rt3_bind_mesh_textures_device", (ctx, s, u, 4, None)))


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    keep, table = calls(None)
    for name, args in table:
        assert getattr(L, name)(*args) == -1, name                      # RT3_E_ARG, as every entry point refuses a NULL context
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    keep, table = calls(C.c_void_p(0x10))                               # never dereferenced by a stub
    for name, args in table:
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args) == -2, name                                    # RT3_E_DEVICE


def test_no_renderer_without_a_device(rt3):
    import torch
    if torch.cuda.is_available():
        return                                                          # (the GPU suite covers the calls themselves)
    with pytest.raises(rt3.Fatal, match="no CPU fallback"):
        rt3.initialize_renderer(0).set_texture(0, np.ones((1, 1, 3), np.float32))


@pytest.mark.parametrize("args,message", [
    (("--texture", "t.pfm", "o.png"), "--texture and --bind-sphere need the path tracer (Mode X): pass --spp."),
    (("--scene", "three", "--spp", "4", "o.png", "--texture"), "--texture has no value."),
    (("--scene", "cornell", "--spp", "4", "--texture", "t.pfm", "o.png"), "--texture and --bind-sphere need a sphere scene (three, weekend, stress100k)."),
    (("--scene", "three", "--spp", "4", "--texture", "t.pfm,mirror", "o.png"), "Invalid texture wrap 'mirror'"),
    (("--scene", "three", "--spp", "4", "--texture", "t.pfm", "--bind-sphere", "all", "o.png"), "Invalid bind-sphere 'all'"),
    (("--scene", "three", "--spp", "4", "--texture", "t.pfm", "--bind-sphere", "x=0", "o.png"), "Invalid bind-sphere 'x=0'"),
    (("--scene", "three", "--spp", "4", "--texture", "t.pfm", "--bind-sphere", "0=256", "o.png"), "Invalid bind-sphere '0=256'"),
    (("--scene", "three", "--spp", "4", "--texture", "t.pfm", "--bind-sphere", "0=1", "o.png"), "--bind-sphere names a slot that no --texture fills."),
    (("--scene", "three", "--spp", "4", "--bind-sphere", "all=0", "o.png"), "--bind-sphere names a slot that no --texture fills."),
    (("--scene", "three", "--spp", "4", "--texture", "t.pfm", "--light-sampling", "o.png"), "--texture is not available with --env-sampling or --light-sampling."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_help_lists_the_options():
    rc, out, err = run("-h")
    assert rc == 0 and "--texture" in out and "--bind-sphere" in out and "FILE.pfm[,repeat|clamp]" in out and "INDEX=SLOT or all=SLOT" in out
