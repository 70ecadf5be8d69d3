"""Lens models (rt3_lens_rays*, rt3_render_lens*, rt3_render_lens_aov*) without a GPU: the wire struct three ways, header / binding /
library coverage with the declared signatures, the Python surface, the NULL context, the "no device" stubs, and the command line's --lens."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = [("model", 0), ("half_fov_turns", 4), ("half_extent", 8), ("origin", 16), ("_pad0", 28), ("right", 32), ("_pad1", 44), ("up", 48),
           ("_pad2", 60), ("forward", 64), ("_pad3", 76)]
# name -> (result, the parameter types of the declaration in include/rt3.h, spaces removed)
DECLARED = {
    "rt3_lens_look_at": ("void", ["rt3_lens*", "uint32_t", "constfloat", "constfloat", "constfloat"]),
    "rt3_lens_rays": ("int", ["rt3_ctx*", "constrt3_lens*", "constrt3_params*", "uint32_t", "uint32_t", "rt3_ray*"]),
    "rt3_lens_rays_device": ("int", ["rt3_ctx*", "constrt3_lens*", "constrt3_params*", "uint32_t", "uint32_t", "void*", "void*"]),
    "rt3_render_lens": ("int", ["rt3_ctx*", "constrt3_lens*", "constrt3_params*", "uint32_t", "uint32_t", "float*"]),
    "rt3_render_lens_device": ("int", ["rt3_ctx*", "constrt3_lens*", "constrt3_params*", "uint32_t", "uint32_t", "void*", "void*"]),
    "rt3_render_lens_aov": ("int", ["rt3_ctx*", "constrt3_lens*", "constrt3_params*", "rt3_aov*"]),
    "rt3_render_lens_aov_device": ("int", ["rt3_ctx*", "constrt3_lens*", "constrt3_params*", "void*", "void*"]),
    "rt3_debug_lens_ray": ("int", ["constrt3_lens*", "constrt3_params*", "uint32_t", "uint32_t", "uint32_t", "rt3_ray*"]),
}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt3.h")).read(), flags=re.S)


def header_declarations():
    out = {}
    for res, name, args in re.findall(r"\b(int|void)\s+(rt3_[a-z_]*lens[a-z_]*)\s*\(([^)]*)\)\s*;", header_text()):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(re.sub(r"\s+", "", a[:a.rindex("*") + 1] if "*" in a else a[:a.rindex(" ")]))
        out[name] = (res, types)
    return out


def test_the_wire_struct_is_80_bytes_here_in_the_header_and_in_the_library(rt3, tmp_path):
    P = rt3.rt3_lens
    assert C.sizeof(P) == 80 and rt3.LENS.itemsize == 80
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == OFFSETS
    assert [(n, rt3.LENS.fields[n][1]) for n in rt3.LENS.names] == OFFSETS
    assert (rt3.LENS_EQUIRECT, rt3.LENS_FISHEYE, rt3.LENS_ORTHO, rt3.LENS_CUBE) == (1, 2, 3, 4)
    text = open(os.path.join(ROOT, "include", "rt3.h")).read()
    for name, value in (("EQUIRECT", 1), ("FISHEYE", 2), ("ORTHO", 3), ("CUBE", 4)):
        assert re.search(r"#define\s+RT3_LENS_%s\s+%du\b" % (name, value), text), name
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rt3.h"\n_Static_assert(sizeof(rt3_lens) == 80, "size");\n' +
                   "".join('_Static_assert(offsetof(rt3_lens, %s) == %d, "%s");\n' % (n, o, n) for n, o in OFFSETS) +
                   '_Static_assert(sizeof(rt3_params) == 44, "rt3_params");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")])
    device = open(os.path.join(ROOT, "raytracer-3_amd", "csrc", "rt3_device.hip")).read()
    assert 'static_assert(sizeof(rt3_lens) == 80, "rt3.h: rt3_lens");' in device


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    assert header_declarations() == DECLARED
    for s, (res, types) in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        assert "environment" not in s
        fn = getattr(L, s)
        assert fn.restype is (C.c_int if res == "int" else None), s
        assert list(fn.argtypes) == [C.c_uint32 if t == "uint32_t" else C.c_void_p for t in types], s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3            # additions only: every existing struct is unchanged
    assert "RT3_ABI_VERSION 3u" in open(os.path.join(ROOT, "include", "rt3.h")).read()
    assert C.sizeof(rt3.rt3_params) == 44


def test_python_surface(rt3):
    sig = inspect.signature(rt3.make_lens)
    assert list(sig.parameters) == ["model", "origin", "at", "vup", "fov_deg", "extent"]
    assert sig.parameters["fov_deg"].default == 180.0 and sig.parameters["extent"].default == (1.0, 1.0)
    assert list(inspect.signature(rt3.lens_ray).parameters) == ["lens", "params", "x", "y", "s"]
    for name, params in (("lens_rays", ["self", "lens", "params", "sample_begin", "sample_count", "device"]),
                         ("render_lens", ["self", "lens", "params", "sample_begin", "sample_count", "device"]),
                         ("render_lens_aov", ["self", "lens", "params", "device"]),
                         ("lens_rays_device", ["self", "lens", "params", "sample_begin", "sample_count", "d_out_ptr", "stream_ptr"]),
                         ("render_lens_device", ["self", "lens", "params", "sample_begin", "sample_count", "d_out_ptr", "stream_ptr"]),
                         ("render_lens_aov_device", ["self", "lens", "params", "d_out_ptr", "stream_ptr"])):
        assert list(inspect.signature(getattr(rt3.HipRenderer, name)).parameters) == params, name
    with pytest.raises(rt3.Fatal, match="equirect"):
        rt3.make_lens("pinhole", (0, 0, 0), (0, 0, -1))
    lens = rt3.make_lens("ortho", (1, 2, 3), (1, 2, 2), extent=(4.0, 3.0))
    assert lens.model == rt3.LENS_ORTHO and list(lens.half_extent) == [2.0, 1.5] and list(lens.origin) == [1.0, 2.0, 3.0]
    text = open(os.path.join(ROOT, "raytracer-3_amd", "host", "renderer", "Renderer.hpp")).read()
    assert re.search(r"std::vector<float>\s+render_lens\s*\(\s*const rt3_lens&", text) and re.search(r"std::vector<rt3_aov>\s+lens_aov\s*\(\s*const rt3_lens&", text)


def calls(rt3, ctx):
    lens = rt3.make_lens("equirect", (0, 0, 0), (0, 0, -1))
    p = rt3.make_params(8, 4, spp=2, max_depth=3)
    out = np.zeros(8 * 4 * 2 * 12, np.float32)
    o = out.ctypes.data_as(C.c_void_p)
    keep = (lens, p, out)
    l, q = C.byref(lens), C.byref(p)
    return keep, (("rt3_lens_rays", (ctx, l, q, 0, 2, o)), ("rt3_lens_rays_device", (ctx, l, q, 0, 2, o, None)),
                  ("rt3_render_lens", (ctx, l, q, 0, 2, o)), ("rt3_render_lens_device", (ctx, l, q, 0, 2, o, None)),
                  ("rt3_render_lens_aov", (ctx, l, q, o)), ("rt3_render_lens_aov_device", (ctx, l, q, o, None)),
                  ("rt3_render_lens", (ctx, None, None, 0, 0, None)), ("rt3_render_lens_aov_device", (ctx, None, None, None, None)))


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    keep, table = calls(rt3, None)
    for name, args in table:
        assert getattr(L, name)(*args) == -1, name                    # RT3_E_ARG, as every entry point refuses a NULL context
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
        rt3.initialize_renderer(0).render_lens(rt3.make_lens("equirect", (0, 0, 0), (0, 0, -1)), rt3.make_params(8, 4))


@pytest.mark.parametrize("args,message", [
    (("--scene", "weekend", "--lens", "equirect", "o.png"), "--lens needs the path tracer (Mode X): pass --spp."),
    (("--lens", "fisheye", "o.png"), "--lens needs the path tracer (Mode X): pass --spp."),
    (("--scene", "three", "--spp", "16", "--lens", "equirect", "--adaptive", "0.05", "o.png"), "--lens is not available with --adaptive."),
    (("--scene", "three", "--spp", "4", "--lens", "equirect", "--frames", "2", "o.png"), "--lens renders one frame: it is not available with --frames."),
    (("--scene", "three", "--spp", "4", "--lens", "ortho", "--gpus", "2", "o.png"), "--lens renders on one device: it is not available with --gpus above 1."),
    (("--scene", "three", "--spp", "4", "--lens", "cube", "-W", "16", "-H", "90", "o.png"), "--lens cube needs a frame of six stacked faces: -H must be 6 times -W."),
    (("--scene", "three", "--spp", "4", "--lens", "pinhole", "o.png"), "Unknown lens 'pinhole'"),
    (("--scene", "three", "--spp", "4", "--lens-fov", "90", "o.png"), "--lens-fov and --lens-extent need --lens."),
    (("--scene", "three", "--spp", "4", "--lens", "fisheye", "--lens-fov", "0", "o.png"), "Invalid lens-fov '0'"),
    (("--scene", "three", "--spp", "4", "--lens", "fisheye", "--lens-fov", "361", "o.png"), "Invalid lens-fov '361'"),
    (("--scene", "three", "--spp", "4", "--lens", "ortho", "--lens-extent", "2", "o.png"), "Invalid lens-extent '2'"),
    (("--scene", "three", "--spp", "4", "--lens", "ortho", "--lens-extent", "2,0", "o.png"), "Invalid lens-extent '2,0'"),
    (("--scene", "three", "--spp", "4", "o.png", "--lens"), "--lens has no value."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_accepts_the_options_and_then_needs_a_device(tmp_path):
    import torch
    if torch.cuda.is_available():
        return
    rc, out, err = run("--scene", "three", "--spp", "4", "-W", "16", "-H", "96", "--lens", "cube", "--hdr", str(tmp_path / "h.pfm"),
                       str(tmp_path / "o.ppm"), "-f", "ppm")
    assert rc == -1 and "fatal:" in err and "--lens" not in err, err


def test_cli_help_lists_the_new_options():
    rc, out, err = run("-h")
    assert rc == 0 and "--lens" in out and "--lens-fov" in out and "--lens-extent" in out and "equirect | fisheye | ortho | cube" in out
