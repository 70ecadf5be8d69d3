"""Lens sequences (rt3_denoise_temporal_optic*, rt3_motion_optic*, rt3_debug_turns, rt3_debug_optic_pixel) without a GPU: header /
binding / library coverage with the declared signatures, the Python and C++ surfaces, the NULL context, the "no device" stubs, properties of the
numpy restatement (tests/optic_ref.py) alone, and the command line's --lens-frames."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import optic_ref as O
from test_cli import run
from test_denoise_abi import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TEMPORAL = ["rt3_ctx*", "uint32_t", "uint32_t", "constrt3_lens*", "constfloat*", "constrt3_aov*", "constrt3_lens*", "constrt3_history*", "constfloat*",
            "constrt3_temporal_params*", "float*", "rt3_history*"]
TEMPORAL_DEVICE = ["rt3_ctx*", "uint32_t", "uint32_t", "constrt3_lens*", "constvoid*", "constvoid*", "constrt3_lens*", "constvoid*", "constvoid*",
                   "constrt3_temporal_params*", "void*", "void*", "void*"]
# name -> (result, the parameter types of the declaration in include/rt3.h, spaces removed)
DECLARED = {
    "rt3_denoise_temporal_optic": ("int", TEMPORAL),
    "rt3_denoise_temporal_optic_device": ("int", TEMPORAL_DEVICE),
    "rt3_motion_optic": ("int", ["rt3_ctx*", "uint32_t", "uint32_t", "constrt3_lens*", "constrt3_aov*", "constfloat*", "uint32_t", "constfloat*", "uint32_t",
                                 "float*"]),
    "rt3_motion_optic_device": ("int", ["rt3_ctx*", "uint32_t", "uint32_t", "constrt3_lens*", "constvoid*", "constvoid*", "uint32_t", "constvoid*", "uint32_t",
                                        "void*", "void*"]),
    "rt3_debug_turns": ("float", ["float", "float"]),
    "rt3_debug_optic_pixel": ("int", ["constrt3_lens*", "uint32_t", "uint32_t", "constfloat", "uint32_t", "float", "uint32_t*", "uint32_t*"]),
}


def header_declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt3.h")).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|float)\s+(rt3_[a-z_]*optic[a-z_]*|rt3_debug_turns)\s*\(([^)]*)\)\s*;", text):
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
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    for s, (res, types) in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        assert "lens" not in s                                            # (the set of rt3_*lens* declarations is pinned by the lens models' tests)
        fn = getattr(L, s)
        assert fn.restype is (C.c_int if res == "int" else C.c_float), s
        want = [C.c_void_p if ("*" in t or t in ("constfloat", "float") and s == "rt3_debug_optic_pixel") else ctype[t] for t in types]
        assert list(fn.argtypes) == want, s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3            # additions only
    assert "RT3_ABI_VERSION 3u" in open(os.path.join(ROOT, "include", "rt3.h")).read()
    assert C.sizeof(rt3.rt3_lens) == 80 and C.sizeof(rt3.TEMPORAL_PARAMS) == 32 and rt3.HISTORY.itemsize == 48


def test_python_and_cpp_surfaces(rt3):
    temporal = inspect.signature(rt3.HipRenderer.denoise_temporal_lens)
    assert list(temporal.parameters) == ["self", "colour", "aov", "lens", "prev", "motion", "iterations", "normal_power", "sigma_luminance", "sigma_depth",
                                         "alpha", "moments_alpha", "depth_tolerance", "normal_tolerance"]
    old = inspect.signature(rt3.HipRenderer.denoise_temporal)
    for k in ("iterations", "normal_power", "sigma_luminance", "sigma_depth", "alpha", "moments_alpha", "depth_tolerance", "normal_tolerance", "prev", "motion"):
        assert temporal.parameters[k].default == old.parameters[k].default, k
    assert list(old.parameters)[-1] == "motion"                          # the camera's method is as it was
    assert list(inspect.signature(rt3.HipRenderer.motion_lens).parameters) == ["self", "aov", "lens", "prev_center_radius", "prev_vertices"]
    assert list(inspect.signature(rt3.turns).parameters) == ["c", "s"]
    sig = inspect.signature(rt3.lens_pixel)
    assert list(sig.parameters) == ["prev_lens", "width", "height", "r", "is_hit"] and sig.parameters["is_hit"].default is True
    assert float(rt3.turns(0.0, 1.0)) == 0.25 and np.isnan(rt3.turns(0.0, 0.0))
    text = open(os.path.join(ROOT, "raytracer-3_amd", "host", "renderer", "Renderer.hpp")).read()
    assert re.search(r"std::vector<float>\s+denoise_temporal_lens\s*\(\s*const rt3_lens&", text)
    assert re.search(r"std::vector<float>\s+motion_lens\s*\(\s*const rt3_lens&", text) and "struct LensHistory" in text
    api = open(os.path.join(ROOT, "raytracer-3_amd", "host", "HostApi.cpp")).read()
    assert "HipRenderer::denoise_temporal_lens(" in api and "HipRenderer::motion_lens(" in api
    assert "rt3_denoise_temporal_optic(" in api and "rt3_motion_optic(" in api


def calls(rt3, ctx):
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(5, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9)
    lens = rt3.make_lens("equirect", (0, 0, 0), (0, 0, -1))
    buf = np.zeros(256, np.float32)
    b = buf.ctypes.data_as(C.c_void_p)
    keep = (p, lens, buf)
    l = C.byref(lens)
    return keep, (("rt3_motion_optic", (ctx, 2, 2, l, b, None, 0, None, 0, b)),
                  ("rt3_motion_optic_device", (ctx, 2, 2, l, b, None, 0, None, 0, b, None)),
                  ("rt3_denoise_temporal_optic", (ctx, 2, 2, l, b, b, None, None, b, C.byref(p), b, b)),
                  ("rt3_denoise_temporal_optic_device", (ctx, 2, 2, l, b, b, None, None, b, C.byref(p), b, b, None)),
                  ("rt3_denoise_temporal_optic", (ctx, 2, 2, None, None, None, None, None, None, None, None, None)))


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


def test_host_functions_refuse_bad_arguments(rt3):
    L = rt3.lib()
    lens = rt3.make_lens("fisheye", (0, 0, 0), (0, 0, -1))
    r = np.array([0.1, 0.2, -1.0], F)
    out, face, valid = np.zeros(3, F), C.c_uint32(7), C.c_uint32(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)       # noqa: E731
    good = (C.byref(lens), 8, 4, p(r), 1, p(out), C.byref(face), C.byref(valid))
    assert L.rt3_debug_optic_pixel(*good) == 0 and valid.value == 1 and face.value == 0
    for i in (0, 3, 5, 6, 7):
        bad = list(good)
        bad[i] = None
        assert L.rt3_debug_optic_pixel(*bad) == -1, i
    assert L.rt3_debug_optic_pixel(C.byref(lens), 1, 4, *good[3:]) == -1 and L.rt3_debug_optic_pixel(C.byref(lens), 8, 1, *good[3:]) == -1
    lens.half_fov_turns = 0.75
    assert L.rt3_debug_optic_pixel(*good) == -1                          # a lens the entry points refuse
    cube = rt3.make_lens("cube", (0, 0, 0), (0, 0, -1))
    assert L.rt3_debug_optic_pixel(C.byref(cube), 4, 24, *good[3:]) == 0 and L.rt3_debug_optic_pixel(C.byref(cube), 4, 20, *good[3:]) == -1


def test_no_renderer_without_a_device(rt3):
    import torch
    if torch.cuda.is_available():
        return                                                         # (the GPU suite covers the calls themselves)
    colour, aov = synthetic(rt3, 4, 8, 1)
    with pytest.raises(rt3.Fatal, match="no CPU fallback"):
        rt3.initialize_renderer(0).denoise_temporal_lens(colour, aov, rt3.make_lens("equirect", (0, 0, 0), (0, 0, -1)))


# ------------------------------------------------------------------------------------------------ the numpy restatement alone
@pytest.mark.parametrize("model,size", [("equirect", (12, 9)), ("fisheye", (12, 9)), ("ortho", (12, 9)), ("cube", (3, 18))])
def test_restatement_shortcut_and_zero_plane(rt3, model, size):
    """An equal lens keeps every pixel in place (length 2 everywhere the history is consistent); pads and other models' fields do not break the
    equality; an all-zero motion plane changes nothing; without a previous frame the plane is not read."""
    w, h = size
    lens = rt3.make_lens(model, (0.3, 1.1, 2.0), (-0.2, 0.4, -1.0), (0.1, 1.0, 0.05), fov_deg=200.0, extent=(3.0, 1.75))
    c0, a0 = synthetic(rt3, h, w, 31)
    c1, a1 = synthetic(rt3, h, w, 32)
    a1["depth"], a1["normal"] = a0["depth"], a0["normal"]
    kw = dict(normal_tolerance=-1.0)                                   # (the synthetic normals are not unit vectors)
    _, h0 = O.denoise_temporal_lens(c0, a0, lens, None, **kw)
    assert (h0["length"] == 1).all()
    twin = rt3.rt3_lens.from_buffer_copy(bytes(lens))
    twin._pad0, twin._pad2 = 3.0, -1.0
    if model != "fisheye":
        twin.half_fov_turns = 0.125
    if model != "ortho":
        twin.half_extent[0] = 9.0
    assert O.same_optic(lens, twin)
    want, wh = O.denoise_temporal_lens(c1, a1, lens, (h0, lens), **kw)
    assert (wh["length"] == 2).all()
    zero = np.zeros((h, w, 4), F)
    for prev_lens, plane in ((twin, None), (lens, zero), (twin, zero)):
        got, gh = O.denoise_temporal_lens(c1, a1, lens, (h0, prev_lens), motion=plane, **kw)
        assert got.tobytes() == want.tobytes() and gh.tobytes() == wh.tobytes()
    other = rt3.rt3_lens.from_buffer_copy(bytes(lens))
    other.origin[0] += 0.25
    assert not O.same_optic(lens, other)
    first, fh = O.denoise_temporal_lens(c0, a0, lens, None, motion=zero, **kw)
    assert fh.tobytes() == h0.tobytes()


# ------------------------------------------------------------------------------------------------ the command line
@pytest.mark.parametrize("args,message", [
    (("--scene", "weekend", "--spp", "1", "--lens-frames", "3", "o.png"), "--lens-frames needs --lens: a camera sequence is --frames."),
    (("--scene", "weekend", "--spp", "1", "--lens", "equirect", "--lens-frames", "0", "o.png"), "--lens-frames must be at least 1."),
    (("--scene", "weekend", "--spp", "1", "--lens", "equirect", "--lens-frames", "x", "o.png"), "Invalid lens-frames 'x'"),
    (("--scene", "weekend", "--spp", "1", "--lens", "equirect", "o.png", "--lens-frames"), "--lens-frames has no value."),
    (("--scene", "three", "--spp", "4", "--lens", "equirect", "--frames", "2", "--lens-frames", "2", "o.png"),
     "--lens renders one frame: it is not available with --frames."),
    (("--scene", "weekend", "--spp", "1", "--lens", "equirect", "--lens-frames", "1", "--slide", "0.1,0,0", "o.png"),
     "--slide needs a sequence: pass --frames N with N of at least 2."),
    (("--lens", "equirect", "--lens-frames", "2", "o.png"), "--lens needs the path tracer (Mode X): pass --spp."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_accepts_the_option_and_then_needs_a_device(tmp_path):
    import torch
    if torch.cuda.is_available():
        return
    rc, out, err = run("--scene", "weekend", "--spp", "1", "-W", "32", "-H", "16", "--lens", "equirect", "--lens-frames", "3", "--orbit", "1.5",
                       "--slide", "0.1,0,0", "--refit", "--denoise", str(tmp_path / "P"), str(tmp_path / "o.ppm"), "-f", "ppm")
    assert rc == -1 and "fatal:" in err and "--lens" not in err and "--slide" not in err, err


def test_cli_help_lists_the_new_option():
    rc, out, err = run("-h")
    assert rc == 0 and "--lens-frames" in out
