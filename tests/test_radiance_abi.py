"""Radiance along caller-supplied rays (rt3_radiance*) without a GPU: the wire struct, header / binding / library coverage with
the declared signatures, the Python methods, the NULL context, the "no device" behaviour every device entry point shares, and the command
line's --rays / --radiance."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("uint32_t", "max_depth"), ("uint32_t", "seed"), ("uint32_t", "flags"), ("uint32_t", "sample_begin"), ("uint32_t", "sample_count"),
          ("float", "t_min")]
# name -> the parameter types of the declaration in include/rt3.h, spaces removed
DECLARED = {
    "rt3_radiance": ["rt3_ctx*", "constrt3_ray*", "constuint32_t*", "uint32_t", "constrt3_radiance_params*", "float*"],
    "rt3_radiance_device": ["rt3_ctx*", "constvoid*", "constvoid*", "uint32_t", "constrt3_radiance_params*", "void*", "void*"],
}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt3.h")).read(), flags=re.S)


def header_declarations():
    out = {}
    for name, args in re.findall(r"\bint\s+(rt3_radiance[a-z_]*)\s*\(([^)]*)\)\s*;", header_text()):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(re.sub(r"\s+", "", a[:a.rindex("*") + 1] if "*" in a else a[:a.rindex(" ")]))
        out[name] = types
    return out


def test_the_wire_struct_is_24_bytes_here_in_the_header_and_in_the_library(rt3, tmp_path):
    P = rt3.RADIANCE_PARAMS
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("max_depth", 0), ("seed", 4), ("flags", 8), ("sample_begin", 12),
                                                                    ("sample_count", 16), ("t_min", 20)]
    assert [t for _, t in P._fields_] == [C.c_uint32] * 5 + [C.c_float]
    m = re.search(r"typedef struct rt3_radiance_params \{(.*?)\} rt3_radiance_params;", header_text(), flags=re.S)
    assert re.findall(r"(uint32_t|float)\s+(\w+);", m.group(1)) == FIELDS
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rt3.h"\n_Static_assert(sizeof(rt3_radiance_params) == 24, "size");\n' +
                   "".join('_Static_assert(offsetof(rt3_radiance_params, %s) == %d, "%s");\n' % (n, 4 * k, n) for k, (_, n) in enumerate(FIELDS)) +
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")])
    device = open(os.path.join(ROOT, "raytracer-3_amd", "csrc", "rt3_device.hip")).read()
    assert 'static_assert(sizeof(rt3_radiance_params) == 24, "rt3.h: rt3_radiance_params");' in device


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    assert header_declarations() == DECLARED
    for s, types in DECLARED.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_uint32 if t == "uint32_t" else C.c_void_p for t in types], s
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3            # additions only: every existing struct is unchanged
    assert "RT3_ABI_VERSION 3u" in open(os.path.join(ROOT, "include", "rt3.h")).read()


def test_python_methods(rt3):
    sig = inspect.signature(rt3.HipRenderer.radiance)
    assert list(sig.parameters) == ["self", "rays", "keys", "samples", "sample_begin", "max_depth", "seed", "flags", "t_min"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, 1, 0, 8, 1, 0, 0.001]
    sig = inspect.signature(rt3.HipRenderer.radiance_device)
    assert list(sig.parameters) == ["self", "d_rays_ptr", "d_keys_ptr", "n", "radiance_params", "d_out_ptr", "stream_ptr"]
    assert sig.parameters["stream_ptr"].default is None


def calls(rt3, ctx):
    rays = rt3.make_rays([[0, 0, 0]] * 4, [[0, 0, -1]] * 4)
    keys = np.arange(4, dtype=np.uint32)
    out = np.zeros((4, 4), np.float32)
    rp = rt3.RADIANCE_PARAMS(4, 1, 0, 0, 2, 0.001)
    r, k, o = (a.ctypes.data_as(C.c_void_p) for a in (rays, keys, out))
    keep = (rays, keys, out, rp)
    return keep, (("rt3_radiance", (ctx, r, k, 4, C.byref(rp), o)), ("rt3_radiance", (ctx, r, None, 4, C.byref(rp), o)),
                  ("rt3_radiance", (ctx, None, None, 0, C.byref(rp), None)),
                  ("rt3_radiance_device", (ctx, r, k, 4, C.byref(rp), o, None)), ("rt3_radiance_device", (ctx, r, None, 4, C.byref(rp), o, None)),
                  ("rt3_radiance_device", (ctx, None, None, 0, None, None, None)))


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
        rt3.initialize_renderer(0).radiance(rt3.make_rays([[0, 0, 0]], [[0, 0, -1]]))


@pytest.mark.parametrize("args,message", [
    (("--scene", "three", "--spp", "4", "--rays", "r.bin", "o.png"), "--rays and --radiance go together"),
    (("--scene", "three", "--spp", "4", "--radiance", "r.pfm", "o.png"), "--rays and --radiance go together"),
    (("--rays", "r.bin", "--radiance", "r.pfm", "o.png"), "--rays and --radiance need the path tracer (Mode X): pass --spp."),
    (("--scene", "three", "--spp", "4", "--radiance", "r.pfm", "o.png", "--rays"), "--rays has no value."),
    (("--scene", "three", "--spp", "4", "--rays", "r.bin", "o.png", "--radiance"), "--radiance has no value."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_accepts_the_options_and_then_needs_a_device(tmp_path):
    """Past the parser the command line reaches for the device: without one that is the fatal convention's -1 with the backend's message,
    with one the render itself (the GPU suite)."""
    import torch
    if torch.cuda.is_available():
        return
    rays = tmp_path / "r.bin"
    rays.write_bytes(np.zeros(2, np.dtype("<f4, <f4, <f4, <f4, <f4, <f4, <f4, <u4")).tobytes())
    rc, out, err = run("--scene", "three", "--spp", "4", "-W", "32", "-H", "18", "--rays", str(rays), "--radiance", str(tmp_path / "r.pfm"),
                       str(tmp_path / "o.ppm"), "-f", "ppm")
    assert rc == -1 and "go together" not in err and "fatal:" in err, err


def test_cli_help_lists_the_new_options():
    rc, out, err = run("-h")
    assert rc == 0 and "--rays" in out and "--radiance" in out and "rt3_ray" in out
