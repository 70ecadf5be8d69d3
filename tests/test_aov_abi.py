"""First-hit AOVs, camera rays and the linear frame without a GPU: the rt3_aov wire struct, the header / binding / library
coverage of the new entry points, their "no device" stubs, the PFM writer byte for byte, and the command line's new usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_cli import EXE, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_DEVICE = ["rt3_camera_rays", "rt3_camera_rays_device", "rt3_render_aov", "rt3_render_aov_device", "rt3_accum_resolve",
              "rt3_accum_resolve_device"]
NEW = NEW_DEVICE + ["rt3_frame_pfm_bytes", "rt3_frame_to_pfm"]


def test_aov_struct_is_48_bytes_and_the_dtype_matches(rt3):
    assert rt3.AOV.itemsize == 48
    offs = {f: rt3.AOV.fields[f][1] for f in ("albedo", "coverage", "normal", "depth", "kind", "index", "_pad")}
    assert offs == {"albedo": 0, "coverage": 12, "normal": 16, "depth": 28, "kind": 32, "index": 36, "_pad": 40}
    # the header's own layout, compiled
    src = ('#include <stddef.h>\n#include "rt3.h"\n_Static_assert(sizeof(rt3_aov) == 48, "size");\n'
           '_Static_assert(offsetof(rt3_aov, coverage) == 12 && offsetof(rt3_aov, normal) == 16 && offsetof(rt3_aov, depth) == 28, "f");\n'
           '_Static_assert(offsetof(rt3_aov, kind) == 32 && offsetof(rt3_aov, index) == 36 && offsetof(rt3_aov, _pad) == 40, "u");\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    for s in NEW:
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
    assert L.rt3_abi_version() == 3                                   # additions only


def test_new_device_entry_points_without_a_device(rt3, tmp_path):
    import torch
    L = rt3.lib()
    if not torch.cuda.is_available():
        # the library: no context can exist, and a NULL one is refused with RT3_E_ARG as by every other device call
        assert L.rt3_camera_rays(None, None, None, 0, 1, None) == -1
        assert L.rt3_camera_rays_device(None, None, None, 0, 1, None, None) == -1
        assert L.rt3_render_aov(None, None, None, None) == -1
        assert L.rt3_render_aov_device(None, None, None, None, None) == -1
        assert L.rt3_accum_resolve(None, None) == -1
        assert L.rt3_accum_resolve_device(None, None, None) == -1
    # the sanitizer build's "no device" stubs: RT3_E_DEVICE from each new device entry point
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    ctx = C.c_void_p(0x10)                                            # never dereferenced by a stub
    buf = np.zeros(64, np.float32)
    args = {"rt3_camera_rays": (ctx, None, None, 0, 1, buf.ctypes.data_as(C.c_void_p)),
            "rt3_camera_rays_device": (ctx, None, None, 0, 1, None, None),
            "rt3_render_aov": (ctx, None, None, buf.ctypes.data_as(C.c_void_p)),
            "rt3_render_aov_device": (ctx, None, None, None, None),
            "rt3_accum_resolve": (ctx, buf.ctypes.data_as(C.c_void_p)),
            "rt3_accum_resolve_device": (ctx, None, None)}
    for name in NEW_DEVICE:
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args[name]) == -2, name


def pfm_expected(img, ch):
    """The PFM bytes built in numpy: header, then rows bottom to top as little-endian float32."""
    h, w = img.shape[:2]
    head = ("PF" if ch == 3 else "Pf") + "\n%d %d\n-1.0\n" % (w, h)
    return head.encode() + np.ascontiguousarray(img[::-1]).astype("<f4").tobytes()


def lib_pfm(rt3, data, w, h, ch, stride):
    L = rt3.lib()
    p = data.ctypes.data_as(C.c_void_p)
    need = L.rt3_frame_pfm_bytes(p, w, h, ch, stride, None, 0)
    out = np.zeros(need, np.uint8)
    assert L.rt3_frame_pfm_bytes(p, w, h, ch, stride, out.ctypes.data_as(C.c_void_p), need) == need
    assert L.rt3_frame_pfm_bytes(p, w, h, ch, stride, out.ctypes.data_as(C.c_void_p), need - 1) == 0      # short buffer
    return out.tobytes()


SPECIALS = np.array([np.inf, -np.inf, np.nan, -0.0, 1e-45, 3.4e38], np.float32)


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (5, 4)])
def test_pfm_bytes_one_and_three_channels(rt3, w, h):
    rng = np.random.default_rng(w * 10 + h)
    rgb = rng.normal(0.0, 3.0, (h, w, 3)).astype(np.float32)
    flat = rgb.reshape(-1)
    flat[: min(len(flat), len(SPECIALS))] = SPECIALS[: min(len(flat), len(SPECIALS))]
    assert lib_pfm(rt3, rgb, w, h, 3, 3) == pfm_expected(rgb, 3)
    grey = rng.normal(0.0, 3.0, (h, w)).astype(np.float32)
    grey.reshape(-1)[: min(grey.size, len(SPECIALS))] = SPECIALS[: min(grey.size, len(SPECIALS))]
    assert lib_pfm(rt3, grey, w, h, 1, 1) == pfm_expected(grey, 1)
    # NaN payloads travel unchanged (bit-for-bit copy)
    assert lib_pfm(rt3, grey, w, h, 1, 1)[-4 * w * h:] == np.ascontiguousarray(grey[::-1]).astype("<f4").tobytes()


def test_pfm_bytes_strides_and_aov_planes(rt3):
    rng = np.random.default_rng(3)
    h, w = 3, 4
    aov = np.zeros((h, w), rt3.AOV)
    aov["albedo"] = rng.random((h, w, 3))
    aov["normal"] = rng.normal(0.0, 1.0, (h, w, 3))
    aov["depth"] = rng.uniform(0.0, 50.0, (h, w))
    aov["depth"][0, 1] = np.inf
    base = aov.view(np.float32).reshape(-1)
    for off, field, ch in ((0, "albedo", 3), (4, "normal", 3), (7, "depth", 1)):
        got = lib_pfm(rt3, base[off:], w, h, ch, 12)
        assert got == pfm_expected(aov[field], ch)
        assert rt3.pfm_bytes(aov[field]) == got                       # the Python helper on a strided view
    rgba = rng.random((h, w, 4)).astype(np.float32)
    assert lib_pfm(rt3, rgba, w, h, 3, 4) == pfm_expected(rgba[:, :, :3], 3)
    assert rt3.pfm_bytes(rgba[:, :, :3]) == pfm_expected(rgba[:, :, :3], 3)
    L = rt3.lib()
    p = rgba.ctypes.data_as(C.c_void_p)
    assert L.rt3_frame_pfm_bytes(p, w, h, 2, 4, None, 0) == 0         # channels 1 | 3 only
    assert L.rt3_frame_pfm_bytes(p, w, h, 3, 2, None, 0) == 0         # stride < channels
    assert L.rt3_frame_pfm_bytes(p, 0, h, 3, 3, None, 0) == 0


def test_frame_to_pfm_writes_the_same_bytes(rt3, tmp_path):
    img = np.arange(24, dtype=np.float32).reshape(2, 4, 3) - 5.5
    path = tmp_path / "x.pfm"
    L = rt3.lib()
    assert L.rt3_frame_to_pfm(img.ctypes.data_as(C.c_void_p), 4, 2, 3, 3, os.fsencode(str(path))) == 0
    assert path.read_bytes() == pfm_expected(img, 3)
    assert L.rt3_frame_to_pfm(img.ctypes.data_as(C.c_void_p), 4, 2, 3, 3, os.fsencode(str(tmp_path / "no" / "x.pfm"))) == -3
    assert L.rt3_frame_to_pfm(img.ctypes.data_as(C.c_void_p), 4, 2, 5, 5, os.fsencode(str(path))) == -1


AOV_USAGE_ERRORS = [
    (("--aov",), "--aov has no value."),
    (("--hdr", "-W", "8", "o.png"), "--hdr has no value."),
    (("--aov", "P", "o.png"), "--aov and --hdr need the path tracer (Mode X): pass --spp."),
    (("--hdr", "x.pfm", "o.png"), "--aov and --hdr need the path tracer (Mode X): pass --spp."),
    (("--scene", "a.scene", "--aov", "P", "o.png"), "--aov and --hdr need the path tracer (Mode X): pass --spp."),
]


@pytest.mark.parametrize("args,msg", AOV_USAGE_ERRORS)
def test_cli_aov_usage_errors(args, msg):
    rc, out, err = run(*args)
    assert rc == -1 and msg in err


def test_cli_help_lists_aov_and_hdr():
    rc, out, err = run("-h")
    assert rc == 0
    for frag in ("-f,--format", "(default: png)", "--spp", "--gpus", "--aov", "PREFIX.albedo.pfm", "--hdr", "3-channel PFM"):
        assert frag in out
