"""The temporal denoiser (rt3_denoise_temporal*) without a GPU: the rt3_history and rt3_temporal_params wire structs, header /
binding / library coverage, the "no device" stubs, the command line's new usage errors, and properties of the numpy restatement
(tests/temporal_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T
from test_cli import run
from test_denoise_abi import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt3_denoise_temporal", "rt3_denoise_temporal_device"]


def syntax_check(src):
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_history_struct_is_48_bytes(rt3):
    H = rt3.HISTORY
    assert H.itemsize == 48 and H == T.HISTORY
    assert [H.fields[f][1] for f in ("colour", "length", "moments", "depth", "_pad0", "normal", "_pad1")] == [0, 12, 16, 24, 28, 32, 44]
    syntax_check('#include <stddef.h>\n#include "rt3.h"\n_Static_assert(sizeof(rt3_history) == 48, "size");\n'
                 '_Static_assert(offsetof(rt3_history, length) == 12 && offsetof(rt3_history, moments) == 16, "a");\n'
                 '_Static_assert(offsetof(rt3_history, depth) == 24 && offsetof(rt3_history, normal) == 32, "b");\n'
                 '_Static_assert(offsetof(rt3_history, _pad1) == 44, "c");\n')


def test_temporal_params_struct_is_32_bytes(rt3):
    P = rt3.TEMPORAL_PARAMS
    assert C.sizeof(P) == 32
    assert [getattr(P, f).offset for f in ("spatial", "alpha", "moments_alpha", "depth_tolerance", "normal_tolerance")] == [0, 16, 20, 24, 28]
    syntax_check('#include <stddef.h>\n#include "rt3.h"\n_Static_assert(sizeof(rt3_temporal_params) == 32, "size");\n'
                 '_Static_assert(offsetof(rt3_temporal_params, spatial) == 0 && offsetof(rt3_temporal_params, alpha) == 16, "a");\n'
                 '_Static_assert(offsetof(rt3_temporal_params, moments_alpha) == 20, "b");\n'
                 '_Static_assert(offsetof(rt3_temporal_params, depth_tolerance) == 24, "c");\n'
                 '_Static_assert(offsetof(rt3_temporal_params, normal_tolerance) == 28, "d");\n')


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    for s in NEW:
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
    assert L.rt3_abi_version() == 3
    assert callable(getattr(rt3.HipRenderer, "denoise_temporal", None))


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(5, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9)
    cam = rt3.main_camera(4, 4).c
    buf = np.zeros(256, np.float32)
    b = buf.ctypes.data_as(C.c_void_p)
    assert L.rt3_denoise_temporal(None, 2, 2, C.byref(cam), b, b, None, None, C.byref(p), b, b) == -1
    assert L.rt3_denoise_temporal_device(None, 2, 2, C.byref(cam), b, b, None, None, C.byref(p), b, b, None) == -1
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    ctx = C.c_void_p(0x10)                                            # never dereferenced by a stub
    for name, args in (("rt3_denoise_temporal", (ctx, 2, 2, C.byref(cam), b, b, None, None, C.byref(p), b, b)),
                       ("rt3_denoise_temporal_device", (ctx, 2, 2, C.byref(cam), b, b, None, None, C.byref(p), b, b, None))):
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args) == -2, name


@pytest.mark.parametrize("args,message", [
    (("--spp", "4", "--frames", "0", "o.png"), "--frames must be at least 1."),
    (("--frames", "x", "o.png"), "Invalid frames 'x'"),
    (("--frames", "3", "o.png"), "--frames needs the path tracer (Mode X): pass --spp."),
    (("--scene", "a.scene", "--frames", "2", "o.png"), "--frames needs the path tracer (Mode X): pass --spp."),
    (("--scene", "cornell", "--orbit", "1", "o.png"), "--orbit needs a look-at camera (--scene weekend or stress100k)."),
    (("--scene", "three", "--frames", "2", "--orbit", "1", "o.png"), "--orbit needs a look-at camera (--scene weekend or stress100k)."),
    (("--spp", "4", "--orbit", "2", "o.png"), "--orbit needs a look-at camera (--scene weekend or stress100k)."),
    (("--scene", "weekend", "--orbit", "abc", "o.png"), "Invalid orbit 'abc'"),
    (("--scene", "weekend", "--orbit", "inf", "o.png"), "Invalid orbit 'inf'"),
    (("--scene", "weekend", "--orbit",), "--orbit has no value."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_help_lists_the_new_options():
    rc, out, err = run("-h")
    assert rc == 0 and "--frames" in out and "--orbit" in out


# ------------------------------------------------------------------------------------------------ the numpy restatement
def look_at(w, h, look_from, at=(0.0, 0.0, 0.0), vfov=20.0, focus=10.0):
    """The book's look-at camera in float32, as rt3_camera_look_at builds it up to rounding (the restatement takes any camera)."""
    f, a, up = (np.array(v, np.float64) for v in (look_from, at, (0.0, 1.0, 0.0)))
    hh = np.tan(np.radians(vfov) / 2.0)
    vh, vw = 2.0 * hh, 2.0 * hh * w / h
    wv = (f - a) / np.linalg.norm(f - a)
    u = np.cross(up, wv)
    u /= np.linalg.norm(u)
    v = np.cross(wv, u)
    hor, ver = focus * vw * u, focus * vh * v
    return T.Cam(f, hor, ver, f - hor / 2 - ver / 2 - focus * wv)


def orbit(w, h, deg):
    a = np.radians(deg)
    return look_at(w, h, (13.0 * np.cos(a) + 3.0 * np.sin(a), 2.0, 3.0 * np.cos(a) - 13.0 * np.sin(a)))


def test_no_history_is_the_spatial_denoiser_bit_for_bit(rt3):
    for (h, w), kw in (((9, 7), {}), ((16, 12), dict(iterations=2, normal_power=8, sigma_luminance=1.5))):
        colour, aov = synthetic(rt3, h, w, w * 100 + h)
        cam = look_at(w, h, (13.0, 2.0, 3.0))
        out, hist = T.denoise_temporal(colour, aov, cam, None, **kw)
        assert np.array_equal(out.view(np.uint32), R.denoise(colour, aov, **kw).view(np.uint32))
        assert (hist["length"] == 1.0).all()
        assert np.array_equal(hist["depth"].view(np.uint32), aov["depth"].view(np.uint32))
        pieces = []
        R.denoise(colour, aov, passes_out=pieces, **kw)
        i1 = pieces[1][0] if len(pieces) > 1 else None
        if i1 is not None:
            assert np.array_equal(hist["colour"].view(np.uint32), i1.view(np.uint32))      # the output of pass 0


def test_an_inconsistent_history_is_no_history(rt3):
    h, w = 10, 8
    colour, aov = synthetic(rt3, h, w, 3, misses=0.0)
    cam = look_at(w, h, (13.0, 2.0, 3.0))
    _, hist = T.denoise_temporal(colour, aov, cam, None)
    hist["depth"] = hist["depth"] + 100.0                               # every tap fails the depth test
    hist["colour"] = 1e6
    out, hist2 = T.denoise_temporal(colour, aov, cam, (hist, cam))
    assert np.array_equal(out.view(np.uint32), R.denoise(colour, aov).view(np.uint32)) and (hist2["length"] == 1.0).all()


def test_equal_cameras_reproject_every_pixel_to_itself():
    w, h = 37, 23
    cam = orbit(w, h, 5.0)
    z = np.random.default_rng(1).uniform(3.0, 30.0, (h, w)).astype(np.float32)
    z[::4, ::3] = np.inf
    r, ok, xp, yp = T.reproject(cam, T.Cam(*T.vecs(cam)), w, h, z)
    assert ok.all()
    assert np.array_equal(xp, np.broadcast_to(np.arange(w, dtype=np.float32), (h, w)))
    assert np.array_equal(yp, np.broadcast_to(np.arange(h, dtype=np.float32)[:, None], (h, w)))


@pytest.mark.parametrize("cam", ["orbit", "tilted"])
def test_a_point_projected_into_its_own_camera_lands_on_its_pixel(cam):
    w, h = 160, 120
    c = orbit(w, h, 17.0) if cam == "orbit" else look_at(w, h, (2.0, 7.0, -4.0), at=(0.5, 1.0, 2.0), vfov=55.0, focus=3.0)
    z = np.random.default_rng(2).uniform(1.0, 40.0, (h, w)).astype(np.float32)
    z[::5, ::7] = np.inf
    r, ok, xp, yp = T.reproject(c, c, w, h, z, shortcut=False)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    assert ok.all()
    err = np.maximum(np.abs(xp - xs), np.abs(yp - ys))
    assert err.max() <= 1e-3, err.max()


def flat_frame(rt3, h, w, value, depth=5.0):
    colour = np.zeros((h, w, 4), np.float32)
    colour[..., :3] = value
    aov = np.zeros((h, w), rt3.AOV)
    aov["albedo"] = (1.0, 1.0, 1.0)
    aov["normal"] = (0.0, 0.0, 1.0)
    aov["depth"] = depth
    aov["coverage"] = 1.0
    return colour, aov


def test_lengths_count_up_and_a_still_camera_averages(rt3):
    h, w = 8, 10
    cam = look_at(w, h, (13.0, 2.0, 3.0))
    prev = None
    values = [1.0, 2.0, 3.0, 6.0, 0.5]
    for k, val in enumerate(values):
        colour, aov = flat_frame(rt3, h, w, val)
        blend = {}
        out, hist = T.denoise_temporal(colour, aov, cam, prev, blended_out=blend)
        assert (hist["length"] == k + 1).all()
        mean = np.mean(values[:k + 1])
        assert np.allclose(blend["i"], mean, rtol=1e-6, atol=0) and np.allclose(out[..., :3], mean, rtol=1e-6, atol=0)
        if k + 1 >= 4:                                                  # the temporal variance of the inputs
            assert np.allclose(blend["v"], np.var(values[:k + 1]), rtol=1e-5)
        else:                                                           # the spatial one of a flat frame
            assert ((blend["v"] >= 0) & (blend["v"] < 1e-5)).all()
        prev = (hist, cam)
    for _ in range(3):                                                  # past 1/alpha frames the floor takes over
        out, hist = T.denoise_temporal(*flat_frame(rt3, h, w, 1.0), cam, prev)
        prev = (hist, cam)
    assert (hist["length"] == 8).all()


def test_a_depth_jump_above_the_tolerance_resets_length(rt3):
    h, w = 12, 12
    cam = look_at(w, h, (13.0, 2.0, 3.0))
    colour, aov = flat_frame(rt3, h, w, 0.5, depth=10.0)
    _, hist = T.denoise_temporal(colour, aov, cam, None)
    _, hist = T.denoise_temporal(colour, aov, cam, (hist, cam))
    assert (hist["length"] == 2).all()
    # gz = 0 on a flat depth plane, so the tolerance is depth_tolerance * 1e-3 * z_hat = 0.02: a step of 0.5 resets, one of 0.01 does not
    aov2 = aov.copy()
    aov2["depth"][:, : w // 2] = 10.5
    aov2["depth"][:, w // 2:] = 10.01
    _, hist2 = T.denoise_temporal(colour, aov2, cam, (hist, cam))
    assert (hist2["length"][:, : w // 2 - 1] == 1).all() and (hist2["length"][:, w // 2 + 1:] == 3).all()
    aov3 = aov.copy()
    aov3["normal"] = (0.0, 1.0, 0.0)                                     # normals turned by 90 degrees: rejected as well
    _, hist3 = T.denoise_temporal(colour, aov3, cam, (hist, cam))
    assert (hist3["length"] == 1).all()


def test_a_turning_camera_keeps_most_history(rt3):
    """A 1-degree orbit of a plane: the interior reprojects to consistent taps, the pixels that come into view have none."""
    w, h = 48, 32
    cams = [orbit(w, h, 0.0), orbit(w, h, 1.0)]
    colour, aov = flat_frame(rt3, h, w, 0.25)
    out = []
    prev = None
    for cam in cams:
        d, o = T.world_point(cam, w, h, None)
        t = (-1.0 - o[1]) / d[..., 1]                                   # the plane y = -1
        aov["depth"] = np.where(t > 0, t, np.inf).astype(np.float32)
        aov["normal"] = np.where(t[..., None] > 0, np.float32([0.0, 1.0, 0.0]), np.float32(0.0))
        o_, hist = T.denoise_temporal(colour, aov, cam, prev)
        prev = (hist, cam)
        out.append(hist)
    share = float((out[1]["length"] == 2).mean())
    assert 0.8 < share < 1.0, share
