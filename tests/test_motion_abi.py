"""The motion plane and the denoiser that reads it (rt3_motion*, rt3_denoise_temporal_motion*) without a GPU: header /
binding / library coverage, the NULL context, the "no device" stubs, the command line's new usage errors, and properties of the numpy
restatement (tests/motion_ref.py) alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_ref as M
import temporal_ref as T
from test_cli import run
from test_denoise_abi import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt3_motion", "rt3_motion_device", "rt3_denoise_temporal_motion", "rt3_denoise_temporal_motion_device"]
F = np.float32


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    for s in NEW:
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
    assert L.rt3_abi_version() == 3
    assert callable(getattr(rt3.HipRenderer, "motion", None))
    import inspect
    sig = inspect.signature(rt3.HipRenderer.denoise_temporal)
    assert list(sig.parameters)[-1] == "motion" and sig.parameters["motion"].default is None


def calls(rt3, ctx):
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(5, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9)
    cam = rt3.main_camera(4, 4).c
    buf = np.zeros(256, np.float32)
    b = buf.ctypes.data_as(C.c_void_p)
    keep = (p, cam, buf)
    return keep, (("rt3_motion", (ctx, 2, 2, C.byref(cam), b, None, 0, None, 0, b)),
                  ("rt3_motion_device", (ctx, 2, 2, C.byref(cam), b, None, 0, None, 0, b, None)),
                  ("rt3_denoise_temporal_motion", (ctx, 2, 2, C.byref(cam), b, b, None, None, b, C.byref(p), b, b)),
                  ("rt3_denoise_temporal_motion_device", (ctx, 2, 2, C.byref(cam), b, b, None, None, b, C.byref(p), b, b, None)))


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    keep, table = calls(rt3, None)
    for name, args in table:
        assert getattr(L, name)(*args) == -1, name
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    keep, table = calls(rt3, C.c_void_p(0x10))                         # never dereferenced by a stub
    for name, args in table:
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args) == -2, name


@pytest.mark.parametrize("args,message", [
    (("--scene", "weekend", "--slide", "0.1,0,0", "o.png"), "--slide needs a sequence: pass --frames N with N of at least 2."),
    (("--scene", "weekend", "--frames", "1", "--slide", "0.1,0,0", "o.png"), "--slide needs a sequence: pass --frames N with N of at least 2."),
    (("--scene", "cornell", "--frames", "2", "--slide", "0.1,0,0", "o.png"), "--slide needs a sphere scene (--scene three, weekend or stress100k)."),
    (("--spp", "4", "--frames", "2", "--slide", "0.1,0,0", "o.png"), "--slide needs a sphere scene (--scene three, weekend or stress100k)."),
    (("--scene", "weekend", "--frames", "2", "--slide", "1,2", "o.png"), "Invalid slide '1,2'"),
    (("--scene", "weekend", "--frames", "2", "--slide", "1,2,3,4", "o.png"), "Invalid slide '1,2,3,4'"),
    (("--scene", "weekend", "--frames", "2", "--slide", "0.1,inf,0", "o.png"), "Invalid slide '0.1,inf,0'"),
    (("--scene", "weekend", "--frames", "2", "--slide", "a,b,c", "o.png"), "Invalid slide 'a,b,c'"),
    (("--scene", "three", "--frames", "2", "--slide", "-0.1,0,0x", "o.png"), "Invalid slide '-0.1,0,0x'"),
    (("--scene", "weekend", "--frames", "2", "--slide"), "--slide has no value."),
    (("--scene", "weekend", "--frames", "2", "--slide", "--spp", "o.png"), "--slide has no value."),
])
def test_cli_usage_errors(args, message):
    rc, out, err = run(*args)
    assert rc == -1 and message in err, err


def test_cli_help_lists_the_new_option():
    rc, out, err = run("-h")
    assert rc == 0 and "--slide" in out


# ------------------------------------------------------------------------------------------------ the numpy restatement
def test_an_all_zero_plane_is_the_camera_only_denoiser_bit_for_bit(rt3):
    for (h, w), kw in (((9, 7), {}), ((16, 12), dict(iterations=2, normal_power=8, sigma_luminance=1.5, depth_tolerance=8.0))):
        cam0 = T.Cam((0, 0, 0), (4, 0, 0), (0, 3, 0), (-2, -1.5, -1))
        cam1 = T.Cam((0.002, 0, 0.001), (4, 0, 0), (0, 3, 0), (-1.998, -1.5, -0.999))
        c0, a0 = synthetic(rt3, h, w, 7 * w + h)
        c1, a1 = synthetic(rt3, h, w, 7 * w + h + 1)
        a1["depth"], a1["normal"] = a0["depth"], a0["normal"]
        _, h0 = T.denoise_temporal(c0, a0, cam0, None, **kw)
        zero = np.zeros((h, w, 4), F)
        for cam in (cam0, cam1):                                       # a byte-equal camera (the shortcut) and a moved one
            want, wh = T.denoise_temporal(c1, a1, cam, (h0, cam0), **kw)
            for m in (None, zero):
                got, gh = M.denoise_temporal(c1, a1, cam, (h0, cam0), motion=m, **kw)
                assert got.tobytes() == want.tobytes() and gh.tobytes() == wh.tobytes()
            assert (wh["length"] == 2).any()
        first, fh = M.denoise_temporal(c0, a0, cam0, None, motion=zero, **kw)          # no previous frame: the plane is not read
        want, wh = T.denoise_temporal(c0, a0, cam0, None, **kw)
        assert first.tobytes() == want.tobytes() and fh.tobytes() == wh.tobytes()


def analytic_aov(rt3, cam, w, h, spheres):
    """The nearest hits of the pixel-centre rays with (centre, radius) spheres: depth, normal, kind, index as rt3_render_aov names them."""
    d, o = T.world_point(cam, w, h, None)
    aov = np.zeros((h, w), rt3.AOV)
    best = np.full((h, w), np.inf, F)
    aov["index"] = 0xFFFFFFFF
    for i, (c, r) in enumerate(spheres):
        c = np.array(c, F)
        oc = (c - o).astype(F)
        hh = T.dot(np.broadcast_to(oc, d.shape), d)
        cc = F(T.dot(oc, oc) - F(r) * F(r))
        disc = hh * hh - cc
        with np.errstate(invalid="ignore"):
            t = np.where(disc > 0, hh - np.sqrt(disc), np.inf).astype(F)
        hit = (disc > 0) & (t > F(0.001)) & (t < best)
        with np.errstate(invalid="ignore"):
            p = o + t[..., None] * d
            n = ((p - c) * (F(1.0) / F(r))).astype(F)
        best = np.where(hit, t, best)
        aov["normal"] = np.where(hit[..., None], n, aov["normal"])
        aov["kind"] = np.where(hit, 2, aov["kind"])
        aov["index"] = np.where(hit, i, aov["index"])
    aov["depth"] = best
    aov["albedo"] = 0.5
    aov["coverage"] = np.where(np.isinf(best), 0.0, 1.0)
    return aov


PREV = [((-0.8, 0.0, -4.0), 0.5), ((0.0, -0.9, -5.0), 0.6), ((0.0, -1001.5, -5.0), 1000.0)]
CUR = [((0.8, 0.1, -3.6), 0.55), PREV[1], PREV[2]]


def records(spheres):
    return np.array([list(c) + [r] for c, r in spheres], F)


@pytest.mark.parametrize("size", [(160, 120), (320, 240)])
@pytest.mark.parametrize("camera", ["still", "moving"])
def test_the_history_follows_a_sphere_that_moves_by_more_than_its_diameter(rt3, size, camera):
    w, h = size
    cam0 = T.Cam((0, 0, 0), (4, 0, 0), (0, 3, 0), (-2, -1.5, -1))
    cam1 = cam0 if camera == "still" else T.Cam((0.05, 0, 0), (4, 0, 0), (0, 3, 0), (-1.95, -1.5, -1))
    a0, a1 = analytic_aov(rt3, cam0, w, h, PREV), analytic_aov(rt3, cam1, w, h, CUR)
    hist = np.zeros((h, w), T.HISTORY)
    hist["depth"], hist["normal"], hist["length"] = a0["depth"], a0["normal"], 1.0
    plane = M.motion(cam1, a1, spheres=(records(CUR), records(PREV)))
    mover = (a1["kind"] == 2) & (a1["index"] == 0)
    assert mover.sum() > 100
    assert np.array_equal(plane[..., 3] != 0, mover) and not plane[~mover].any()       # only the mover has a motion record
    with_m = M.history_weight(a1, cam1, hist, cam0, plane) >= F(0.01)
    without = M.history_weight(a1, cam1, hist, cam0, None) >= F(0.01)
    share_with, share_without = float(with_m[mover].mean()), float(without[mover].mean())
    print("%dx%d %s camera: %d pixels show the mover; valid history with the motion plane %.3f, without %.3f"
          % (w, h, camera, int(mover.sum()), share_with, share_without))
    assert share_with >= 0.90 and share_without <= 0.10
    assert np.array_equal(with_m[~mover], without[~mover])


def test_the_plane_of_a_face_carries_barycentrics_to_the_previous_triangle(rt3):
    """One triangle facing the camera that moved rigidly: every pixel on it gets the translation back, to rounding."""
    w, h = 64, 48
    cam = T.Cam((0, 0, 0), (4, 0, 0), (0, 3, 0), (-2, -1.5, -1))
    cur = np.array([[-3, -2, -4, 1], [3, -2, -4, 1], [0, 3, -4, 1]], F)
    shift = np.array([0.25, -0.125, 0.5, 0], F)
    prev = cur - shift
    d, o = T.world_point(cam, w, h, None)
    aov = np.zeros((h, w), rt3.AOV)
    aov["depth"] = (F(-4.0) / d[..., 2]).astype(F)                      # the plane z = -4
    aov["kind"], aov["index"] = 1, 0
    aov["kind"][0, :] = 0                                               # a row of misses
    aov["depth"][0, :] = np.inf
    aov["index"][1, :] = 7                                              # a row of face indices out of range
    plane = M.motion(cam, aov, mesh=(np.array([[0, 1, 2]]), cur, prev))
    assert not plane[:2].any() and (plane[2:, :, 3] == 1).all()
    assert np.abs(plane[2:, :, :3] + shift[:3]).max() < 1e-5
    assert not M.motion(cam, aov, mesh=(np.array([[0, 1, 2]]), cur, cur.copy())).any()       # byte-equal vertices: nothing moved
    assert not M.motion(cam, aov).any()                                 # no previous arrays: nothing moved
    flat = cur.copy()
    flat[2] = flat[1]                                                    # a degenerate current triangle: den == 0
    assert not M.motion(cam, aov, mesh=(np.array([[0, 1, 2]]), flat, prev)).any()
