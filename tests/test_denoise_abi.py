"""The denoiser (rt3_denoise*) without a GPU: the rt3_denoise_params wire struct, header / binding / library coverage, the
"no device" stubs, the command line's new usage error, and the numpy reference (tests/denoise_ref.py) against its own per-pixel form and the
properties the specification states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
from test_cli import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt3_denoise", "rt3_denoise_device"]


def test_params_struct_is_16_bytes(rt3):
    P = rt3.DENOISE_PARAMS
    assert C.sizeof(P) == 16
    assert [getattr(P, f).offset for f in ("iterations", "normal_power", "sigma_luminance", "sigma_depth")] == [0, 4, 8, 12]
    src = ('#include <stddef.h>\n#include "rt3.h"\n_Static_assert(sizeof(rt3_denoise_params) == 16, "size");\n'
           '_Static_assert(offsetof(rt3_denoise_params, iterations) == 0 && offsetof(rt3_denoise_params, normal_power) == 4, "u");\n'
           '_Static_assert(offsetof(rt3_denoise_params, sigma_luminance) == 8 && offsetof(rt3_denoise_params, sigma_depth) == 12, "f");\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    for s in NEW:
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
    assert L.rt3_abi_version() == 3


def test_null_context_and_stubs(rt3, tmp_path):
    L = rt3.lib()
    p = rt3.DENOISE_PARAMS(5, 128, 4.0, 1.0)
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data_as(C.c_void_p)
    assert L.rt3_denoise(None, 2, 2, b, b, C.byref(p), b) == -1
    assert L.rt3_denoise_device(None, 2, 2, b, b, C.byref(p), b, None) == -1
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    S = C.CDLL(str(so))
    ctx = C.c_void_p(0x10)                                            # never dereferenced by a stub
    for name, args in (("rt3_denoise", (ctx, 2, 2, b, b, C.byref(p), b)), ("rt3_denoise_device", (ctx, 2, 2, b, b, C.byref(p), b, None))):
        fn = getattr(S, name)
        fn.restype = C.c_int
        assert fn(*args) == -2, name


@pytest.mark.parametrize("args", [("--denoise", "x.pfm", "o.png"), ("--scene", "a.scene", "--denoise", "x.pfm", "o.png")])
def test_cli_denoise_needs_mode_x(args):
    rc, out, err = run(*args)
    assert rc == -1 and "--denoise needs the path tracer (Mode X): pass --spp." in err


def test_cli_denoise_usage_and_help():
    rc, out, err = run("--denoise")
    assert rc == -1 and "--denoise has no value." in err
    rc, out, err = run("--aov", "P", "--denoise", "x.pfm", "o.png")                    # the existing message comes first, unchanged
    assert rc == -1 and "--aov and --hdr need the path tracer (Mode X): pass --spp." in err
    rc, out, err = run("-h")
    assert rc == 0 and "--denoise" in out


# ------------------------------------------------------------------------------------------------ the numpy reference
def test_reference_exp_is_within_two_ulp():
    x = -np.concatenate([np.linspace(0.0, 87.0, 100001), [0.0, 1e-8, 1e-30]]).astype(np.float32)
    e = R.exp32(x)
    t = np.exp(x.astype(np.float64))
    assert e.dtype == np.float32 and (np.abs(e - t) <= 2.0 * 2.0 ** -24 * t).all()
    assert R.exp32(np.float32([-np.inf, -104.5, -200.0])).tolist() == [0.0, 0.0, 0.0] and R.exp32(np.float32([0.0]))[0] == 1.0


def synthetic(rt3, h, w, seed, misses=0.2, zero_normals=0.05):
    """A random frame: colour, and AOVs with unit normals (some exactly zero), depths with misses (+inf) and albedos around the threshold."""
    rng = np.random.default_rng(seed)
    colour = np.zeros((h, w, 4), np.float32)
    colour[..., :3] = rng.gamma(1.0, 0.5, (h, w, 3))
    colour[..., 3] = rng.normal(size=(h, w))                          # ignored
    aov = np.zeros((h, w), rt3.AOV)
    alb = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    alb[rng.random((h, w, 3)) < 0.1] = 0.0
    alb[rng.random((h, w, 3)) < 0.05] = np.float32(2.0 ** -10)
    aov["albedo"] = alb
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n = (0.7 * n + 0.3 * np.array([0.0, 0.0, 1.0])).astype(np.float32)  # mostly facing +z, so neighbours are not all orthogonal
    n[rng.random((h, w)) < zero_normals] = 0.0
    aov["normal"] = n
    z = (5.0 + np.add.outer(np.arange(h), np.arange(w)) * 0.05 + rng.normal(0.0, 0.02, (h, w))).astype(np.float32)
    z[rng.random((h, w)) < misses] = np.inf
    aov["depth"] = z
    aov["coverage"] = np.where(np.isinf(z), 0.0, 1.0)
    return colour, aov


@pytest.mark.parametrize("h,w,kw", [(1, 1, {}), (3, 2, dict(iterations=2, normal_power=4)), (5, 7, dict(iterations=3, sigma_luminance=0.5)),
                                    (6, 5, dict(iterations=2, normal_power=1, sigma_depth=3.0))])
def test_reference_equals_its_per_pixel_form(rt3, h, w, kw):
    colour, aov = synthetic(rt3, h, w, h * 31 + w)
    a = R.denoise(colour, aov, **kw)
    b = R.denoise_scalar(colour, aov, **kw)
    assert a.dtype == np.float32 and a.shape == (h, w, 4)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_reference_keeps_a_flat_frame_and_has_positive_denominators(rt3):
    h, w = 12, 9
    colour = np.zeros((h, w, 4), np.float32)
    colour[..., :3] = (0.25, 0.5, 0.125)                               # dyadic: every weighted mean of equal values is exact
    aov = np.zeros((h, w), rt3.AOV)
    aov["albedo"] = (0.5, 0.5, 0.5)
    aov["normal"] = (0.0, 0.0, 1.0)
    aov["depth"] = 4.0
    out = R.denoise(colour, aov)
    assert np.array_equal(out[..., :3], colour[..., :3]) and not out[..., 3].any()
    colour, aov = synthetic(rt3, 17, 23, 5)
    with np.errstate(all="raise"):
        i, L, albedo, n, z, gz = R.prepare(colour, aov)
    v = R.moments(L, n, z, gz, 7, np.float32(1.0))
    assert (v >= 0).all() and np.isfinite(v).all()
    assert (gz >= 0).all() and (gz[np.isinf(z)] == 0).all()
    out = R.denoise(colour, aov)
    assert np.isfinite(out).all()


def test_reference_demodulates_and_remodulates_around_the_threshold(rt3):
    colour = np.array([[[3.0, 3.0, 3.0, 9.0]]], np.float32)
    aov = np.zeros((1, 1), rt3.AOV)
    aov["albedo"] = (0.5, 2.0 ** -10, 0.0)
    aov["depth"] = np.inf
    pieces = []
    R.denoise(colour, aov, iterations=1, passes_out=pieces)
    i, v = pieces[0]
    assert i[0, 0].tolist() == [6.0, 3.0, 3.0] and v[0, 0] == 0.0        # only a > 2^-10 divides
    out = R.denoise(colour, aov, iterations=1)
    assert np.allclose(out[0, 0, :3], 3.0, rtol=1e-6) and out[0, 0, 3] == 0.0


def split(rt3, h, w, kind, seed):
    """A frame split into region A (left) and B (right) with w_g = 0 across: orthogonal axis-aligned normals, or hits next to misses."""
    colour, aov = synthetic(rt3, h, w, seed, misses=0.0, zero_normals=0.0)
    b = np.zeros((h, w), bool)
    b[:, w // 2:] = True
    if kind == "normals":
        aov["normal"] = np.where(b[..., None], np.float32([1.0, 0.0, 0.0]), np.float32([0.0, 1.0, 0.0]))
    else:
        aov["depth"] = np.where(b, np.float32(np.inf), aov["depth"])
        aov["normal"] = np.where(b[..., None], np.float32(0.0), aov["normal"])
    return colour, aov, b


@pytest.mark.parametrize("kind", ["normals", "misses"])
def test_reference_independence_property(rt3, kind):
    colour, aov, b = split(rt3, 13, 20, kind, 3)
    out1 = R.denoise(colour, aov, iterations=4)
    c2 = colour.copy()
    c2[b, :3] = np.random.default_rng(1).uniform(0.0, 50.0, (int(b.sum()), 3))
    out2 = R.denoise(c2, aov, iterations=4)
    assert np.array_equal(out1[~b].view(np.uint32), out2[~b].view(np.uint32))
    assert not np.array_equal(out1[b], out2[b])
