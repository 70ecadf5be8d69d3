"""The display transform's law (include/rt3.h "Display transform") on the host, against tests/display_ref.py: the sRGB table against
exact rationals, the histogram bins, the auto-exposure's gain and the per-pixel words bit for bit, the refusals, the ABI and the command line's usage
errors.  No device: rt3_debug_display_bin / _gain / _pixel / _srgb_table are rt3_display_law.hpp — the functions the kernels call — compiled for the host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import display_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
VP, U32, F32 = C.c_void_p, C.c_uint32, C.c_float
INF, NAN = F(np.inf), F(np.nan)
FLT_MAX = np.finfo(F).max
DENORM = np.array([1], U).view(F)[0]
PAIRS = [(c, t) for c in ("clamp", "reinhard", "filmic") for t in ("linear", "gamma2", "srgb")]
SIGNATURES = {
    "rt3_display": [VP, U32, U32, VP, VP, VP], "rt3_display_device": [VP, U32, U32, VP, VP, VP, VP],
    "rt3_debug_display_state": [VP, VP, VP, VP], "rt3_debug_display_bin": [VP, VP], "rt3_debug_display_gain": [VP, VP, VP],
    "rt3_debug_display_pixel": [VP, F32, VP, VP], "rt3_debug_display_srgb_table": [VP],
}


def p(a):
    return a.ctypes.data_as(VP)


def near(v):
    v = F(v)
    return [np.nextafter(v, F(0.0)), v, np.nextafter(v, INF)]


def special_values():
    """NaN, +-inf, negatives, 0, denormals, FLT_MAX, 2^-16 and 2^16 with their neighbours, the neighbourhood of 1 and of the half-float limit."""
    vals = [NAN, INF, -INF, F(-1.0), F(-0.0), F(0.0), DENORM, F(1e-40), FLT_MAX, F(0.18), F(0.5), F(2.0), F(1e4)]
    for v in (2.0 ** -16, 2.0 ** 16, 1.0, 65504.0, 2.0 ** -20, 2.0 ** 20):
        vals += near(v)
    return np.array(vals, F)


def special_colours():
    """Greys of every special value, each value alone in each channel (the others 0 and 0.25), and every ordered pair in (r, g)."""
    v = special_values()
    rows = [np.stack([v, v, v], 1)]
    for c in range(3):
        for other in (0.0, 0.25):
            a = np.full((len(v), 3), other, F)
            a[:, c] = v
            rows.append(a)
    g1, g2 = np.meshgrid(v, v, indexing="ij")
    rows.append(np.stack([g1.ravel(), g2.ravel(), np.full(g1.size, 0.125, F)], 1))
    return np.concatenate(rows).astype(F)


def random_colours(n, seed):
    """n positive colours spread over 2^-24 .. 2^24 (every histogram bin and the tails on both sides)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 2.0, (n, 3)) * np.exp2(rng.uniform(-24.0, 24.0, (n, 3)))).astype(F)


# ---- the table
def test_srgb_table_is_the_exact_rational_one(rt3):
    got = rt3.display_srgb_table()
    ref = R.srgb_table()
    assert got.dtype == np.uint8 and got.shape == (4096,)
    assert np.array_equal(got, ref)
    steps = np.diff(got.astype(np.int64))
    assert steps.min() >= 0 and steps.max() == 1                                     # monotone, steps of at most 1
    assert got[0] == 0 and got[-1] == 255 and len(np.unique(got)) == 256              # every code


def test_srgb_table_is_the_rounded_float64_encoding(rt3):
    x = np.arange(4096) / 4095.0
    enc = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    assert np.array_equal(rt3.display_srgb_table(), np.floor(255.0 * enc + 0.5).astype(np.uint8))


# ---- the bins
def test_bins_of_special_values(rt3):
    c = special_colours()
    got = rt3.display_bin(c)
    assert np.array_equal(got, R.bins(c))
    one = lambda *rgb: rt3.display_bin(np.array(rgb, F))
    assert one(NAN, NAN, NAN) == one(-1, -INF, -0.0) == one(0, 0, 0) == one(DENORM, DENORM, DENORM) == rt3.DISPLAY_DARK == R.DARK
    assert one(INF, 0, 0) == one(FLT_MAX, FLT_MAX, FLT_MAX) == one(0, INF, NAN) == 511
    assert one(1, 1, 1) in (16 * 16 - 1, 16 * 16)                                    # (the weights add up to 1 within an ulp)


def test_bins_at_every_edge(rt3):
    edges = ((np.arange(512, dtype=np.int64) + 1776) << 19).astype(U)                 # the bit pattern bin k starts at
    y = np.concatenate([(edges - U(1)).view(F), edges.view(F), (edges + U(1)).view(F), ((np.int64(2288) << 19) + np.arange(-1, 2)).astype(U).view(F)])
    grey = np.stack([y, y, y], 1)
    for c in (grey, np.stack([y, 0 * y, 0 * y], 1), np.stack([0 * y, y, 0 * y], 1), np.stack([0 * y, 0 * y, y], 1)):
        got = rt3.display_bin(c)
        assert np.array_equal(got, R.bins(c))
    k = rt3.display_bin(grey[512:1024])                                                # luminance(y, y, y) is y within an ulp: the bin or the one below
    d = k.astype(np.int64) - np.arange(512)
    assert ((d == 0) | (d == -1)).all()


def test_bins_of_random_colours(rt3):
    c = random_colours(10000, 1)
    got = rt3.display_bin(c)
    ref = R.bins(c)
    assert np.array_equal(got, ref)
    assert (ref == R.DARK).any() and (ref == 511).any() and len(np.unique(ref)) > 400


# ---- the gain
TRIMS = [(0, 0), (1023, 0), (0, 1023), (512, 511), (102, 51)]


def histograms():
    rng = np.random.default_rng(2)
    out = {"empty": np.zeros(512, U)}
    for name, k, n in (("one pixel", 200, 1), ("one pixel in bin 0", 0, 1), ("bin 0", 0, 12345), ("bin 511", 511, 54321), ("2^26 in one bin", 300, 1 << 26),
                       ("2^26 in bin 511", 511, 1 << 26)):
        h = np.zeros(512, U)
        h[k] = n
        out[name] = h
    out["two far bins"] = np.zeros(512, U)
    out["two far bins"][[3, 500]] = (1000, 24)
    out["uniform"] = np.full(512, 131072, U)                                           # 2^26 in all
    for i in range(6):
        h = rng.integers(0, 1 << rng.integers(1, 17), 512).astype(U)
        h[rng.random(512) < rng.random()] = 0
        out["random %d" % i] = h
    return out


@pytest.mark.parametrize("trim", TRIMS, ids=lambda t: "%d-%d" % t)
def test_gain_of_histograms(rt3, trim):
    for name, h in histograms().items():
        for exposure, key in ((1.0, 0.18), (0.37, 2.5), (3e30, 1e20), (1e-30, 1e-30)):   # (the last two: +inf and 0 after rounding)
            got = rt3.display_gain(h, exposure, key, *trim)
            ref = R.gain(h, exposure, key, *trim)
            assert got.view(U) == ref.view(U), (name, trim, exposure, key, got, ref)
    assert rt3.display_gain(np.zeros(512, U), 2.5, 0.18, *trim) == F(2.5)              # n == 0: the exposure itself


def test_gain_maps_the_log_average_to_the_key(rt3):
    h = np.zeros(512, U)
    h[16 * 16 + 8] = 1000                                                              # every pixel in [1.5, 1.5625): octave 0, 8 / 16 into it
    g = rt3.display_gain(h, 1.0, 0.18, 0, 0)
    assert g == F(0.18) / np.array([(111 << 23) + ((16 * 16 + 8) << 19) + (1 << 18)], U).view(F)[0]
    assert g == F(0.18) / F(1.53125)                                                   # the bin's centre
    h[511] = 10                                                                        # a bright tail of 1 %: trimmed away by the default 51 / 1024
    assert rt3.display_gain(h, 1.0, 0.18, 102, 51) == g and rt3.display_gain(h, 1.0, 0.18, 0, 0) < g


# ---- the pixels
@pytest.mark.parametrize("curve,transfer", PAIRS, ids=lambda v: v)
def test_pixels(rt3, curve, transfer):
    colours = np.concatenate([special_colours(), random_colours(10000, 3)])
    for gain in (F(2.0 ** -20), F(1.0), F(2.0 ** 20)):
        for white in ((F(2.0 ** -10), F(4.0), INF) if curve == "reinhard" else (F(4.0),)):
            got = rt3.display_pixel(colours, gain, curve, transfer, white)
            ref = R.pixels(colours, gain, R.CURVES[curve], R.TRANSFERS[transfer], white)
            bad = np.flatnonzero(got != ref)
            assert len(bad) == 0, (gain, white, len(bad), colours[bad[:3]], got[bad[:3]], ref[bad[:3]])
            assert (got & 0xFF == 0xFF).all()
    some = special_colours()[::7]
    for gain in (INF, F(0.0), NAN, F(-1.0), FLT_MAX, DENORM):                         # gains only a degenerate histogram or a caller's own call can give
        assert np.array_equal(rt3.display_pixel(some, gain, curve, transfer), R.pixels(some, gain, R.CURVES[curve], R.TRANSFERS[transfer]))


def test_pixel_landmarks(rt3):
    word = lambda rgb, *a: rt3.display_pixel(np.array(rgb, F), *a)
    assert word((0, 0, 0), 1.0, "filmic", "srgb") == 0x000000FF
    assert word((1, 1, 1), 1.0, "clamp", "linear") == word((7, INF, 1), 1.0, "clamp", "gamma2") == 0xFFFFFFFF
    assert word((1, 0.5, 0.25), 1.0, "clamp", "linear") == 0xFF8040FF                # round half away from zero: 127.5 -> 128
    assert word((0.25, 0.25, 0.25), 1.0, "clamp", "gamma2") == 0x808080FF
    assert word((0.5, 0.5, 0.5), 1.0, "clamp", "srgb") == 0xBCBCBCFF                  # sRGB(0.5) = 187.5: code 188
    assert word((4, 4, 4), 1.0, "reinhard", "linear", 4.0) == 0xFFFFFFFF             # `white` is mapped to 1
    assert word((1, 1, 1), 1.0, "reinhard", "linear", INF) in (0x7F7F7FFF, 0x808080FF)     # plain Reinhard: 1 / 2
    assert word((NAN, -1, INF), 0.0, "filmic", "srgb") == 0x000000FF                 # 0 * inf becomes 0


# ---- refusals
def params(rt3, **kw):
    return rt3.display_params(**kw)


BAD = [dict(curve=3), dict(curve=0xFFFFFFFF), dict(transfer=3), dict(trim_low=1024, trim_high=0), dict(trim_low=0, trim_high=1024), dict(trim_low=512, trim_high=512),
       dict(trim_low=0xFFFFFFFF, trim_high=2), dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=np.inf), dict(exposure=np.nan),
       dict(key=0.0), dict(key=-0.18), dict(key=np.inf), dict(key=np.nan), dict(white=2.0 ** -11), dict(white=0.0), dict(white=-4.0),
       dict(white=-np.inf), dict(white=np.nan)]


def test_refusals_write_nothing(rt3):
    L = rt3.lib()
    hist = np.zeros(512, U)
    hist[100] = 7
    rgb = np.array([0.5, 0.25, 0.125], F)
    gain, word = C.c_float(9.0), C.c_uint32(9)
    good = params(rt3)
    assert L.rt3_debug_display_gain(p(hist), C.byref(good), C.byref(gain)) == 0 and gain.value != 9.0
    assert L.rt3_debug_display_pixel(p(rgb), 1.0, C.byref(good), C.byref(word)) == 0 and word.value != 9
    assert L.rt3_debug_display_pixel(p(rgb), 1.0, C.byref(params(rt3, white=np.inf, trim_low=1023, trim_high=0)), C.byref(word)) == 0      # the ranges' ends
    gain.value, word.value = 9.0, 9
    for kw in BAD:
        bad = params(rt3, **kw)
        assert L.rt3_debug_display_gain(p(hist), C.byref(bad), C.byref(gain)) == -1, kw
        assert L.rt3_debug_display_pixel(p(rgb), 1.0, C.byref(bad), C.byref(word)) == -1, kw
    for bits in (2, 4, 0x80000000, 3):                                                # unknown flag bits, alone and next to the known one
        bad = params(rt3)
        bad.flags = bits
        assert L.rt3_debug_display_gain(p(hist), C.byref(bad), C.byref(gain)) == -1, bits
        assert L.rt3_debug_display_pixel(p(rgb), 1.0, C.byref(bad), C.byref(word)) == -1, bits
    assert L.rt3_debug_display_gain(None, C.byref(good), C.byref(gain)) == -1 and L.rt3_debug_display_gain(p(hist), None, C.byref(gain)) == -1
    assert L.rt3_debug_display_gain(p(hist), C.byref(good), None) == -1
    assert L.rt3_debug_display_pixel(None, 1.0, C.byref(good), C.byref(word)) == -1 and L.rt3_debug_display_pixel(p(rgb), 1.0, None, C.byref(word)) == -1
    assert L.rt3_debug_display_pixel(p(rgb), 1.0, C.byref(good), None) == -1
    b = C.c_uint32(9)
    assert L.rt3_debug_display_bin(None, C.byref(b)) == -1 and L.rt3_debug_display_bin(p(rgb), None) == -1 and L.rt3_debug_display_srgb_table(None) == -1
    assert gain.value == 9.0 and word.value == 9 and b.value == 9                     # a refused call writes nothing
    with pytest.raises(rt3.Fatal):
        rt3.display_params(curve="aces")
    with pytest.raises(rt3.Fatal):
        rt3.display_gain(np.zeros(511, U))


# ---- ABI
def test_struct_size_header_binding_and_library(rt3, tmp_path):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    header = open(os.path.join(ROOT, "include", "rt3.h")).read()
    for s, args in SIGNATURES.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
    flat = re.sub(r"\s+", " ", header)
    assert ("int rt3_display(rt3_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const rt3_display_params* p, "
            "uint32_t* out_pixels);") in flat
    assert ("int rt3_display_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const void* d_rgba, const rt3_display_params* p, "
            "void* d_out_pixels, void* stream);") in flat
    assert "int rt3_debug_display_state(rt3_ctx* ctx, uint32_t hist[512], uint32_t* dark, float* gain);" in flat
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rt3.h"\n_Static_assert(sizeof(rt3_display_params) == 32, "size");\n'
                   '_Static_assert(offsetof(rt3_display_params, exposure) == 20 && offsetof(rt3_display_params, white) == 28, "floats");\n'
                   '_Static_assert(RT3_DISPLAY_FILMIC == 2 && RT3_DISPLAY_SRGB == 2 && RT3_DISPLAY_AUTO_EXPOSURE == 1, "constants");\n'
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    unit = open(os.path.join(ROOT, "raytracer-3_amd", "csrc", "rt3_display.hip")).read()
    assert 'static_assert(sizeof(rt3_display_params) == 32, "rt3.h: rt3_display_params");' in unit
    assert C.sizeof(rt3.DISPLAY_PARAMS) == 32 and rt3.DISPLAY_PARAMS.exposure.offset == 20
    assert (rt3.DISPLAY_CLAMP, rt3.DISPLAY_REINHARD, rt3.DISPLAY_FILMIC) == (0, 1, 2) == (rt3.DISPLAY_LINEAR, rt3.DISPLAY_GAMMA2, rt3.DISPLAY_SRGB)
    assert rt3.DISPLAY_AUTO_EXPOSURE == 1
    d = rt3.display_params()
    assert (d.curve, d.transfer, d.flags, d.trim_low, d.trim_high, d.exposure, d.key, d.white) == (2, 2, 0, 102, 51, 1.0, F(0.18), 4.0)
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3 and "RT3_ABI_VERSION 3u" in header      # a struct of its own and functions: nothing else
    assert C.sizeof(rt3.rt3_stats) == 80


def test_null_context_and_no_device(rt3, tmp_path):
    L = rt3.lib()
    frame, out, good = np.zeros((2, 2, 4), F), np.full(4, 9, U), rt3.display_params()
    hist, dark, gain = np.full(512, 9, U), C.c_uint32(9), C.c_float(9.0)
    assert L.rt3_display(None, 2, 2, p(frame), C.byref(good), p(out)) == -1             # RT3_E_ARG, as every entry point refuses a NULL context
    assert L.rt3_display_device(None, 2, 2, p(frame), C.byref(good), p(out), None) == -1
    assert L.rt3_debug_display_state(None, p(hist), C.byref(dark), C.byref(gain)) == -1
    assert (out == 9).all() and (hist == 9).all() and dark.value == 9 and gain.value == 9.0
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    stubs = C.CDLL(str(so))
    for name in ("rt3_display", "rt3_display_device", "rt3_debug_display_state"):
        fn = getattr(stubs, name)
        fn.restype = C.c_int
    assert stubs.rt3_display(VP(0x10), U32(2), U32(2), p(frame), C.byref(good), p(out)) == -2       # RT3_E_DEVICE: "no device"
    assert stubs.rt3_display_device(VP(0x10), U32(2), U32(2), p(frame), C.byref(good), p(out), None) == -2
    assert stubs.rt3_debug_display_state(VP(0x10), p(hist), C.byref(dark), C.byref(gain)) == -2


# ---- the command line
def test_cli_usage_errors():
    from test_cli import run
    rc, out, err = run("--scene", "three", "--spp", "4", "--display", "bogus", "o.png")
    assert rc == -1 and "Unknown display curve 'bogus'" in err, err
    rc, out, err = run("--scene", "three", "--spp", "4", "--display", "filmic,nope", "o.png")
    assert rc == -1 and "Unknown display transfer 'nope'" in err, err
    rc, out, err = run("--scene", "three", "--spp", "4", "--display", "filmic,srgb,-1", "o.png")
    assert rc == -1 and "Invalid display exposure '-1'" in err, err
    for bad in ("filmic,srgb,0", "filmic,srgb,nan", "filmic,srgb,inf", "filmic,srgb,1x", "filmic,srgb,", "filmic,,1", "filmic,srgb,1,2"):
        rc, out, err = run("--scene", "three", "--spp", "4", "--display", bad, "o.png")
        assert rc == -1 and ("Invalid display exposure" in err or "Unknown display transfer" in err), (bad, err)
    rc, out, err = run("--display", "filmic", "o.png")                                 # the built-in scene without --spp is Mode R
    assert rc == -1 and "--display needs the path tracer (Mode X): pass --spp." in err, err
    rc, out, err = run("--display")
    assert rc == -1 and "--display has no value." in err, err
    rc, out, err = run("-h")
    assert rc == 0 and "--display" in out and "clamp | reinhard | filmic" in out
