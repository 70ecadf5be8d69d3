"""The law of display sequences (include/rt3.h "Display sequences") on the host, against tests/display_sequence_ref.py: the exposure
that follows a sequence (integers), its convergence, the bloom pyramid bit for bit, three properties of the bloom that do not go through the
reference, the refusals, the ABI and the command line's usage errors.  No device: rt3_debug_exposure_step / rt3_debug_bloom are
rt3_display_sequence_law.hpp — the functions the kernels call — compiled for the host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import display_ref as D
import display_sequence_ref as R
from test_display_ref import BAD
from test_gpu_display import frame_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
VP, U32, U64, F32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
MAX = R.MAX_LEVEL
BLOOM_SIZES = [(1, 1), (2, 3), (67, 3), (257, 5), (320, 203)]
SIGNATURES = {
    "rt3_display_sequence": [VP, U32, U32, VP, VP, VP, VP, VP], "rt3_display_sequence_device": [VP, U32, U32, VP, VP, VP, VP, VP, VP],
    "rt3_debug_display_bloom": [VP, VP, VP, U64, VP, VP], "rt3_debug_exposure_step": [VP, VP, VP, VP],
    "rt3_debug_bloom": [U32, U32, VP, F32, F32, U32, VP, VP],
}
# what rt3dseq::refusal adds to rt3disp::refusal
BAD_SEQUENCE = [dict(adapt=(0, 64)), dict(adapt=(1025, 64)), dict(adapt=(256, 0)), dict(adapt=(256, 1025)), dict(adapt=(0xFFFFFFFF, 1)),
                dict(bloom=(9, 1.0, 0.25)), dict(bloom=(0xFFFFFFFF, 1.0, 0.25)),
                dict(bloom=(0, -1.0, 0.25)), dict(bloom=(0, np.inf, 0.25)), dict(bloom=(0, np.nan, 0.25)), dict(bloom=(3, -0.5, 0.25)),
                dict(bloom=(0, 1.0, -0.25)), dict(bloom=(0, 1.0, np.inf)), dict(bloom=(3, 1.0, np.nan))]


def p(a):
    return a.ctypes.data_as(VP) if a is not None else None


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(U), np.asarray(b, F).view(U))


def hist_at(level_bin, count=1000):
    """A histogram whose every counted pixel is in one bin: its target is bin << 19 whatever the trims."""
    h = np.zeros(512, U)
    h[level_bin] = count
    return h


def record(rt3, level, frames, gain=1.0):
    return np.array((level, frames, gain, 0), rt3.EXPOSURE)


def check_step(rt3, prev, hist, **kw):
    params = rt3.display_sequence_params(auto=True, **kw)
    got = rt3.exposure_step(prev, hist, params)
    ref = R.exposure_step(None if prev is None else (int(prev["level"]), int(prev["frames"])), hist, True, kw.get("exposure", 1.0), kw.get("key", 0.18),
                          kw.get("trim_low", 102), kw.get("trim_high", 51), kw.get("adapt", (256, 64)))
    assert (int(got["level"]), int(got["frames"]), int(got["_pad"])) == (ref[0], ref[1], 0) and same_bits(got["gain"], ref[2]), (prev, kw, got, ref)
    return got


# ---- the exposure law
def test_exposure_step_equals_the_reference(rt3):
    rng = np.random.default_rng(11)
    hists = [np.zeros(512, U), hist_at(0), hist_at(511), hist_at(300, 1)]
    for _ in range(12):
        h = np.zeros(512, U)
        lo = int(rng.integers(0, 500))
        hi = int(rng.integers(lo + 1, 513))
        h[lo:hi] = rng.integers(0, 1 << int(rng.integers(1, 20)), hi - lo)
        hists.append(h)
    trims = [(102, 51), (0, 0), (1023, 0), (0, 1023), (500, 500)]
    for k, h in enumerate(hists):
        tl, th = trims[k % len(trims)]
        n, tgt = R.target(h, tl, th)
        assert 0 <= tgt <= MAX
        prevs = [None, record(rt3, 12345, 0), record(rt3, 0, 1), record(rt3, MAX, 7), record(rt3, tgt, 3), record(rt3, 200 << 19, 0xFFFFFFFF),
                 record(rt3, 200 << 19, 0xFFFFFFFE)]
        for d in (1, 1023, 1024, 1025):                                                  # both directions, next to the target
            prevs += [record(rt3, min(tgt + d, MAX), 2), record(rt3, max(tgt - d, 0), 2)]
        for prev in prevs:
            for rate in (1, 64, 256, 1024):
                for adapt in ((rate, 1024 if rate != 1024 else 1), (1 if rate != 1 else 1024, rate)):
                    check_step(rt3, prev, h, adapt=adapt, trim_low=tl, trim_high=th, exposure=0.75, key=0.25)
    # |d| of 0, 1, 1023 and 511 << 19 for every rate: the step is max(1, |d| * rate >> 10) and never more than |d|
    for d in (0, 1, 1023, MAX):
        for rate in (1, 64, 256, 1024):
            h = hist_at(0, 5) if d == 0 else _hist_for(d)
            up = check_step(rt3, record(rt3, 0, 1), h, adapt=(rate, 1), trim_low=0, trim_high=0)
            down = check_step(rt3, record(rt3, MAX, 1), hist_at(511) if d == 0 else _hist_for(MAX - d), adapt=(1, rate), trim_low=0, trim_high=0)
            want = 0 if d == 0 else max(1, (d * rate) >> 10)
            assert int(up["level"]) == want and int(down["level"]) == MAX - want and want <= d, (d, rate, up, down)


def _hist_for(level):
    """A histogram whose target is exactly `level` in the cases used here: bins only give multiples of 2^19, so two bins and no trim."""
    k, b = level >> 19, level & ((1 << 19) - 1)
    if b == 0:
        return hist_at(k)
    # ((a * k + b * (k + 1)) << 19) // (a + b) == level  <=  a + b = 2^19
    h = np.zeros(512, U)
    h[k], h[k + 1] = (1 << 19) - b, b
    return h


def test_targets_of_the_two_bin_histograms():
    for level in (0, 1, 1023, MAX - 1023, MAX - 1, MAX):
        assert R.target(_hist_for(level), 0, 0)[1] == level


def test_exposure_without_history_and_without_the_flag(rt3):
    h = hist_at(200)
    first = check_step(rt3, None, h)
    assert (int(first["level"]), int(first["frames"])) == (200 << 19, 1)
    assert same_bits(first["gain"], D.gain(h))                                            # the first frame is rt3_display's auto-exposure
    dark = check_step(rt3, None, np.zeros(512, U), exposure=0.5)
    assert (int(dark["level"]), int(dark["frames"])) == (0, 0) and dark["gain"] == F(0.5)     # an all-dark first frame sets nothing
    kept = check_step(rt3, record(rt3, 77 << 19, 4), np.zeros(512, U))
    assert (int(kept["level"]), int(kept["frames"])) == (77 << 19, 5)                     # a black frame does not move the eye
    assert same_bits(kept["gain"], R.gain_of_level(77 << 19))
    for prev in (None, record(rt3, 3 << 19, 9), record(rt3, 400 << 19, 9)):                # rates of 1024 reproduce rt3_display
        got = check_step(rt3, prev, h, adapt=(1024, 1024))
        assert int(got["level"]) == 200 << 19 and same_bits(got["gain"], D.gain(h))
    given = rt3.exposure_step(None, h, rt3.display_sequence_params(exposure=0.625))
    assert (int(given["level"]), int(given["frames"]), float(given["gain"]), int(given["_pad"])) == (0, 0, 0.625, 0)


@pytest.mark.parametrize("rate", [1024, 256, 64])
def test_convergence_never_overshoots_and_lands_on_the_target(rt3, rate):
    ref_steps = {}
    for start, goal, adapt in ((0, MAX, (rate, 1)), (MAX, 0, (1, rate))):
        level, steps = start, 0
        while level != goal:                                                            # the reference's chain gives the count
            level = R.step_level(level, goal, *adapt)
            steps += 1
        ref_steps[start] = steps
        params = rt3.display_sequence_params(auto=True, adapt=adapt, trim_low=0, trim_high=0)
        h = hist_at(goal >> 19)
        state, got, last = record(rt3, start, 1), 0, start
        while int(state["level"]) != goal:
            state = rt3.exposure_step(state, h, params)
            got += 1
            level = int(state["level"])
            assert (last < level <= goal) if goal > start else (goal <= level < last), (rate, got, last, level)
            last = level
            assert got <= steps
        assert got == steps and int(state["frames"]) == 1 + steps
        again = rt3.exposure_step(state, h, params)                                        # there, it stays there
        assert int(again["level"]) == goal
    assert ref_steps[0] == ref_steps[MAX]
    if rate == 1024:
        assert ref_steps[0] == 1
    else:
        assert 10 < ref_steps[0] < 400


# ---- the bloom law
def special(w, h, seed):
    """test_gpu_display's special frame (NaN, +-inf, negatives, denormals, 2^-24 .. 2^24) with a tenth of its pixels brought near the threshold."""
    frame = frame_of("special", w, h, seed).copy()
    rng = np.random.default_rng(seed + 1)
    near = rng.random((h, w)) < 0.3
    frame[near, :3] = rng.uniform(0.0, 6.0, (int(near.sum()), 3)).astype(F)
    return frame


@pytest.mark.parametrize("size", BLOOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_bloom_equals_the_reference_bit_for_bit(rt3, size):
    w, h = size
    frame = special(w, h, 31 * w + h)
    for levels in (1, 3, 8):
        for gain, threshold in ((0.75, 1.0), (2.0 ** -12, 0.0), (1.0, 3.5)):
            u1, b = rt3.bloom_plane(frame, gain, threshold, levels)
            ref_u1, ref_b = R.bloom(frame, gain, threshold, levels)
            assert u1.shape == ((h + 1) // 2, (w + 1) // 2, 4) and b.shape == (h, w, 4)
            assert same_bits(u1[..., :3], ref_u1) and same_bits(b[..., :3], ref_b), (levels, gain, threshold)
            assert not u1[..., 3].any() and not b[..., 3].any()
            assert np.isfinite(b).all() and (b >= 0).all()
    assert (R.bloom(frame, 0.75, 1.0, 3)[1] > 0).any()                                     # (the frames do bloom)


def test_bloom_of_a_constant_frame_is_the_constant(rt3):
    frame = np.full((37, 53, 4), 2.0, F)
    for levels in (1, 2, 4, 8):
        u1, b = rt3.bloom_plane(frame, 1.0, 0.0, levels)
        assert (b[..., :3] == 2.0).all() and (u1[..., :3] == F(2.0 * levels)).all(), levels


@pytest.mark.parametrize("size,levels", [(128, 3), (384, 5)])
def test_bloom_moves_with_the_frame_by_whole_coarse_texels(rt3, size, levels):
    rng = np.random.default_rng(size)
    s, c = 1 << levels, size // 2 - (1 << levels)

    def blob(dx, dy):
        frame = np.zeros((size, size, 4), F)
        frame[c + dy:c + dy + 9, c + dx:c + dx + 7, :3] = patch
        return frame

    patch = rng.uniform(1.5, 30.0, (9, 7, 3)).astype(F)
    base = rt3.bloom_plane(blob(0, 0), 1.0, 1.0, levels)[1]
    moved = rt3.bloom_plane(blob(s, s), 1.0, 1.0, levels)[1]
    assert (base[0] == 0).all() and (base[-1] == 0).all() and (base[:, 0] == 0).all() and (base[:, -1] == 0).all()      # away from the borders
    assert (moved[0] == 0).all() and (moved[-1] == 0).all() and base.max() > 0
    assert same_bits(moved[s:, s:], base[:-s, :-s])
    nudged = rt3.bloom_plane(blob(1, 1), 1.0, 1.0, levels)[1]
    assert not same_bits(nudged[1:, 1:], base[:-1, :-1])                                  # the pyramid is not shift-invariant below its coarsest texel


def test_no_pixel_above_the_threshold_gives_no_bloom(rt3):
    frame = special(67, 31, 5)
    frame[..., :3] = np.clip(np.nan_to_num(frame[..., :3], nan=0.0, posinf=1.0, neginf=0.0), 0.0, 0.9)
    assert 0.5 < D.luminance(frame[..., :3]).max() < 1.0
    for levels in (1, 3, 8):
        u1, b = rt3.bloom_plane(frame, 1.0, 1.0, levels)
        assert not u1.any() and not b.any()
    x = R.exposed(frame, 1.0)
    assert same_bits(R.composite(x, R.bloom(frame, 1.0, 1.0, 3)[1], 0.5), x)                # x' = x exactly: the words are the no-bloom words
    words = R.display_sequence(frame, bloom_params=(3, 1.0, 0.5))[0]
    assert np.array_equal(words, D.display(frame)[0])


# ---- refusals
def test_refusals_write_nothing(rt3):
    L = rt3.lib()
    hist = hist_at(100, 7)
    out = record(rt3, 9, 9, 9.0).reshape(1)
    prev = record(rt3, 5 << 19, 2).reshape(1)
    good = rt3.display_sequence_params(auto=True)

    def step(pv, h, prm, o):
        return L.rt3_debug_exposure_step(p(pv), p(h), C.byref(prm) if prm is not None else None, p(o))

    assert step(prev, hist, good, out) == 0 and int(out[0]["frames"]) == 3
    assert step(prev, hist, rt3.display_sequence_params(auto=True, adapt=(1, 1024), bloom=(8, 0.0, 0.0)), out) == 0      # the ranges' ends
    assert step(record(rt3, R.MAX_LEVEL, 1).reshape(1), hist, good, out) == 0
    out[0] = (9, 9, 9.0, 9)
    untouched = out.tobytes()
    for kw in BAD:
        assert step(prev, hist, rt3.display_sequence_params(auto=True, **kw), out) == -1, kw
    for kw in BAD_SEQUENCE:
        assert step(prev, hist, rt3.display_sequence_params(auto=True, **kw), out) == -1, kw
    for word in range(3):
        bad = rt3.display_sequence_params(auto=True)
        bad._pad[word] = 1
        assert step(prev, hist, bad, out) == -1, word
    bad = rt3.display_sequence_params(auto=True)
    bad.display.flags = 3
    assert step(prev, hist, bad, out) == -1
    assert step(prev, hist, rt3.display_sequence_params(auto=False), out) == -1             # prev_exposure without the flag
    assert step(record(rt3, R.MAX_LEVEL + 1, 1).reshape(1), hist, good, out) == -1         # a host level above 511 << 19
    assert step(record(rt3, 0xFFFFFFFF, 0).reshape(1), hist, good, out) == -1
    assert step(prev, None, good, out) == -1 and step(prev, hist, None, out) == -1 and step(prev, hist, good, None) == -1
    assert out.tobytes() == untouched                                                    # a refused call writes nothing

    frame = np.full((3, 4, 4), 2.0, F)
    u1, b = np.full((2, 2, 4), 9.0, F), np.full((3, 4, 4), 9.0, F)

    def bloom(w, h, c, threshold, levels, a=u1, o=b):
        return L.rt3_debug_bloom(w, h, p(c), 1.0, threshold, levels, p(a), p(o))

    assert bloom(4, 3, frame, 1.0, 8) == 0 and (b[..., :3] != 9).all()
    u1[:], b[:] = 9.0, 9.0
    assert bloom(4, 3, frame, 1.0, 1, a=None) == 0 and (u1 == 9).all() and bloom(4, 3, frame, 1.0, 1, o=None, a=None) == 0     # either output may be NULL
    b[:] = 9.0
    assert bloom(4, 3, frame, 1.0, 0) == -1 and bloom(4, 3, frame, 1.0, 9) == -1
    assert bloom(0, 3, frame, 1.0, 3) == -1 and bloom(4, 0, frame, 1.0, 3) == -1 and bloom(8193, 8192, frame, 1.0, 3) == -1
    assert bloom(4, 3, None, 1.0, 3) == -1
    for t in (-1.0, np.inf, np.nan):
        assert bloom(4, 3, frame, t, 3) == -1, t
    assert (u1 == 9).all() and (b == 9).all()
    with pytest.raises(rt3.Fatal):
        rt3.exposure_step(None, np.zeros(511, U), good)
    with pytest.raises(rt3.Fatal):
        rt3.bloom_plane(frame[..., :3], 1.0, 1.0, 3)
    with pytest.raises(rt3.Fatal):
        rt3.bloom_plane(frame, 1.0, 1.0, 9)


# ---- ABI
def test_struct_sizes_header_binding_and_library(rt3, tmp_path):
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
    assert ("int rt3_display_sequence(rt3_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const rt3_display_sequence_params* p, "
            "const rt3_exposure* prev_exposure, rt3_exposure* out_exposure, uint32_t* out_pixels);") in flat
    assert ("int rt3_display_sequence_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const void* d_rgba, const rt3_display_sequence_params* p, "
            "const void* d_prev_exposure, void* d_out_exposure, void* d_out_pixels, void* stream);") in flat
    assert ("int rt3_debug_exposure_step(const rt3_exposure* prev, const uint32_t hist[512], const rt3_display_sequence_params* p, "
            "rt3_exposure* out);") in flat
    assert ("int rt3_debug_bloom(uint32_t w, uint32_t h, const float* rgba, float gain, float threshold, uint32_t levels, float* out_u1, "
            "float* out_bloom);") in flat
    assert "int rt3_debug_display_bloom(rt3_ctx* ctx, float* out_u1, float* out_bloom, uint64_t capacity_pixels, uint32_t* w, uint32_t* h);" in flat
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rt3.h"\n'
                   '_Static_assert(sizeof(rt3_exposure) == 16 && sizeof(rt3_display_sequence_params) == 64 && sizeof(rt3_display_params) == 32, "sizes");\n'
                   '_Static_assert(offsetof(rt3_exposure, level) == 0 && offsetof(rt3_exposure, frames) == 4 && offsetof(rt3_exposure, gain) == 8 '
                   '&& offsetof(rt3_exposure, _pad) == 12, "rt3_exposure");\n'
                   '_Static_assert(offsetof(rt3_display_sequence_params, display) == 0 && offsetof(rt3_display_sequence_params, adapt_brighter) == 32 '
                   '&& offsetof(rt3_display_sequence_params, adapt_darker) == 36 && offsetof(rt3_display_sequence_params, bloom_levels) == 40 '
                   '&& offsetof(rt3_display_sequence_params, bloom_threshold) == 44 && offsetof(rt3_display_sequence_params, bloom_intensity) == 48 '
                   '&& offsetof(rt3_display_sequence_params, _pad) == 52, "rt3_display_sequence_params");\n'
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    unit = open(os.path.join(ROOT, "raytracer-3_amd", "csrc", "rt3_display_sequence.hip")).read()
    assert 'static_assert(sizeof(rt3_exposure) == 16, "rt3.h: rt3_exposure");' in unit
    assert 'static_assert(sizeof(rt3_display_sequence_params) == 64, "rt3.h: rt3_display_sequence_params");' in unit
    assert rt3.EXPOSURE.itemsize == 16 and [rt3.EXPOSURE.fields[k][1] for k in ("level", "frames", "gain", "_pad")] == [0, 4, 8, 12]
    P = rt3.DISPLAY_SEQUENCE_PARAMS
    assert C.sizeof(P) == 64 and (P.display.offset, P.adapt_brighter.offset, P.adapt_darker.offset, P.bloom_levels.offset, P.bloom_threshold.offset,
                                  P.bloom_intensity.offset, P._pad.offset) == (0, 32, 36, 40, 44, 48, 52)
    d = rt3.display_sequence_params()
    assert (d.display.curve, d.display.flags, d.adapt_brighter, d.adapt_darker, d.bloom_levels, d.bloom_threshold, d.bloom_intensity, list(d._pad)) == \
        (2, 0, 256, 64, 0, 1.0, 0.25, [0, 0, 0])
    b = rt3.display_sequence_params(bloom=(5, 2.0, 0.5), adapt=(1024, 1), auto=True)
    assert (b.display.flags, b.adapt_brighter, b.adapt_darker, b.bloom_levels, b.bloom_threshold, b.bloom_intensity) == (1, 1024, 1, 5, 2.0, 0.5)
    assert rt3.EXPOSURE_MAX_LEVEL == 511 << 19 == R.MAX_LEVEL
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3 and "RT3_ABI_VERSION 3u" in header      # two structs of their own and functions: nothing else
    assert C.sizeof(rt3.DISPLAY_PARAMS) == 32 and C.sizeof(rt3.rt3_stats) == 80


def test_null_context_and_no_device(rt3, tmp_path):
    L = rt3.lib()
    frame, out, good = np.zeros((2, 2, 4), F), np.full(4, 9, U), rt3.display_sequence_params(bloom=(2, 1.0, 0.25))
    state = np.full(4, 9, U)
    u1, b, w, h = np.full(4, 9.0, F), np.full(16, 9.0, F), C.c_uint32(9), C.c_uint32(9)
    assert L.rt3_display_sequence(None, 2, 2, p(frame), C.byref(good), None, p(state), p(out)) == -1      # RT3_E_ARG, as every entry point refuses a NULL context
    assert L.rt3_display_sequence_device(None, 2, 2, p(frame), C.byref(good), None, p(state), p(out), None) == -1
    assert L.rt3_debug_display_bloom(None, p(u1), p(b), 4, C.byref(w), C.byref(h)) == -1
    assert (out == 9).all() and (state == 9).all() and (u1 == 9).all() and (b == 9).all() and w.value == 9 and h.value == 9
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    stubs = C.CDLL(str(so))
    for name in ("rt3_display_sequence", "rt3_display_sequence_device", "rt3_debug_display_bloom"):
        getattr(stubs, name).restype = C.c_int
    assert stubs.rt3_display_sequence(VP(0x10), U32(2), U32(2), p(frame), C.byref(good), None, p(state), p(out)) == -2       # RT3_E_DEVICE: "no device"
    assert stubs.rt3_display_sequence_device(VP(0x10), U32(2), U32(2), p(frame), C.byref(good), None, p(state), p(out), None) == -2
    assert stubs.rt3_debug_display_bloom(VP(0x10), p(u1), p(b), U64(4), C.byref(w), C.byref(h)) == -2


# ---- the command line
def test_cli_usage_errors_and_help():
    from test_cli import run
    base = ("--scene", "three", "--spp", "4")
    rc, out, err = run(*base, "--display-frames", "Q", "--frames", "3", "o.png")
    assert rc == -1 and "--display-frames needs --display" in err, err
    rc, out, err = run(*base, "--display", "filmic", "--display-frames", "Q", "o.png")
    assert rc == -1 and "--display-frames needs a sequence" in err, err
    rc, out, err = run(*base, "--display", "filmic,srgb,2", "--adapt", "256,64", "o.png")
    assert rc == -1 and "--adapt needs --display with the auto exposure" in err, err
    rc, out, err = run(*base, "--adapt", "256,64", "o.png")
    assert rc == -1 and "--adapt needs --display" in err, err
    rc, out, err = run(*base, "--bloom", "3", "o.png")
    assert rc == -1 and "--bloom needs --display" in err, err
    for bad in ("0,64", "1025,64", "256", "256,64,1", "256,x", "2.5,64", "256,"):
        rc, out, err = run(*base, "--display", "filmic,srgb,auto", "--adapt", bad, "o.png")
        assert rc == -1 and "Invalid adapt '%s'" % bad in err, (bad, err)
    for bad in ("0", "9", "3,-1", "3,1,-0.5", "3,1,0.5,7", "three", "2.5", "3,inf", "3,1,nan"):
        rc, out, err = run(*base, "--display", "filmic", "--bloom", bad, "o.png")
        assert rc == -1 and "Invalid bloom '%s'" % bad in err, (bad, err)
    rc, out, err = run("-h")
    assert rc == 0 and "--display-frames" in out and "--adapt" in out and "--bloom" in out
