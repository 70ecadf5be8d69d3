"""The display transform (include/rt3.h "Display transform") restated in numpy float32 and Python integers.

Every statistic of the auto-exposure is an integer and every per-pixel step is + - * /, sqrt, fma, a comparison or a table lookup, each an IEEE f32
operation rounded on its own, so this file reproduces rt3_debug_display_* (host) and rt3_display* (device) bit for bit: the tests compare words and
bit patterns.  The fused multiply-adds are environment_sample_ref.fma32; the sRGB table is rebuilt with exact rationals (fractions.Fraction)."""
from fractions import Fraction

import numpy as np

from environment_sample_ref import FLT_MAX, fma32

F = np.float32
U = np.uint32
CLAMP, REINHARD, FILMIC = 0, 1, 2
LINEAR, GAMMA2, SRGB = 0, 1, 2
AUTO_EXPOSURE = 1
BINS = 512
DARK = 0xFFFFFFFF
CURVES = {"clamp": CLAMP, "reinhard": REINHARD, "filmic": FILMIC}
TRANSFERS = {"linear": LINEAR, "gamma2": GAMMA2, "srgb": SRGB}

_table = None


def srgb_table():
    """table[i] = the number of k in 1..255 whose encoded value (k - 0.5) / 255 is at or below the sRGB encoding of i / 4095, in exact rationals:
    12.92 x for x <= 0.0031308, else 1.055 x^(5/12) - 0.055, where x^(5/12) >= t is decided as x^5 >= t^12."""
    global _table
    if _table is not None:
        return _table
    a, b, knee, slope = Fraction("1.055"), Fraction("0.055"), Fraction("0.0031308"), Fraction("12.92")
    edges = [Fraction(2 * k - 1, 510) for k in range(1, 256)]                      # (k - 0.5) / 255, increasing
    t12 = [((e + b) / a) ** 12 for e in edges]
    out = np.zeros(4096, np.uint8)
    count = 0
    for i in range(4096):
        x = Fraction(i, 4095)
        if x <= knee:
            y = slope * x
            while count < 255 and edges[count] <= y:
                count += 1
        else:
            x5 = x ** 5
            while count < 255 and t12[count] <= x5:                                # (the encoding is monotone: the count never falls)
                count += 1
        out[i] = count
    _table = out
    return out


def _pos(c, hi):
    """c > 0 ? fminf(c, hi) : 0 — NaN and negatives become 0."""
    c = np.asarray(c, F)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, np.minimum(c, F(hi)), F(0.0)).astype(F)


def luminance(rgb):
    rgb = np.asarray(rgb, F)
    with np.errstate(over="ignore"):
        return fma32(F(0.0722), rgb[..., 2], fma32(F(0.7152), rgb[..., 1], F(0.2126) * rgb[..., 0]))


def bins(rgb):
    """(K, 3+) float32 -> (K,) uint32: the histogram bin 0..511 of each pixel, DARK for a pixel below 2^-16."""
    rgb = np.ascontiguousarray(np.asarray(rgb, F).reshape(-1, np.shape(rgb)[-1])[:, :3])
    y = np.ascontiguousarray(luminance(_pos(rgb, FLT_MAX)).astype(F))
    k = (y.view(U) >> 19).astype(np.int64) - 1776
    return np.where(k < 0, DARK, np.minimum(k, BINS - 1)).astype(U)


def histogram(rgb):
    """-> (hist uint32 (512,), dark) of the pixels of a frame."""
    b = bins(rgb)
    dark = int((b == DARK).sum())
    hist = np.bincount(b[b != DARK].astype(np.int64), minlength=BINS).astype(U)
    return hist, dark


def gain(hist, exposure=1.0, key=0.18, trim_low=102, trim_high=51):
    """The auto-exposure gain of a histogram: the rank trim, S, the 64-bit floor division, the bin centre, exposure * (key / Lavg)."""
    h = [int(v) for v in np.asarray(hist).reshape(BINS)]
    n = sum(h)
    if n == 0:
        return F(exposure)
    lo, hi = (n * int(trim_low)) >> 10, (n * int(trim_high)) >> 10
    m = n - lo - hi
    s = begin = 0
    for k in range(BINS):
        end = begin + h[k]
        s += max(0, min(end, n - hi) - max(begin, lo)) * k
        begin = end
    p = (s << 19) // m
    lavg = np.array([(111 << 23) + p + (1 << 18)], U).view(F)[0]
    with np.errstate(over="ignore", under="ignore"):
        return F(F(exposure) * (F(key) / lavg))


def pack_channel(z):
    """glm::packUnorm4x8's channel: clamp to [0, 1], round(z * 255) half away from zero."""
    z = np.asarray(z, F)
    m = np.where(z < 0, F(0.0), z)
    m = np.where(F(1.0) < m, F(1.0), m).astype(F)
    v = m * F(255.0)
    return (np.floor(v.astype(np.float64) + 0.5)).astype(np.int64).astype(U) & U(0xFF)       # (v >= 0: roundf is floor(v + 0.5), exact in float64)


def pixels(rgb, g, curve, transfer, white=4.0):
    """(K, 3+) float32, the gain -> (K,) uint32 words 0xFF | B << 8 | G << 16 | R << 24."""
    rgb = np.asarray(rgb, F).reshape(-1, np.shape(rgb)[-1])[:, :3]
    with np.errstate(all="ignore"):
        x = _pos(F(g) * rgb, 65504.0)
        if curve == CLAMP:
            y = x
        elif curve == REINHARD:
            yx = luminance(x)
            w = F(white)
            s = ((F(1.0) + yx / (w * w)) / (F(1.0) + yx)).astype(F)
            y = x * s[:, None]
        else:
            y = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        z = np.minimum(y.astype(F), F(1.0))
        if transfer == LINEAR:
            byte = pack_channel(z)
        elif transfer == GAMMA2:
            byte = pack_channel(np.sqrt(z))
        else:
            idx = np.floor((z * F(4095.0)).astype(np.float64) + 0.5).astype(np.int64)
            byte = srgb_table()[idx].astype(U)
    return (U(0xFF) | (byte[:, 2] << U(8)) | (byte[:, 1] << U(16)) | (byte[:, 0] << U(24))).astype(U)


def display(frame, curve=FILMIC, transfer=SRGB, exposure=1.0, auto=False, key=0.18, white=4.0, trim_low=102, trim_high=51):
    """A whole frame (h, w, 4) float32 -> ((h, w) uint32 words, hist, dark, gain); hist and dark are None without auto-exposure."""
    frame = np.asarray(frame, F)
    h, w = frame.shape[:2]
    flat = frame.reshape(-1, frame.shape[-1])
    hist = dark = None
    g = F(exposure)
    if auto:
        hist, dark = histogram(flat)
        g = gain(hist, exposure, key, trim_low, trim_high)
    return pixels(flat, g, curve, transfer, white).reshape(h, w), hist, dark, g
