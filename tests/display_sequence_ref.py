"""Display sequences (include/rt3.h "Display sequences") restated in numpy float32 and Python integers.

The exposure law is integers up to one float expression (display_ref's); the bloom law is + - * / and two fused multiply-adds on float32 arrays, every
operation rounded on its own, so this file reproduces rt3_debug_exposure_step / rt3_debug_bloom (host) and rt3_display_sequence* (device) bit for bit.
The histogram, the trim, the curve, the transfer and the pack are display_ref's."""
import numpy as np

import display_ref as D

F = np.float32
U = np.uint32
MAX_LEVEL = 511 << 19
HALF_MAX = 65504.0


# ---- the exposure
def target(hist, trim_low=102, trim_high=51):
    """(n, P_t) of a histogram: the counted pixels and (S << 19) // m; P_t is 0 when n == 0."""
    h = [int(v) for v in np.asarray(hist).reshape(D.BINS)]
    n = sum(h)
    if n == 0:
        return 0, 0
    lo, hi = (n * int(trim_low)) >> 10, (n * int(trim_high)) >> 10
    m = n - lo - hi
    s = begin = 0
    for k in range(D.BINS):
        end = begin + h[k]
        s += max(0, min(end, n - hi) - max(begin, lo)) * k
        begin = end
    return n, (s << 19) // m


def gain_of_level(level, exposure=1.0, key=0.18):
    lavg = np.array([(111 << 23) + int(level) + (1 << 18)], U).view(F)[0]
    with np.errstate(over="ignore", under="ignore"):
        return F(F(exposure) * (F(key) / lavg))


def step_level(level, tgt, brighter, darker):
    """One frame's move: a share rate / 1024 of the way, at least 1, never past the target (rate <= 1024); no move when already there."""
    d = tgt - level
    if d == 0:
        return level
    step = max(1, (abs(d) * (brighter if d > 0 else darker)) >> 10)
    return level + step if d > 0 else level - step


def exposure_step(prev, hist, auto=True, exposure=1.0, key=0.18, trim_low=102, trim_high=51, adapt=(256, 64), clamp_prev=False):
    """-> (level, frames, gain float32).  prev: None or (level, frames, ...).  clamp_prev: the device form's reading of a level above MAX_LEVEL."""
    if not auto:
        assert prev is None
        return 0, 0, F(exposure)
    n, tgt = target(hist, trim_low, trim_high)
    frames = int(prev[1]) if prev is not None else 0
    if frames == 0:
        if n == 0:
            return 0, 0, F(exposure)
        return tgt, 1, gain_of_level(tgt, exposure, key)
    before = int(prev[0])
    if clamp_prev:
        before = min(before, MAX_LEVEL)
    assert before <= MAX_LEVEL
    level = before if n == 0 else step_level(before, tgt, int(adapt[0]), int(adapt[1]))
    return level, min(frames + 1, 0xFFFFFFFF), gain_of_level(level, exposure, key)


# ---- the bloom: (h, w, 3) float32 planes
def exposed(frame, g):
    """x = positive(gain * c, 65504) of a frame's first three channels."""
    rgb = np.asarray(frame, F)[..., :3]
    with np.errstate(all="ignore"):
        return D._pos(F(g) * rgb, HALF_MAX)


def bright(x, threshold):
    with np.errstate(all="ignore"):
        y = D.luminance(x).astype(F)
        t = F(threshold)
        k = np.where(y > t, (y - t) / np.where(y > t, y, F(1.0)), F(0.0)).astype(F)
        return (x * k[..., None]).astype(F)


def half(n):
    return (n + 1) >> 1


def down(s):
    h, w = s.shape[:2]
    i, j = np.arange(half(w)), np.arange(half(h))
    ia, ib = np.minimum(2 * i, w - 1), np.minimum(2 * i + 1, w - 1)
    ja, jb = np.minimum(2 * j, h - 1), np.minimum(2 * j + 1, h - 1)
    top, bottom = s[ja], s[jb]
    with np.errstate(all="ignore"):
        return (((top[:, ia] + top[:, ib]) + (bottom[:, ia] + bottom[:, ib])) * F(0.25)).astype(F)


def up(u, w, h):
    """up(U) onto a w x h plane."""
    hc, wc = u.shape[:2]
    i, j = np.arange(w), np.arange(h)
    ia, ja = i >> 1, j >> 1
    ib = np.where(i & 1, np.minimum(ia + 1, wc - 1), np.maximum(ia - 1, 0))
    jb = np.where(j & 1, np.minimum(ja + 1, hc - 1), np.maximum(ja - 1, 0))
    near, far = u[ja], u[jb]
    with np.errstate(all="ignore"):
        ra = F(0.75) * near[:, ia] + F(0.25) * near[:, ib]
        rb = F(0.75) * far[:, ia] + F(0.25) * far[:, ib]
        return (F(0.75) * ra + F(0.25) * rb).astype(F)


def bloom(frame, g, threshold, levels):
    """-> (U_1 (h_1, w_1, 3), B (h, w, 3)) of a frame (h, w, 3+) under the gain g."""
    assert 1 <= levels <= 8
    x = exposed(frame, g)
    h, w = x.shape[:2]
    d = [bright(x, threshold)]
    for _ in range(levels):
        d.append(down(d[-1]))
    u = d[levels]
    for l in range(levels - 1, 0, -1):
        with np.errstate(all="ignore"):
            u = (d[l] + up(u, d[l].shape[1], d[l].shape[0])).astype(F)
    with np.errstate(all="ignore"):
        return u, (up(u, w, h) * (F(1.0) / F(levels))).astype(F)


def composite(x, b, intensity):
    with np.errstate(all="ignore"):
        return np.minimum(x + F(intensity) * b, F(HALF_MAX)).astype(F)


def display_sequence(frame, prev=None, curve=D.FILMIC, transfer=D.SRGB, exposure=1.0, auto=False, key=0.18, white=4.0, trim_low=102, trim_high=51,
                     adapt=(256, 64), bloom_params=None, clamp_prev=False):
    """A whole frame (h, w, 4) float32 -> ((h, w) uint32 words, (level, frames, gain), U_1 or None, B or None)."""
    frame = np.asarray(frame, F)
    h, w = frame.shape[:2]
    hist = D.histogram(frame.reshape(-1, frame.shape[-1]))[0] if auto else None
    state = exposure_step(prev, hist, auto, exposure, key, trim_low, trim_high, adapt, clamp_prev)
    g = state[2]
    x = exposed(frame, g)
    u1 = b = None
    if bloom_params is not None and bloom_params[0] != 0:
        levels, threshold, intensity = bloom_params
        u1, b = bloom(frame, g, threshold, levels)
        x = composite(x, b, intensity)
    return D.pixels(x.reshape(-1, 3), F(1.0), curve, transfer, white).reshape(h, w), state, u1, b      # (1 * x' = x', in [0, 65504]: pixels() leaves it)
