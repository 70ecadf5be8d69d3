"""The display transform (rt3_display*) on the GPU, word for word and bit for bit against tests/display_ref.py: the law for the nine
curve x transfer pairs with and without auto-exposure, the state the auto-exposure leaves, repeatability, the host / device / stream forms, the anchor
(clamp + linear | gamma2 of the linear frame is render_path's frame), the device pipeline behind the denoiser, the accumulation and the stats left alone,
the command line's --display, and the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_ref as R
from test_display_ref import BAD, PAIRS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")

F, U = np.float32, np.uint32
FLT_MAX = np.finfo(F).max
# 1x1, a partial wave, a partial block, many blocks on the same bins, and one frame just over both grid caps (k_display_map: 2048 blocks of 256 pixels;
# k_display_histogram: 256 blocks of 1024 threads, two pixels each — 2^19 pixels a turn either way): both grid-stride loops turn
SIZES = [(1, 1), (67, 3), (257, 5), (320, 203), (1031, 509)]
assert 1031 * 509 > 2048 * 256 > 1031 * 508


def frame_of(kind, w, h, seed):
    """(h, w, 4) float32.  special: colours spread over 2^-24 .. 2^24 with NaN, +-inf, negatives, 0, denormals and FLT_MAX strewn in; tail: values near 0.1
    and a few pixels at 1e4; dark: nothing reaches 2^-16 (n == 0)."""
    rng = np.random.default_rng(seed)
    n = w * h
    if kind == "special":
        c = (rng.uniform(0.5, 2.0, (n, 4)) * np.exp2(rng.uniform(-24.0, 24.0, (n, 4)))).astype(F)
        odd = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1e-40, FLT_MAX, 2.0 ** -16, 2.0 ** 16, 1.0, 65504.0], F)
        where = rng.random((n, 4)) < 0.05
        c[where] = odd[rng.integers(0, len(odd), int(where.sum()))]
        c[0] = (np.nan, np.inf, -1.0, 7.0)                                          # (also in the 1x1 frame)
    elif kind == "tail":
        c = rng.uniform(0.05, 0.2, (n, 4)).astype(F)
        c[rng.integers(0, n, max(1, n // 200)), :3] = 1e4
    else:
        c = rng.uniform(0.0, 1.5e-5, (n, 4)).astype(F)                               # luminance < 2^-16 = 1.53e-5
        where = rng.random((n, 4)) < 0.1
        c[where] = np.array([np.nan, -np.inf, -3.0, 0.0, 1e-42], F)[rng.integers(0, 5, int(where.sum()))]
    c[:, 3] = rng.uniform(-1e30, 1e30, n).astype(F)                                  # the fourth float is ignored
    return c.reshape(h, w, 4)


def words(t):
    """A torch tensor of words -> numpy uint32."""
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy().view(U)


def same_bits(a, b):
    return np.asarray(a, F).view(U) == np.asarray(b, F).view(U)


def set_spheres(rt3, r, cr, mats):
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    r.set_spheres(cr, mats)


# ------------------------------------------------------------------------------------------------ 1: the law and the state
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ["special", "tail", "dark"])
def test_words_and_state_equal_the_reference(rt3, renderer, kind, size):
    import torch
    w, h = size
    frame = frame_of(kind, w, h, 1000 * w + h)
    d_frame = torch.from_numpy(frame).cuda()
    hist, dark = R.histogram(frame.reshape(-1, 4))
    assert hist.sum() + dark == w * h and (hist.sum() == 0) == (kind == "dark")
    exposure, key, white, trims = (0.75, 0.18, 4.0, (102, 51)) if kind != "tail" else (1.0, 0.25, 2.0, (0, 100))
    gain = R.gain(hist, exposure, key, *trims)
    for auto, g in ((False, F(exposure)), (True, gain)):
        for curve, transfer in PAIRS:
            got = renderer.display(d_frame, curve, transfer, exposure, auto, key, white, *trims)
            assert tuple(got.shape) == (h, w) and got.is_cuda
            ref = R.pixels(frame.reshape(-1, 4), g, R.CURVES[curve], R.TRANSFERS[transfer], white).reshape(h, w)
            bad = np.argwhere(words(got) != ref)
            assert len(bad) == 0, (curve, transfer, auto, len(bad), bad[:3], frame[tuple(bad[0])])
            if auto:
                s_hist, s_dark, s_gain = renderer.display_state()
                assert np.array_equal(s_hist, hist) and s_dark == dark and same_bits(s_gain, gain), (curve, transfer, s_dark, dark, s_gain, gain)
    if kind == "tail" and w * h >= 10000:                                            # the trimmed tail does not move the exposure
        body = frame.copy()
        body[(frame[..., :3] == 1e4).any(-1), :3] = 0.1
        assert 0.5 < float(gain) / float(R.gain(R.histogram(body.reshape(-1, 4))[0], exposure, key, *trims)) <= 1.0
    if kind == "dark":
        assert gain == F(exposure)


def test_two_calls_in_a_row_are_identical(rt3, renderer):
    frame = frame_of("special", 320, 203, 5)
    a = renderer.display(frame, "reinhard", "srgb", auto=True)
    sa = renderer.display_state()
    b = renderer.display(frame, "reinhard", "srgb", auto=True)
    sb = renderer.display_state()
    assert a.tobytes() == b.tobytes()                                               # the state is zeroed at the start of each call
    assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1] and same_bits(sa[2], sb[2]) and sa[0].sum() + sa[1] == 320 * 203
    other = frame_of("tail", 67, 3, 6)
    renderer.display(other, auto=True)
    hist, dark = R.histogram(other.reshape(-1, 4))
    so = renderer.display_state()
    assert np.array_equal(so[0], hist) and so[1] == dark                             # nothing of the larger frame is left
    renderer.display(frame, "clamp", "linear")                                       # a call without the flag leaves the state alone
    sk = renderer.display_state()
    assert np.array_equal(sk[0], hist) and sk[1] == dark and same_bits(sk[2], so[2])


# ------------------------------------------------------------------------------------------------ 2: the forms
def test_host_device_and_stream_forms_are_equal(rt3, renderer):
    import torch
    L = rt3.lib()
    w, h = 257, 5
    frame = frame_of("special", w, h, 7)
    d_frame = torch.from_numpy(frame).cuda()
    for kw in (dict(curve="filmic", transfer="srgb", auto=True, exposure=0.5), dict(curve="reinhard", transfer="gamma2", white=2.0)):
        host = renderer.display(frame, **kw)
        assert host.dtype == U and host.shape == (h, w)
        assert np.array_equal(host, R.display(frame, R.CURVES[kw["curve"]], R.TRANSFERS[kw["transfer"]], kw.get("exposure", 1.0), kw.get("auto", False),
                                              white=kw.get("white", 4.0))[0])
        t = renderer.display(d_frame, **kw)
        assert t.dtype == getattr(torch, "uint32", torch.int32) and np.array_equal(words(t), host)
        p = rt3.display_params(**kw)
        out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        renderer.display_device(w, h, d_frame.data_ptr(), p, out.data_ptr())           # NULL: the context's own stream
        renderer.synchronize()
        assert np.array_equal(words(out), host)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out2 = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            assert L.rt3_display_device(renderer._ctx, w, h, C.c_void_p(d_frame.data_ptr()), C.byref(p), C.c_void_p(out2.data_ptr()),
                                        C.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
        assert np.array_equal(words(out2), host)
    rows = renderer.display(frame[1:4], "filmic", "srgb")                            # geometry does not matter: a shard's rows are the frame's rows
    assert np.array_equal(rows, renderer.display(frame, "filmic", "srgb")[1:4])


# ------------------------------------------------------------------------------------------------ 3: the anchor
@pytest.mark.parametrize("flags,transfer", [(0, "linear"), (1, "gamma2")], ids=["linear", "gamma2"])
def test_clamp_of_the_linear_frame_is_render_paths_frame(rt3, renderer, flags, transfer):
    assert rt3.FLAG_GAMMA2 == 1
    w, h = 64, 48
    set_spheres(rt3, renderer, *rt3.scene_three_spheres())
    cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=11, flags=flags)
    packed = renderer.render_path(cam.c, p)
    lin = renderer.accum_resolve(p)
    got = renderer.display(lin, "clamp", transfer, exposure=1.0)
    assert got.shape == packed.shape and np.array_equal(got, packed)
    assert len(np.unique(packed)) > 100                                             # (a frame with something in it)


# ------------------------------------------------------------------------------------------------ 4: the pipeline on the device
def test_render_aov_denoise_display_without_a_host_copy(rt3, renderer):
    import torch
    w, h = 96, 64
    set_spheres(rt3, renderer, *rt3.scene_three_spheres())
    cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=5)
    stream = torch.cuda.current_stream().cuda_stream
    d_pix = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_lin = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_aov = torch.zeros((h, w, 12), dtype=torch.float32, device="cuda")
    renderer.render_path_device(cam.c, p, d_pix.data_ptr(), stream)
    renderer.accum_resolve_device(d_lin.data_ptr(), stream)
    renderer.render_aov_device(cam.c, p, d_aov.data_ptr(), stream)
    d_den = renderer.denoise(d_lin, d_aov)
    d_out = renderer.display(d_den, "filmic", "srgb", auto=True)                      # every step queued; nothing has come back to the host yet
    den = d_den.cpu().numpy()
    ref, hist, dark, gain = R.display(den, R.FILMIC, R.SRGB, auto=True)
    assert np.array_equal(words(d_out), ref)
    s_hist, s_dark, s_gain = renderer.display_state()
    assert np.array_equal(s_hist, hist) and s_dark == dark and same_bits(s_gain, gain)
    assert np.array_equal(renderer.display(den, "filmic", "srgb", auto=True), ref)   # the host form of the same floats


# ------------------------------------------------------------------------------------------------ 5: accumulation and stats untouched
def test_progressive_render_and_stats_across_a_display(rt3, renderer):
    w, h = 48, 32
    set_spheres(rt3, renderer, *rt3.scene_three_spheres())
    cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=3, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_VARIANCE)
    one = renderer.render_path(cam.c, p)
    acc1, sq1, _ = renderer.accum_download(p, want_sq=True)
    renderer.render_path_range(cam.c, p, 0, 2)
    st = renderer.stats()
    frame = frame_of("special", w + 9, h + 5, 4)
    renderer.display(frame, auto=True)
    renderer.display(frame, "clamp", "linear")
    assert bytes(renderer.stats()) == bytes(st)
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 2), one)
    acc2, sq2, done = renderer.accum_download(p, want_sq=True)
    assert done == 4 and acc1.tobytes() == acc2.tobytes() and sq1.tobytes() == sq2.tobytes()


# ------------------------------------------------------------------------------------------------ 6: the command line
def test_cli_writes_the_python_result(rt3, renderer, tmp_path):
    w, h = 64, 48
    base = [EXE, "--scene", "three", "--spp", "4", "-W", str(w), "-H", str(h), "-f", "ppm"]
    subprocess.run(base + ["--display", "reinhard,srgb,auto", "--hdr", "H.pfm", "a.ppm"], cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    subprocess.run(base + ["--display", "filmic,gamma2,0.5", "--denoise", "D.pfm", "b.ppm"], cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    set_spheres(rt3, renderer, *rt3.scene_three_spheres())
    cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=50, seed=1, flags=rt3.FLAG_GAMMA2)
    renderer.render_path(cam.c, p)
    lin = renderer.accum_resolve(p)
    den = renderer.denoise(lin, renderer.render_aov(cam.c, p))

    def rgb(words):
        return np.stack([words >> 24, (words >> 16) & 0xFF, (words >> 8) & 0xFF], -1).astype(np.uint8)

    def ppm(name):
        return np.frombuffer((tmp_path / name).read_bytes()[-3 * w * h:], np.uint8).reshape(h, w, 3)

    assert np.array_equal(ppm("a.ppm"), rgb(renderer.display(lin, "reinhard", "srgb", auto=True)))     # the linear frame's transform
    assert np.array_equal(ppm("b.ppm"), rgb(renderer.display(den, "filmic", "gamma2", exposure=0.5)))  # with --denoise: the denoised frame's
    assert (tmp_path / "H.pfm").read_bytes() == rt3.pfm_bytes(lin[..., :3]) and (tmp_path / "D.pfm").read_bytes() == rt3.pfm_bytes(den[..., :3])


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_argument_errors(rt3, renderer):
    import torch
    L = rt3.lib()
    ctx = renderer._ctx
    w, h = 8, 4
    frame = frame_of("tail", w, h, 1)
    out = np.full((h, w), 9, U)
    good = rt3.display_params(auto=True)

    def host(w_, h_, p, c=frame, o=out):
        return L.rt3_display(ctx, w_, h_, c.ctypes.data_as(C.c_void_p) if c is not None else None, C.byref(p) if p is not None else None,
                             o.ctypes.data_as(C.c_void_p) if o is not None else None)

    assert host(w, h, None) == -1 and host(w, h, good, c=None) == -1 and host(w, h, good, o=None) == -1
    assert host(0, h, good) == -1 and host(w, 0, good) == -1
    assert host(8193, 8192, good) == -1                                              # more than 2^26 pixels: refused before anything is read
    assert host(0xFFFFFFFF, 0xFFFFFFFF, good) == -1
    for kw in BAD:
        assert host(w, h, rt3.display_params(**kw)) == -1, kw
    for bits in (2, 3, 0x80000000):
        bad = rt3.display_params()
        bad.flags = bits
        assert host(w, h, bad) == -1, bits
    assert b"flags" in L.rt3_last_error(ctx)
    assert (out == 9).all()                                                          # a refused call writes nothing
    assert host(w, h, good) == 0 and (out != 9).all()
    assert host(w, h, rt3.display_params(white=np.inf, trim_low=1023, trim_high=0, exposure=1e-30, key=1e30)) == 0

    d = torch.zeros(w * h * 8 + 64, dtype=torch.float32, device="cuda")
    base = d.data_ptr()
    c, o = base, base + w * h * 16

    def dev(c_, o_, p=good, w_=w, h_=h):
        return L.rt3_display_device(ctx, w_, h_, C.c_void_p(c_), C.byref(p) if p is not None else None, C.c_void_p(o_), None)

    assert dev(c, o) == 0
    assert dev(c + 4, o) == -1 and dev(c + 8, o) == -1 and dev(c, o + 2) == -1 and dev(c, o + 1) == -1     # alignment: 16 bytes in, 4 bytes out
    assert dev(c, o + 4) == 0                                                        # (4 bytes are enough for the output)
    assert dev(c, c) == -1 and dev(c, c + w * h * 16 - 4) == -1                                            # the output overlaps the input
    assert dev(c + w * h * 4 - 16, c) == -1                                                                # (the input begins in the output's last bytes)
    assert dev(c + w * h * 4, c) == 0 and dev(c, c + w * h * 16) == 0                                      # one right behind the other is fine
    assert dev(None, o) == -1 and dev(c, None) == -1 and dev(c, o, None) == -1
    assert dev(c, o, w_=8193, h_=8192) == -1
    torch.cuda.synchronize()
    with pytest.raises(rt3.Fatal, match="white"):
        renderer.display(frame, "reinhard", white=0.0)
    with pytest.raises(rt3.Fatal):
        renderer.display(frame[..., :3])
    fresh = rt3.initialize_renderer(0)                                               # no scene needed; no state before the first auto call
    try:
        hist, dark, gain = np.full(512, 9, U), C.c_uint32(9), C.c_float(9.0)
        state = lambda: L.rt3_debug_display_state(fresh._ctx, hist.ctypes.data_as(C.c_void_p), C.byref(dark), C.byref(gain))
        assert state() == -4                                                        # RT3_E_STATE
        fresh.display(frame, "filmic", "srgb")
        assert state() == -4 and (hist == 9).all() and dark.value == 9 and gain.value == 9.0     # a call without the flag is not one
        assert fresh.display(frame, auto=True).tobytes() == renderer.display(frame, auto=True).tobytes()
        assert state() == 0 and hist.sum() + dark.value == w * h
        assert L.rt3_debug_display_state(fresh._ctx, None, None, None) == 0
    finally:
        fresh.close()
