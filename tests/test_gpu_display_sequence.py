"""Display sequences (rt3_display_sequence*) on the GPU, word for word and bit for bit against tests/display_sequence_ref.py: the anchor
to rt3_display, the exposure's chain through one device record, the bloom pyramid's U_1 and B and the words behind them, the cases where bloom must
change nothing, repeatability and the host / device / stream / numpy / torch forms, the accumulation and the stats left alone, the refusals, and the
command line's --display-frames, --adapt and --bloom."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_ref as D
import display_sequence_ref as R
from test_display_ref import BAD, PAIRS
from test_display_sequence_ref import BAD_SEQUENCE, BLOOM_SIZES, same_bits, special
from test_gpu_display import frame_of, set_spheres, words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")
F, U = np.float32, np.uint32
VP = C.c_void_p
BIG = (1031, 509)                                                                     # just over both grid caps: every grid-stride loop turns (test_gpu_display.py)


def state_of(t):
    """A 16-byte device tensor -> (level, frames, gain float32, pad)."""
    w = t.cpu().numpy().view(U)
    return int(w[0]), int(w[1]), w[2:3].view(F)[0], int(w[3])


def check_state(got, ref):
    level, frames, gain = (int(got["level"]), int(got["frames"]), got["gain"]) if isinstance(got, np.void) else got[:3]
    assert (level, frames) == (ref[0], ref[1]) and same_bits(gain, ref[2]), (got, ref)


# ------------------------------------------------------------------------------------------------ 1: the anchor to rt3_display
@pytest.mark.parametrize("size", [(1, 1), (67, 3), BIG], ids=lambda s: "%dx%d" % s)
def test_without_bloom_and_history_it_is_rt3_display(rt3, renderer, size):
    import torch
    w, h = size
    frame = frame_of("special", w, h, 7 * w + h)
    d_frame = torch.from_numpy(frame).cuda()
    for auto in (False, True):
        kw = dict(curve="reinhard", transfer="srgb", exposure=0.75, auto=auto, white=2.0)
        plain = words(renderer.display(d_frame, **kw))
        got, state = renderer.display_sequence(d_frame, **kw)
        assert np.array_equal(words(got), plain)
        level, frames, gain, pad = state_of(state)
        if auto:
            assert same_bits(gain, renderer.display_state()[2]) and frames == 1 and level == R.target(D.histogram(frame.reshape(-1, 4))[0])[1] and pad == 0
            for prev in ((0, 5), (R.MAX_LEVEL, 1), (level, 0xFFFFFFFF), (0xFFFFFFFF, 3)):          # rates of 1024: any history is forgotten (the last is read as 511 << 19)
                d_prev = torch.from_numpy(np.array([prev[0], prev[1], 0, 0], U).view(np.int32)).cuda()
                again, s2 = renderer.display_sequence(d_frame, d_prev, adapt=(1024, 1024), **kw)
                assert np.array_equal(words(again), plain)
                assert state_of(s2)[0] == level and same_bits(state_of(s2)[2], gain) and state_of(s2)[1] == min(prev[1] + 1, 0xFFFFFFFF)
        else:
            assert (level, frames, pad) == (0, 0, 0) and gain == F(0.75)
    dark = frame_of("dark", w, h, 3)                                                   # n == 0: nothing is set, the gain is the exposure
    got, state = renderer.display_sequence(dark, auto=True, exposure=0.5)
    assert np.array_equal(got, renderer.display(dark, auto=True, exposure=0.5))
    assert (int(state["level"]), int(state["frames"]), int(state["_pad"])) == (0, 0, 0) and state["gain"] == F(0.5)


# ------------------------------------------------------------------------------------------------ 2: the exposure on the device
def test_a_chain_through_one_device_record(rt3, renderer):
    import torch
    w, h = 320, 203
    rng = np.random.default_rng(2)
    dim = (rng.uniform(0.5, 2.0, (h, w, 4)) * 0.01).astype(F)
    lit = (rng.uniform(0.5, 2.0, (h, w, 4)) * 8.0).astype(F)
    black = frame_of("dark", w, h, 9)
    chain = [dim, lit, lit, black, dim, dim]
    record = torch.zeros(4, dtype=torch.int32, device="cuda")                              # frames == 0: no level yet
    out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    params = rt3.display_sequence_params("filmic", "srgb", auto=True, adapt=(256, 64))
    prev, levels = None, []
    for k, frame in enumerate(chain):
        d_frame = torch.from_numpy(frame).cuda()
        torch.cuda.synchronize()
        renderer.display_sequence_device(w, h, d_frame.data_ptr(), params, record.data_ptr(), record.data_ptr(), out.data_ptr())      # prev == out
        renderer.synchronize()
        ref_words, ref, _, _ = R.display_sequence(frame, prev, auto=True, adapt=(256, 64))
        got = state_of(record)
        check_state(got, ref)
        assert got[3] == 0 and np.array_equal(words(out), ref_words), k
        prev = ref
        levels.append(ref[0])
    assert levels[0] < levels[1] < levels[2] == levels[3] > levels[4] > levels[5] > levels[0]      # up, up, kept by the black frame, down, down
    assert levels[1] - levels[0] == max(1, ((R.target(D.histogram(lit.reshape(-1, 4))[0])[1] - levels[0]) * 256) >> 10)


# ------------------------------------------------------------------------------------------------ 3: the bloom on the device
@pytest.mark.parametrize("size", BLOOM_SIZES + [BIG], ids=lambda s: "%dx%d" % s)
def test_bloom_planes_equal_the_reference_bit_for_bit(rt3, renderer, size):
    import torch
    w, h = size
    frame = special(w, h, 13 * w + h)
    d_frame = torch.from_numpy(frame).cuda()
    for levels in (1, 3, 8):
        for auto in (False, True):
            bloom = (levels, 1.0, 0.5)
            got, state = renderer.display_sequence(d_frame, curve="reinhard", transfer="gamma2", exposure=0.75, auto=auto, bloom=bloom)
            ref_words, ref, ref_u1, ref_b = R.display_sequence(frame, None, D.REINHARD, D.GAMMA2, 0.75, auto, bloom_params=bloom)
            check_state(state_of(state), ref)
            u1, b = renderer.display_bloom_state()
            assert u1.shape == ((h + 1) // 2, (w + 1) // 2, 4) and b.shape == (h, w, 4)
            assert same_bits(u1[..., :3], ref_u1), (levels, auto)
            assert same_bits(b[..., :3], ref_b), (levels, auto)
            assert np.array_equal(words(got), ref_words), (levels, auto)
    assert w * h < 4 or (ref_b > 0).any()


def test_bloom_words_for_every_curve_and_transfer(rt3, renderer):
    w, h = 320, 203
    frame = special(w, h, 77)
    plain = {}
    for curve, transfer in PAIRS:
        got, _ = renderer.display_sequence(frame, curve=curve, transfer=transfer, auto=True, key=0.25, white=2.0, bloom=(3, 0.5, 0.75))
        ref = R.display_sequence(frame, None, D.CURVES[curve], D.TRANSFERS[transfer], auto=True, key=0.25, white=2.0, bloom_params=(3, 0.5, 0.75))[0]
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (curve, transfer, len(bad), bad[:3])
        plain[curve, transfer] = renderer.display(frame, curve, transfer, auto=True, key=0.25, white=2.0)
        assert (got != plain[curve, transfer]).any()                                     # (the bloom shows in the words)


# ------------------------------------------------------------------------------------------------ 4: where bloom must change nothing
def test_no_op_bloom_gives_the_words_without_bloom(rt3, renderer):
    w, h = 257, 5
    lit = special(w, h, 4)
    plain = renderer.display(lit, "filmic", "srgb", auto=True)
    got, _ = renderer.display_sequence(lit, auto=True, bloom=(3, 1.0, 0.0))              # intensity 0: x + 0 * B = x
    assert np.array_equal(got, plain)
    assert renderer.display_bloom_state()[1].any()                                       # (B itself is not zero)
    low = lit.copy()
    low[..., :3] = np.clip(np.nan_to_num(low[..., :3], nan=0.0, posinf=1.0, neginf=0.0), 0.0, 0.9)
    for levels in (1, 8):
        got, _ = renderer.display_sequence(low, exposure=1.0, bloom=(levels, 1.0, 4.0))      # nothing above the threshold: B == 0
        assert np.array_equal(got, renderer.display(low, "filmic", "srgb"))
        u1, b = renderer.display_bloom_state()
        assert not u1.any() and not b.any()


# ------------------------------------------------------------------------------------------------ 5: repeatability and the forms
def test_two_calls_and_all_forms_are_equal(rt3, renderer):
    import torch
    L = rt3.lib()
    w, h = 257, 5
    frame = special(w, h, 8)
    d_frame = torch.from_numpy(frame).cuda()
    kw = dict(curve="filmic", transfer="srgb", auto=True, exposure=0.5, adapt=(300, 100), bloom=(4, 0.75, 0.5))
    prev = np.array((150 << 19, 3, 1.0, 0), rt3.EXPOSURE)
    host, s_host = renderer.display_sequence(frame, prev, **kw)
    host2, s_host2 = renderer.display_sequence(frame, prev, **kw)
    assert host.tobytes() == host2.tobytes() and s_host.tobytes() == s_host2.tobytes()          # the pyramid and the state hold nothing of the call before
    ref_words, ref, _, _ = R.display_sequence(frame, (150 << 19, 3), D.FILMIC, D.SRGB, 0.5, True, adapt=(300, 100), bloom_params=(4, 0.75, 0.5))
    assert host.dtype == U and np.array_equal(host, ref_words)
    check_state(s_host, ref)
    d_prev = torch.from_numpy(prev.reshape(1).view(np.int32).copy()).cuda()
    t, s_t = renderer.display_sequence(d_frame, d_prev, **kw)                              # torch == numpy
    assert t.is_cuda and s_t.is_cuda and np.array_equal(words(t), host) and s_t.cpu().numpy().tobytes() == s_host.tobytes()
    p = rt3.display_sequence_params(**kw)
    out, rec = torch.zeros((h, w), dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    renderer.display_sequence_device(w, h, d_frame.data_ptr(), p, d_prev.data_ptr(), rec.data_ptr(), out.data_ptr())      # NULL: the context's own stream
    renderer.synchronize()
    assert np.array_equal(words(out), host) and rec.cpu().numpy().tobytes() == s_host.tobytes()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out2, rec2 = torch.zeros((h, w), dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        assert L.rt3_display_sequence_device(renderer._ctx, w, h, VP(d_frame.data_ptr()), C.byref(p), VP(d_prev.data_ptr()), VP(rec2.data_ptr()),
                                             VP(out2.data_ptr()), VP(s.cuda_stream)) == 0
    s.synchronize()
    assert np.array_equal(words(out2), host) and rec2.cpu().numpy().tobytes() == s_host.tobytes()
    renderer.display_sequence_device(w, h, d_frame.data_ptr(), p, d_prev.data_ptr(), 0, out.data_ptr())                    # no out_exposure wanted
    renderer.synchronize()
    assert np.array_equal(words(out), host)


def test_progressive_render_and_stats_across_a_call(rt3, renderer):
    w, h = 48, 32
    set_spheres(rt3, renderer, *rt3.scene_three_spheres())
    cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=3, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_VARIANCE)
    one = renderer.render_path(cam.c, p)
    acc1, sq1, _ = renderer.accum_download(p, want_sq=True)
    renderer.render_path_range(cam.c, p, 0, 2)
    st = renderer.stats()
    frame = special(w + 9, h + 5, 4)
    _, state = renderer.display_sequence(frame, auto=True, bloom=(3, 1.0, 0.25))
    renderer.display_sequence(frame, state, auto=True)
    renderer.display_bloom_state()
    assert bytes(renderer.stats()) == bytes(st)
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 2), one)
    acc2, sq2, done = renderer.accum_download(p, want_sq=True)
    assert done == 4 and acc1.tobytes() == acc2.tobytes() and sq1.tobytes() == sq2.tobytes()


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_argument_errors(rt3, renderer):
    import torch
    L = rt3.lib()
    ctx = renderer._ctx
    w, h = 8, 4
    frame = frame_of("tail", w, h, 1)
    out = np.full((h, w), 9, U)
    state = np.full(4, 9, U)
    prev = np.array([(100 << 19, 2, 1.0, 0)], rt3.EXPOSURE)
    good = rt3.display_sequence_params(auto=True, bloom=(2, 0.05, 0.25))

    def ptr(a):
        return a.ctypes.data_as(VP) if a is not None else None

    def host(w_, h_, p, c=frame, o=out, pv=prev, s=state):
        return L.rt3_display_sequence(ctx, w_, h_, ptr(c), C.byref(p) if p is not None else None, ptr(pv), ptr(s), ptr(o))

    assert host(w, h, None) == -1 and host(w, h, good, c=None) == -1 and host(w, h, good, o=None) == -1
    assert host(0, h, good) == -1 and host(w, 0, good) == -1 and host(8193, 8192, good) == -1 and host(0xFFFFFFFF, 0xFFFFFFFF, good) == -1
    for kw in BAD:
        assert host(w, h, rt3.display_sequence_params(auto=True, **kw)) == -1, kw
    for kw in BAD_SEQUENCE:
        assert host(w, h, rt3.display_sequence_params(auto=True, **kw)) == -1, kw
    for word in range(3):
        bad = rt3.display_sequence_params(auto=True)
        bad._pad[word] = 0x80000000
        assert host(w, h, bad) == -1, word
    assert b"_pad" in L.rt3_last_error(ctx)
    bad = rt3.display_sequence_params(auto=True)
    bad.display.flags = 3
    assert host(w, h, bad) == -1
    assert host(w, h, rt3.display_sequence_params(auto=False)) == -1 and b"prev_exposure" in L.rt3_last_error(ctx)      # prev without the flag
    assert host(w, h, good, pv=np.array([(R.MAX_LEVEL + 1, 2, 1.0, 0)], rt3.EXPOSURE)) == -1                            # a host level above 511 << 19
    assert (out == 9).all() and (state == 9).all()                                    # a refused call writes nothing
    assert host(w, h, good) == 0 and (out != 9).all() and state[1] == 3 and state[3] == 0
    assert host(w, h, good, pv=None, s=None) == 0                                      # both records are optional
    assert host(w, h, rt3.display_sequence_params(auto=False), pv=None) == 0 and tuple(state) == (0, 0, np.array([1.0], F).view(U)[0], 0)
    both = prev.copy()
    assert host(w, h, good, pv=both, s=both.view(U)) == 0 and int(both[0]["frames"]) == 3      # prev == out on the host too

    n = w * h
    d = torch.zeros(n * 8 + 64, dtype=torch.float32, device="cuda")
    d.view(torch.int32)[n * 5 + 1] = 2                                                 # the record at e: level 0, frames 2
    base = d.data_ptr()
    c, o, e, e2 = base, base + n * 16, base + n * 20, base + n * 20 + 16
    torch.cuda.synchronize()

    def dev(c_=c, o_=o, pv=e, s=e2, p=good, w_=w, h_=h):
        return L.rt3_display_sequence_device(ctx, w_, h_, VP(c_), C.byref(p) if p is not None else None, VP(pv), VP(s), VP(o_), None)

    assert dev() == 0 and dev(s=e) == 0 and dev(pv=None, s=None) == 0
    assert dev(c_=c + 4) == -1 and dev(c_=c + 8) == -1 and dev(o_=o + 2) == -1 and dev(pv=e + 2) == -1 and dev(s=e2 + 1) == -1      # alignment
    assert dev(o_=o + 4, pv=e + 4, s=e2 + 4) == 0                                                                  # (4 bytes are enough for the three)
    assert dev(o_=c) == -1 and dev(o_=c + n * 16 - 4) == -1 and dev(c_=c + n * 4 - 16, o_=c) == -1                 # the words overlap the frame
    assert dev(pv=c) == -1 and dev(s=c + 16) == -1 and dev(pv=o + 4) == -1 and dev(s=o + n * 4 - 4) == -1           # a record in the frame, in the words
    assert dev(pv=e, s=e + 4) == -1 and dev(pv=e + 12, s=e) == -1                                                  # the records overlap without being one
    assert dev(c_=None) == -1 and dev(o_=None) == -1 and dev(p=None) == -1 and dev(w_=8193, h_=8192) == -1
    assert dev(p=rt3.display_sequence_params(auto=False)) == -1 and dev(p=rt3.display_sequence_params(auto=False), pv=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(rt3.Fatal, match="bloom_levels"):
        renderer.display_sequence(frame, bloom=(9, 1.0, 0.25))
    with pytest.raises(rt3.Fatal):
        renderer.display_sequence(frame[..., :3])
    with pytest.raises(rt3.Fatal):
        renderer.display_sequence(torch.from_numpy(frame).cuda(), prev[0], auto=True)      # a host record with a device frame
    fresh = rt3.initialize_renderer(0)                                                 # no scene needed; no pyramid before the first call with bloom
    try:
        u1, b, fw, fh = np.full(n * 4, 9.0, F), np.full(n * 4, 9.0, F), C.c_uint32(9), C.c_uint32(9)
        bloom = lambda cap: L.rt3_debug_display_bloom(fresh._ctx, ptr(u1), ptr(b), cap, C.byref(fw), C.byref(fh))
        assert bloom(n) == -4                                                          # RT3_E_STATE
        fresh.display_sequence(frame, auto=True)
        assert bloom(n) == -4 and (u1 == 9).all() and (b == 9).all() and fw.value == 9    # a call without bloom is not one
        with pytest.raises(rt3.Fatal):
            fresh.display_bloom_state()
        got, _ = fresh.display_sequence(frame, prev[0], auto=True, bloom=(2, 0.05, 0.25))
        assert got.tobytes() == renderer.display_sequence(frame, prev[0], auto=True, bloom=(2, 0.05, 0.25))[0].tobytes()
        assert bloom(n - 1) == -1 and (fw.value, fh.value) == (w, h) and (b == 9).all()   # a short capacity: the size is reported
        assert bloom(n) == 0 and (b.reshape(h, w, 4)[..., :3] > 0).any()
        assert L.rt3_debug_display_bloom(fresh._ctx, None, None, n, C.byref(fw), C.byref(fh)) == 0
        assert L.rt3_debug_display_bloom(fresh._ctx, ptr(u1), ptr(b), n, None, C.byref(fh)) == -1
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 7: the command line
def rgb(w):
    return np.stack([w >> 24, (w >> 16) & 0xFF, (w >> 8) & 0xFF], -1).astype(np.uint8)


def read_pfm(path, w, h):
    """A 3-channel little-endian PFM (rows bottom to top) -> (h, w, 4) float32, the fourth float 0."""
    raw = open(path, "rb").read()
    body = np.frombuffer(raw[-12 * w * h:], "<f4").reshape(h, w, 3)[::-1]
    return np.concatenate([body, np.zeros((h, w, 1), F)], -1).astype(F)


@pytest.mark.parametrize("lens", [False, True], ids=["camera", "equirect"])
def test_cli_writes_an_image_per_frame(rt3, renderer, tmp_path, lens):
    w, h = 64, 48
    sequence = ["--lens", "equirect", "--lens-frames", "3"] if lens else ["--frames", "3"]
    cmd = [EXE, "--scene", "weekend", "-W", str(w), "-H", str(h), "--spp", "1", "-f", "ppm"] + sequence + [
        "--orbit", "10", "--denoise", "P", "--display", "filmic,srgb,auto", "--adapt", "256,64", "--bloom", "3,1,0.5", "--display-frames", "Q", "last.ppm"]
    subprocess.run(cmd, cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    prev = None
    for k in range(3):
        frame = read_pfm(str(tmp_path / ("P.%d.pfm" % k)), w, h)
        got, prev = renderer.display_sequence(frame, prev, curve="filmic", transfer="srgb", auto=True, adapt=(256, 64), bloom=(3, 1.0, 0.5))
        image = np.frombuffer((tmp_path / ("Q.%d.ppm" % k)).read_bytes()[-3 * w * h:], np.uint8).reshape(h, w, 3)
        assert np.array_equal(image, rgb(got)), k
        assert int(prev["frames"]) == k + 1
    assert not (tmp_path / "Q.3.ppm").exists() and (tmp_path / "last.ppm").exists()


def test_cli_without_the_new_options_is_unchanged(rt3, renderer, tmp_path):
    w, h = 64, 48
    base = [EXE, "--scene", "three", "--spp", "4", "-W", str(w), "-H", str(h), "-f", "ppm", "--display", "reinhard,srgb,auto", "--hdr", "H.pfm"]
    subprocess.run(base + ["a.ppm"], cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    subprocess.run(base + ["--bloom", "4,0.05,1", "b.ppm"], cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    lin = read_pfm(str(tmp_path / "H.pfm"), w, h)

    def ppm(name):
        return np.frombuffer((tmp_path / name).read_bytes()[-3 * w * h:], np.uint8).reshape(h, w, 3)

    assert np.array_equal(ppm("a.ppm"), rgb(renderer.display(lin, "reinhard", "srgb", auto=True)))      # rt3_display, as before
    assert np.array_equal(ppm("b.ppm"), rgb(renderer.display_sequence(lin, curve="reinhard", transfer="srgb", auto=True, bloom=(4, 0.05, 1.0))[0]))
    assert not np.array_equal(ppm("a.ppm"), ppm("b.ppm"))                                # --bloom acts on the single image (the key is 0.18: much of it is above 0.05)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["H.pfm", "a.ppm", "b.ppm"]
