"""The temporal denoiser (rt3_denoise_temporal*) on the GPU: agreement with the numpy restatement (tests/temporal_ref.py) on
synthetic frames and rendered moving-camera sequences, no history = rt3_denoise bit for bit, the host / device / torch forms, the accumulation
and the stats left alone, argument errors, a quality floor against a high-spp frame, and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as T
from test_denoise_abi import synthetic
from test_gpu_denoise import bits, check_close, mse, set_mesh, set_spheres

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")


def check_history(got, ref):
    """length exactly; the float fields within the bound of check_close; depth and normal bit for bit."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert np.array_equal(got["length"], ref["length"]), "length differs at %d pixels" % int((got["length"] != ref["length"]).sum())
    assert np.array_equal(bits(got["depth"]), bits(ref["depth"])) and np.array_equal(bits(got["normal"]), bits(ref["normal"]))
    for f in ("colour", "moments"):
        a, b = got[f].astype(np.float64), ref[f].astype(np.float64)
        assert np.isfinite(a).all() and (np.abs(a - b) <= 1e-5 * np.abs(b) + 1e-6).all(), f
    assert not got["_pad0"].any() and not got["_pad1"].any()


def orbit_camera(rt3, w, h, deg, at=(0.0, 0.0, 0.0), look_from=(13.0, 2.0, 3.0)):
    a = np.radians(deg)
    dx, dz = look_from[0] - at[0], look_from[2] - at[2]
    f = (at[0] + (np.cos(a) * dx + np.sin(a) * dz), look_from[1], at[2] + (np.cos(a) * dz - np.sin(a) * dx))
    return rt3.Camera().look_at(w, h, f, at, vfov=20.0, focus_dist=10.0)


def perturbed(rt3, cam_c, scale, seed):
    """A copy of camera_c moved and turned a little (synthetic sequences)."""
    rng = np.random.default_rng(seed)
    c = rt3.rt3_camera.from_buffer_copy(bytes(cam_c))
    for f in ("origin", "horizontal", "vertical", "lower_left_corner"):
        v = getattr(c, f)
        for i in range(3):
            v[i] = float(np.float32(v[i] + scale * rng.normal()))
    return c


# ------------------------------------------------------------------------------------------------ 1: agreement with the restatement
PARAMS = [{}, dict(iterations=1, alpha=0.5, moments_alpha=0.1), dict(iterations=3, normal_power=16, sigma_luminance=2.0, depth_tolerance=8.0,
                                                                    normal_tolerance=0.5)]


@pytest.mark.parametrize("size", [(2, 2), (31, 17), (96, 64)])
@pytest.mark.parametrize("kw", PARAMS)
def test_agrees_with_the_restatement_on_synthetic_sequences(rt3, renderer, size, kw):
    w, h = size
    cam = orbit_camera(rt3, w, h, 0.0).c
    gpu_prev = ref_prev = None
    for k in range(4):
        colour, aov = synthetic(rt3, h, w, 1000 * k + w)
        if k:
            aov["depth"] = ref_prev[0]["depth"] * np.float32(1.0 + 1e-4 * k)     # mostly consistent with the last frame
            aov["normal"] = ref_prev[0]["normal"]
        c = cam if k % 2 else perturbed(rt3, cam, 0.002 * k, k)              # even frames move, odd frames keep the camera
        got, gh = renderer.denoise_temporal(colour, aov, c, gpu_prev, **kw)
        want, wh = T.denoise_temporal(colour, aov, c, ref_prev, **kw)
        check_close(got, want)
        check_history(gh[0], wh)
        gpu_prev, ref_prev = gh, (wh, c)
        cam = c
    if w * h >= 64:
        assert (wh["length"] > 1).any()


@pytest.mark.parametrize("scene,kw", [("cornell", {}), ("weekend", {}), ("weekend", PARAMS[2])])
def test_agrees_with_the_restatement_on_rendered_sequences(rt3, renderer, scene, kw):
    w, h = 96, 72
    if scene == "cornell":
        set_mesh(rt3, renderer, *rt3.scene_cornell(16))
        cams = [rt3.main_camera(w, h)] * 3
        flags, lens = rt3.FLAG_BLACK_BACKGROUND, 0.0
    else:
        set_spheres(rt3, renderer, *rt3.scene_weekend(42))
        cams = [orbit_camera(rt3, w, h, 1.5 * k) for k in range(3)]
        flags, lens = 0, 0.05
    gpu_prev = ref_prev = None
    for k, cam in enumerate(cams):
        p = rt3.make_params(w, h, spp=2, max_depth=8, seed=10 + k, flags=flags, lens_radius=lens)
        renderer.render_path(cam.c, p)
        lin, aov = renderer.accum_resolve(p), renderer.render_aov(cam.c, p)
        got, gh = renderer.denoise_temporal(lin, aov, cam.c, gpu_prev, **kw)
        want, wh = T.denoise_temporal(lin, aov, cam.c, ref_prev, **kw)
        check_close(got, want)
        check_history(gh[0], wh)
        gpu_prev, ref_prev = gh, (wh, cam.c)
    share = float((wh["length"] == 3).mean())
    print("%s: %.3f of the pixels have 3 frames of history" % (scene, share))
    assert share > 0.5


# ------------------------------------------------------------------------------------------------ 2: no history, a still camera
def test_no_history_is_rt3_denoise_bit_for_bit(rt3, renderer):
    w, h = 70, 45
    colour, aov = synthetic(rt3, h, w, 9)
    cam = orbit_camera(rt3, w, h, 0.0).c
    for kw in ({}, dict(iterations=2, normal_power=4)):
        out, (hist, _) = renderer.denoise_temporal(colour, aov, cam, None, **kw)
        assert np.array_equal(bits(out), bits(renderer.denoise(colour, aov, **kw)))
        assert (hist["length"] == 1).all()
        bad = hist.copy()
        bad["depth"] = np.where(np.isinf(bad["depth"]), np.float32(1.0), bad["depth"] + np.float32(1000.0))   # every tap inconsistent
        bad["colour"] = 1e6
        out2, (hist2, _) = renderer.denoise_temporal(colour, aov, cam, (bad, cam), **kw)
        assert np.array_equal(bits(out2), bits(out)) and (hist2["length"] == 1).all()


def test_a_still_camera_counts_up_and_averages(rt3, renderer):
    w, h = 40, 30
    cam = orbit_camera(rt3, w, h, 0.0).c
    values = [1.0, 2.0, 3.0, 6.0, 0.5]
    prev = None
    for k, val in enumerate(values):
        colour = np.zeros((h, w, 4), np.float32)
        colour[..., :3] = val
        aov = np.zeros((h, w), rt3.AOV)
        aov["albedo"], aov["normal"], aov["depth"], aov["coverage"] = (1.0, 1.0, 1.0), (0.0, 0.0, 1.0), 7.0, 1.0
        out, prev = renderer.denoise_temporal(colour, aov, cam, prev)
        assert (prev[0]["length"] == k + 1).all()
        assert np.allclose(out[..., :3], np.mean(values[: k + 1]), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ 3: the forms
def test_host_device_and_torch_forms_are_equal(rt3, renderer):
    import torch
    L = rt3.lib()
    w, h = 61, 37
    cam0 = orbit_camera(rt3, w, h, 0.0).c
    cam1 = perturbed(rt3, cam0, 0.001, 5)
    c0, a0 = synthetic(rt3, h, w, 21)
    c1, a1 = synthetic(rt3, h, w, 22)
    a1["depth"], a1["normal"] = a0["depth"], a0["normal"]
    o0, h0 = renderer.denoise_temporal(c0, a0, cam0, None, iterations=3)
    o1, h1 = renderer.denoise_temporal(c1, a1, cam1, h0, iterations=3)
    assert (h1[0]["length"] == 2).any()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(h, w, -1)).cuda()    # noqa: E731
    t0, th0 = renderer.denoise_temporal(t(c0), t(a0), cam0, None, iterations=3)
    t1, th1 = renderer.denoise_temporal(t(c1), t(a1), cam1, th0, iterations=3)
    assert t1.shape == (h, w, 4) and t1.dtype == torch.float32 and t1.is_cuda
    assert t0.cpu().numpy().tobytes() == o0.tobytes() and t1.cpu().numpy().tobytes() == o1.tobytes()
    assert th1[0].cpu().numpy().tobytes() == h1[0].tobytes()
    s = torch.cuda.Stream()
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(3, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9)
    d_c, d_a, d_h = t(c1), t(a1), t(h0[0])
    with torch.cuda.stream(s):
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        hist = torch.zeros((h, w, 12), dtype=torch.float32, device="cuda")
        assert L.rt3_denoise_temporal_device(renderer._ctx, w, h, C.byref(cam1), C.c_void_p(d_c.data_ptr()), C.c_void_p(d_a.data_ptr()),
                                             C.byref(cam0), C.c_void_p(d_h.data_ptr()), C.byref(p), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(hist.data_ptr()), C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert out.cpu().numpy().tobytes() == o1.tobytes() and hist.cpu().numpy().tobytes() == h1[0].tobytes()
    with pytest.raises(rt3.Fatal, match="48-byte"):
        renderer.denoise_temporal(t(c1), t(a1), cam1, (th0[0][:, :, :4].contiguous(), cam0))


# ------------------------------------------------------------------------------------------------ 4: accumulation and stats untouched
def test_progressive_render_continues_across_a_temporal_denoise(rt3, renderer):
    w, h = 48, 32
    set_mesh(rt3, renderer, *rt3.scene_cornell(16))
    cam = rt3.main_camera(w, h)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=3, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND | rt3.FLAG_VARIANCE)
    one = renderer.render_path(cam.c, p)
    acc1, sq1, _ = renderer.accum_download(p, want_sq=True)
    renderer.render_path_range(cam.c, p, 0, 2)
    st = renderer.stats()
    colour, aov = synthetic(rt3, h + 5, w + 9, 4)
    c2 = orbit_camera(rt3, w + 9, h + 5, 0.0).c
    _, prev = renderer.denoise_temporal(colour, aov, c2, None)
    renderer.denoise_temporal(colour, aov, c2, prev)
    assert bytes(renderer.stats()) == bytes(st)
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 2), one)
    acc2, sq2, done = renderer.accum_download(p, want_sq=True)
    assert done == 4 and acc1.tobytes() == acc2.tobytes() and sq1.tobytes() == sq2.tobytes()


# ------------------------------------------------------------------------------------------------ 5: argument errors
def test_argument_errors(rt3, renderer):
    import torch
    L = rt3.lib()
    ctx = renderer._ctx
    w, h = 8, 4
    colour, aov = synthetic(rt3, h, w, 1)
    cam = orbit_camera(rt3, w, h, 0.0).c
    out = np.zeros((h, w, 4), np.float32)
    hist = np.zeros((h, w), rt3.HISTORY)
    prev = np.zeros((h, w), rt3.HISTORY)

    def P(*spatial, alpha=0.2, moments_alpha=0.2, dtol=2.0, ntol=0.9):
        return rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(*(spatial or (5, 128, 4.0, 1.0))), alpha, moments_alpha, dtol, ntol)

    good = P()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731

    def host(w_=w, h_=h, p=good, c=cam, pc=None, ph=None, o=out, oh=hist, col=colour, a=aov):
        return L.rt3_denoise_temporal(ctx, w_, h_, C.byref(c) if c is not None else None, ptr(col), ptr(a),
                                      C.byref(pc) if pc is not None else None, ptr(ph), C.byref(p) if p is not None else None, ptr(o), ptr(oh))

    assert host() == 0 and host(pc=cam, ph=prev) == 0
    assert host(p=None) == -1 and host(c=None) == -1 and host(col=None) == -1 and host(a=None) == -1
    assert host(o=None) == -1 and host(oh=None) == -1
    assert host(pc=cam) == -1 and host(ph=prev) == -1                   # prev_cam and prev_history: both or neither
    assert host(1, h) == -1 and host(w, 1) == -1 and host(8193, 8192) == -1
    for bad in (P(0, 128, 4.0, 1.0), P(5, 96, 4.0, 1.0), P(5, 128, 0.0, 1.0), P(5, 128, 4.0, float("nan")),
                P(alpha=0.0), P(alpha=1.5), P(alpha=float("nan")), P(moments_alpha=0.0), P(moments_alpha=2.0),
                P(dtol=0.0), P(dtol=-1.0), P(dtol=float("inf")), P(dtol=float("nan")), P(ntol=1.01), P(ntol=-1.5), P(ntol=float("nan"))):
        assert host(p=bad) == -1
    for ok in (P(alpha=1.0, moments_alpha=1e-30, dtol=1e30, ntol=-1.0), P(ntol=1.0)):
        assert host(p=ok) == 0
    for field, i, value in (("origin", 0, float("inf")), ("horizontal", 1, float("nan")), ("lower_left_corner", 2, float("-inf"))):
        c = rt3.rt3_camera.from_buffer_copy(bytes(cam))
        getattr(c, field)[i] = value
        assert host(c=c) == -1 and host(pc=c, ph=prev) == -1, field
    flat = rt3.rt3_camera.from_buffer_copy(bytes(cam))
    for i in range(3):
        flat.vertical[i] = 2.0 * flat.horizontal[i]                            # horizontal x vertical = 0
    through = rt3.rt3_camera.from_buffer_copy(bytes(cam))
    for i in range(3):
        through.lower_left_corner[i] = through.origin[i] + through.horizontal[i]   # the image plane contains the origin
    for c in (flat, through):
        assert host(c=c) == -1 and host(pc=c, ph=prev) == -1
    assert host(o=colour) == -1 and host(oh=prev, pc=cam, ph=prev) == -1    # an output aliases an input
    shared = np.zeros((h, w), rt3.HISTORY)
    assert host(o=shared.view(np.float32), oh=shared) == -1                  # the two outputs share a buffer

    n = w * h
    d = torch.zeros(n * 4 * 16 + 64, dtype=torch.float32, device="cuda")
    base = d.data_ptr()
    c_, a_, ph_, o_, oh_ = base, base + n * 16, base + n * 64, base + n * 112, base + n * 128

    def dev(c=c_, a=a_, ph=ph_, o=o_, oh=oh_, pc=cam):
        return L.rt3_denoise_temporal_device(ctx, w, h, C.byref(cam), C.c_void_p(c), C.c_void_p(a), C.byref(pc) if pc is not None else None,
                                             C.c_void_p(ph) if ph is not None else None, C.byref(good), C.c_void_p(o), C.c_void_p(oh), None)

    assert dev() == 0 and dev(pc=None, ph=None) == 0
    assert dev(c=c_ + 4) == -1 and dev(a=a_ + 8) == -1 and dev(ph=ph_ + 4) == -1 and dev(o=o_ + 4) == -1 and dev(oh=oh_ + 4) == -1
    assert dev(o=c_) == -1 and dev(o=a_ + 32) == -1 and dev(o=ph_ + 16) == -1                 # the frame overlaps an input
    assert dev(oh=a_) == -1 and dev(oh=ph_) == -1 and dev(oh=c_ + 16) == -1                   # the history overlaps an input
    assert dev(oh=o_ + 16) == -1 and dev(oh=o_ - 16) == -1                                    # the outputs overlap each other
    assert dev(c=0) == -1 and dev(o=0) == -1 and dev(oh=0) == -1
    torch.cuda.synchronize()
    with pytest.raises(rt3.Fatal, match="normal_tolerance"):
        renderer.denoise_temporal(colour, aov, cam, None, normal_tolerance=2.0)
    fresh = rt3.initialize_renderer(0)                                 # no scene needed
    try:
        assert fresh.denoise_temporal(colour, aov, cam)[0].tobytes() == renderer.denoise_temporal(colour, aov, cam)[0].tobytes()
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 6: quality floor
# An 8-frame weekend orbit (1 degree per frame) at 320x240 and 1 spp per frame; the last frame against a 1024-spp frame of its camera.
# Measured on an MI355X (profiles/temporal_bench_mi355x.log): MSE 0.00312 for rt3_denoise of the last frame alone, 0.00211 for the temporal
# output (x1.48; raw 1-spp frame 0.0115).  The run is deterministic; the bound leaves headroom for a change of the filter's constants.
QUALITY_BOUND = 1.25


def test_temporal_output_is_closer_to_a_high_spp_frame_than_the_spatial_one(rt3, renderer):
    w, h = 320, 240
    set_spheres(rt3, renderer, *rt3.scene_weekend(42))
    prev = None
    for k in range(8):
        cam = orbit_camera(rt3, w, h, float(k))
        p = rt3.make_params(w, h, spp=1, max_depth=50, seed=100 + k, lens_radius=0.05)
        renderer.render_path(cam.c, p)
        lin, aov = renderer.accum_resolve(p), renderer.render_aov(cam.c, p)
        out, prev = renderer.denoise_temporal(lin, aov, cam.c, prev)
    spatial = renderer.denoise(lin, aov)
    pr = rt3.make_params(w, h, spp=1024, max_depth=50, seed=7, lens_radius=0.05)
    renderer.render_path(cam.c, pr)
    ref = renderer.accum_resolve(pr)
    m_raw, m_sp, m_t = mse(lin, ref), mse(spatial, ref), mse(out, ref)
    print("weekend orbit 320x240 1 spp, frame 8: MSE raw %.5g, rt3_denoise %.5g, temporal %.5g, spatial / temporal %.3f"
          % (m_raw, m_sp, m_t, m_sp / m_t))
    assert m_sp / m_t >= QUALITY_BOUND, (m_sp, m_t)


# ------------------------------------------------------------------------------------------------ 7: the command line
def test_cli_writes_a_pfm_per_frame(tmp_path):
    w, h = 64, 48
    args = [EXE, "--scene", "weekend", "--spp", "1", "-W", str(w), "-H", str(h), "--frames", "3", "--orbit", "1", "--denoise", "P", "out.png"]
    subprocess.run(args, cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    for k in range(3):
        data = (tmp_path / ("P.%d.pfm" % k)).read_bytes()
        head = b"PF\n%d %d\n-1.0\n" % (w, h)
        assert data.startswith(head), data[:20]
        px = np.frombuffer(data[len(head):], "<f4")
        assert px.size == w * h * 3 and np.isfinite(px).all() and px.any()
    assert (tmp_path / "out.png").exists() and not (tmp_path / "P").exists()
