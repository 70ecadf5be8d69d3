"""The denoiser (rt3_denoise*) on the GPU: agreement with the numpy reference (tests/denoise_ref.py), the independence
property bit for bit, the host / device / torch forms, the accumulation and the stats left alone, argument errors, a quality floor against a
high-spp frame, and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
from test_denoise_abi import split, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def set_mesh(rt3, r, faces, verts, fmats):
    r.set_spheres(np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    r.set_mesh(faces, verts, fmats)


def set_spheres(rt3, r, cr, mats):
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    r.set_spheres(cr, mats)


def cornell_frame(rt3, r, w, h, spp, seed=1, grid=64):
    """(linear frame, AOVs) of the command line's cornell render."""
    set_mesh(rt3, r, *rt3.scene_cornell(grid))
    cam = rt3.main_camera(w, h)
    p = rt3.make_params(w, h, spp=spp, max_depth=50, seed=seed, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND)
    r.render_path(cam.c, p)
    return r.accum_resolve(p), r.render_aov(cam.c, p)


def check_close(got, ref):
    """|gpu - ref| <= 1e-5 |ref| + 1e-6 per channel; the message gives the largest error as a share of that bound."""
    assert got.shape == ref.shape and not got[..., 3].any()
    err = np.abs(got.astype(np.float64) - ref)
    bound = 1e-5 * np.abs(ref.astype(np.float64)) + 1e-6
    worst = float((err / bound).max()) if err.size else 0.0
    assert np.isfinite(got).all() and worst <= 1.0, "max |gpu - ref| / bound = %.3f (max abs error %.3g)" % (worst, err.max())
    return worst


# ------------------------------------------------------------------------------------------------ 1: agreement with the reference
CASES = [((1, 1), {}), ((2, 3), dict(iterations=3)), ((7, 5), dict(iterations=4, normal_power=1)),
         ((64, 48), {}), ((64, 48), dict(iterations=8, normal_power=1024, sigma_luminance=0.25, sigma_depth=8.0)),
         ((333, 97), dict(iterations=6, normal_power=16, sigma_luminance=10.0, sigma_depth=0.5))]


@pytest.mark.parametrize("size,kw", CASES)
def test_agrees_with_the_reference_on_synthetic_frames(rt3, renderer, size, kw):
    w, h = size
    colour, aov = synthetic(rt3, h, w, w * 1000 + h)
    print("%dx%d %s: max |gpu - ref| / bound = %.3g" % (w, h, kw, check_close(renderer.denoise(colour, aov, **kw), R.denoise(colour, aov, **kw))))


def test_agrees_with_the_reference_on_a_cornell_frame(rt3, renderer):
    lin, aov = cornell_frame(rt3, renderer, 640, 360, 4)
    check_close(renderer.denoise(lin, aov), R.denoise(lin, aov))
    check_close(renderer.denoise(lin, aov, iterations=3, normal_power=32, sigma_luminance=2.0), R.denoise(lin, aov, iterations=3,
                                                                                                      normal_power=32, sigma_luminance=2.0))


# ------------------------------------------------------------------------------------------------ 2: independence, bit for bit
@pytest.mark.parametrize("kind", ["normals", "misses"])
def test_region_a_does_not_see_region_b(rt3, renderer, kind):
    colour, aov, b = split(rt3, 70, 90, kind, 11)
    out1 = renderer.denoise(colour, aov, iterations=6)
    c2 = colour.copy()
    c2[b, :3] = np.random.default_rng(2).uniform(0.0, 100.0, (int(b.sum()), 3))
    out2 = renderer.denoise(c2, aov, iterations=6)
    assert np.array_equal(bits(out1[~b]), bits(out2[~b]))
    assert not np.array_equal(out1[b], out2[b])


# ------------------------------------------------------------------------------------------------ 3: the forms
def test_host_device_and_torch_forms_are_equal(rt3, renderer):
    import torch
    L = rt3.lib()
    w, h = 93, 41
    colour, aov = synthetic(rt3, h, w, 77)
    host = renderer.denoise(colour, aov, iterations=4)
    assert renderer.denoise(colour, aov, iterations=4).tobytes() == host.tobytes()
    d_col = torch.from_numpy(colour).cuda()
    d_aov = torch.from_numpy(aov.view(np.float32).reshape(h, w, 12)).cuda()
    t = renderer.denoise(d_col, d_aov, iterations=4)
    assert t.shape == (h, w, 4) and t.dtype == torch.float32 and t.is_cuda
    assert t.cpu().numpy().tobytes() == host.tobytes()
    s = torch.cuda.Stream()
    p = rt3.DENOISE_PARAMS(4, 128, 4.0, 1.0)
    with torch.cuda.stream(s):
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        assert L.rt3_denoise_device(renderer._ctx, w, h, C.c_void_p(d_col.data_ptr()), C.c_void_p(d_aov.data_ptr()), C.byref(p),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert out.cpu().numpy().tobytes() == host.tobytes()
    with pytest.raises(rt3.Fatal, match="48-byte"):
        renderer.denoise(d_col, d_aov[:, :, :4].contiguous())


# ------------------------------------------------------------------------------------------------ 4: accumulation and stats untouched
def test_progressive_render_continues_across_a_denoise(rt3, renderer):
    w, h = 48, 32
    set_mesh(rt3, renderer, *rt3.scene_cornell(16))
    cam = rt3.main_camera(w, h)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=3, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND | rt3.FLAG_VARIANCE)
    one = renderer.render_path(cam.c, p)
    acc1, sq1, _ = renderer.accum_download(p, want_sq=True)
    renderer.render_path_range(cam.c, p, 0, 2)
    st = renderer.stats()
    colour, aov = synthetic(rt3, h + 5, w + 9, 4)
    renderer.denoise(colour, aov)
    st2 = renderer.stats()
    assert bytes(st2) == bytes(st)
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
    out = np.zeros((h, w, 4), np.float32)
    good = rt3.DENOISE_PARAMS(5, 128, 4.0, 1.0)

    def host(w_, h_, p, c=colour, a=aov, o=out):
        return L.rt3_denoise(ctx, w_, h_, c.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), C.byref(p) if p is not None else None,
                             o.ctypes.data_as(C.c_void_p))

    assert host(w, h, good) == 0
    assert host(w, h, None) == -1
    assert host(0, h, good) == -1 and host(w, 0, good) == -1
    assert host(8193, 8192, good) == -1                                 # more than 2^26 pixels
    bad = [(0, 128, 4.0, 1.0), (9, 128, 4.0, 1.0), (5, 0, 4.0, 1.0), (5, 3, 4.0, 1.0), (5, 2048, 4.0, 1.0), (5, 96, 4.0, 1.0),
           (5, 128, 0.0, 1.0), (5, 128, -1.0, 1.0), (5, 128, float("inf"), 1.0), (5, 128, float("nan"), 1.0),
           (5, 128, 4.0, 0.0), (5, 128, 4.0, float("inf")), (5, 128, 4.0, float("nan"))]
    for fields in bad:
        assert host(w, h, rt3.DENOISE_PARAMS(*fields)) == -1, fields
    for fields in ((1, 1, 1e-30, 1e-30), (8, 1024, 1e30, 1e30)):
        assert host(w, h, rt3.DENOISE_PARAMS(*fields)) == 0, fields
    d = torch.zeros(w * h * 4 * 6 + 64, dtype=torch.float32, device="cuda")
    base = d.data_ptr()
    c, a, o = base, base + w * h * 16, base + w * h * 64

    def dev(c_, a_, o_, p=good):
        return L.rt3_denoise_device(ctx, w, h, C.c_void_p(c_), C.c_void_p(a_), C.byref(p), C.c_void_p(o_), None)

    assert dev(c, a, o) == 0
    assert dev(c + 4, a, o) == -1 and dev(c, a + 8, o) == -1 and dev(c, a, o + 4) == -1      # alignment
    assert dev(c, a, c) == -1 and dev(c, a, a + 32) == -1                                      # the output overlaps an input
    assert dev(None, a, o) == -1 and dev(c, a, None) == -1
    assert L.rt3_denoise_device(ctx, w, h, C.c_void_p(c), C.c_void_p(a), None, C.c_void_p(o), None) == -1
    assert L.rt3_denoise_device(ctx, 8193, 8192, C.c_void_p(c), C.c_void_p(a), C.byref(good), C.c_void_p(o), None) == -1
    torch.cuda.synchronize()
    with pytest.raises(rt3.Fatal, match="power of two"):
        renderer.denoise(colour, aov, normal_power=100)
    fresh = rt3.initialize_renderer(0)                                 # no scene needed
    try:
        assert fresh.denoise(colour, aov).tobytes() == renderer.denoise(colour, aov).tobytes()
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 6: quality floor
def mse(a, b):
    return float(np.mean((a[..., :3].astype(np.float64) - b[..., :3]) ** 2))


# The weekend spheres are 1-3 pixels wide at 160x120, where the filter has little to average: ratio 1.85 there, 2.37 at 240x180, 2.74 at
# 320x240, 3.92 at 1920x1080 (profiles/denoise_bench_mi355x.log); so the floor is checked at 320x240.
@pytest.mark.parametrize("name,w,h", [("cornell", 160, 120), ("weekend", 320, 240)])
def test_denoised_frame_is_closer_to_a_high_spp_frame(rt3, renderer, name, w, h):
    if name == "cornell":
        set_mesh(rt3, renderer, *rt3.scene_cornell(16))
        cam, lens, flags = rt3.main_camera(w, h), 0.0, rt3.FLAG_BLACK_BACKGROUND
    else:
        set_spheres(rt3, renderer, *rt3.scene_weekend(42))
        cam, lens, flags = rt3.weekend_camera(w, h), 0.05, 0
    frames = {}
    for spp, seed in ((4, 1), (1024, 2)):
        p = rt3.make_params(w, h, spp=spp, max_depth=50, seed=seed, flags=flags, lens_radius=lens)
        renderer.render_path(cam.c, p)
        frames[spp] = (renderer.accum_resolve(p), p)
    raw, p4 = frames[4]
    ref = frames[1024][0]
    den = renderer.denoise(raw, renderer.render_aov(cam.c, p4))
    ratio = mse(raw, ref) / mse(den, ref)
    print("%s: MSE raw %.5g, denoised %.5g, ratio %.2f" % (name, mse(raw, ref), mse(den, ref), ratio))
    assert ratio >= 2.0, ratio


# ------------------------------------------------------------------------------------------------ 7: the command line
def test_cli_writes_the_python_result(rt3, renderer, tmp_path):
    w, h = 64, 48
    args = [EXE, "--scene", "cornell", "--spp", "4", "-W", str(w), "-H", str(h), "--denoise", "D.pfm", "out.png"]
    subprocess.run(args, cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    lin, aov = cornell_frame(rt3, renderer, w, h, 4)
    want = rt3.pfm_bytes(renderer.denoise(lin, aov)[..., :3])
    assert (tmp_path / "D.pfm").read_bytes() == want
    two = tmp_path / "two"
    two.mkdir()
    env = dict(os.environ, RT3_DEVICE_LIST="0,0")
    subprocess.run(args[:1] + ["--gpus", "2"] + args[1:], cwd=str(two), env=env, check=True, capture_output=True, timeout=300)
    assert (two / "D.pfm").read_bytes() == want
