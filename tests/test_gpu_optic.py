"""Lens sequences (rt3_denoise_temporal_optic*, rt3_motion_optic*) on the GPU: agreement with the numpy restatement
(tests/optic_ref.py) on synthetic and rendered sequences of all four lens models — the column wrap of an equirectangular frame and the face
edges of a cube frame among them —, no history = rt3_denoise bit for bit, a still lens, the motion plane bit for bit, the host / device /
torch forms, the accumulation and the stats left alone, argument errors, and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import optic_ref as O
from test_denoise_abi import synthetic
from test_gpu_denoise import bits, check_close, set_mesh, set_spheres
from test_gpu_motion import slid, tessellated_sphere
from test_gpu_temporal import check_history

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")
F = np.float32
MODELS = ("equirect", "fisheye", "ortho", "cube")
SIZES = {"equirect": ((2, 2), (31, 17), (96, 48)), "fisheye": ((2, 2), (31, 17), (96, 48)), "ortho": ((2, 2), (31, 17), (96, 48)),
         "cube": ((2, 12), (5, 30), (16, 96))}
CASES = [(m, s) for m in MODELS for s in SIZES[m]]
ORIGIN, AT, VUP = (0.3, 1.1, 2.0), (-0.2, 0.4, -1.0), (0.1, 1.0, 0.05)


def a_lens(rt3, model, origin=ORIGIN, at=AT, vup=VUP):
    return rt3.make_lens(model, origin, at, vup, fov_deg=200.0, extent=(3.0, 1.75))


def perturbed(rt3, model, scale, seed):
    """a_lens moved and turned a little (synthetic sequences)."""
    rng = np.random.default_rng(seed)
    return a_lens(rt3, model, np.array(ORIGIN) + scale * rng.normal(size=3), np.array(AT) + scale * rng.normal(size=3),
                  np.array(VUP) + scale * rng.normal(size=3))


def orbit_lens(rt3, model, deg, at=(0.0, 0.0, 0.0), look_from=(13.0, 2.0, 3.0)):
    a = np.radians(deg)
    dx, dz = look_from[0] - at[0], look_from[2] - at[2]
    f = (at[0] + (np.cos(a) * dx + np.sin(a) * dz), look_from[1], at[2] + (np.cos(a) * dz - np.sin(a) * dx))
    return rt3.make_lens(model, f, at, fov_deg=120.0, extent=(8.0, 8.0))


def sequence(rt3, renderer, w, h, lenses, kw=None, seed=0, check=True):
    """Synthetic frames through both implementations: frame k is mostly consistent with frame k - 1.  Returns the last (gpu history, reference
    history, reference previous) triple."""
    kw = kw or {}
    gpu_prev = ref_prev = None
    for k, lens in enumerate(lenses):
        colour, aov = synthetic(rt3, h, w, 1000 * k + w + seed)
        if k:
            aov["depth"] = ref_prev[0]["depth"] * np.float32(1.0 + 1e-4 * k)
            aov["normal"] = ref_prev[0]["normal"]
        got, gh = renderer.denoise_temporal_lens(colour, aov, lens, gpu_prev, **kw)
        want, wh = O.denoise_temporal_lens(colour, aov, lens, ref_prev, **kw)
        if check:
            check_close(got, want)
            check_history(gh[0], wh)
        last_prev = ref_prev
        gpu_prev, ref_prev = gh, (wh, lens)
    return gh, wh, last_prev, aov


# ------------------------------------------------------------------------------------------------ 1: agreement with the restatement
KW = dict(normal_tolerance=0.5, depth_tolerance=4.0)          # (the synthetic normals are 0.7 n + 0.3 z: not unit vectors)


@pytest.mark.parametrize("model,size", CASES)
def test_agrees_with_the_restatement_on_synthetic_sequences(rt3, renderer, model, size):
    w, h = size
    lenses, lens = [], a_lens(rt3, model)
    for k in range(4):                                                  # even frames move the lens, odd frames keep it (the shortcut)
        lens = lens if k % 2 else perturbed(rt3, model, 0.002 * (k + 1), k)
        lenses.append(lens)
    gh, wh, _, _ = sequence(rt3, renderer, w, h, lenses, KW)
    if w * h >= 64:
        assert (wh["length"] > 1).any()


@pytest.mark.parametrize("kw", [dict(iterations=1, alpha=0.5, moments_alpha=0.1, normal_tolerance=-1.0),
                                dict(iterations=3, normal_power=16, sigma_luminance=2.0, depth_tolerance=8.0, normal_tolerance=0.5)])
def test_other_parameters(rt3, renderer, kw):
    lenses = [perturbed(rt3, "fisheye", 0.003, k) for k in range(3)]
    sequence(rt3, renderer, 31, 17, lenses, kw)


def test_a_yawed_equirect_lens_wraps_its_columns(rt3, renderer):
    """The previous lens is the current one turned about `up` by 0.4 and then -0.4 of a column: x' leaves [0, W - 1] on both sides, and the taps
    of those pixels come from the other edge of the frame."""
    w, h = 32, 16
    lenses = []
    for k, cols in enumerate((0.0, 0.4, 0.0)):
        a = 2.0 * np.pi * cols / w
        lenses.append(rt3.make_lens("equirect", (0.5, 0.25, -1.0), (0.5 + np.sin(a), 0.25, -1.0 - np.cos(a))))
    kw = dict(normal_tolerance=-1.0, depth_tolerance=1e3)
    gh, wh, prev, aov = sequence(rt3, renderer, w, h, lenses, kw)
    seen = set()
    for cur, before in ((lenses[1], lenses[0]), (lenses[2], lenses[1])):
        view, ok, xp, yp = O.reproject(cur, before, w, h, aov["depth"].astype(F))
        seen.add("low" if (ok & (xp < 0)).any() else "")
        seen.add("high" if (ok & (xp > w - 1)).any() else "")
    assert {"low", "high"} <= seen
    view, ok, xp, yp = O.reproject(lenses[2], lenses[1], w, h, aov["depth"].astype(F))
    edge = ok & ((xp < 0) | (xp > w - 1))
    assert edge.any() and (wh["length"][edge] > 1).any()                  # a wrapped tap carried history across the seam


def test_a_cube_frame_keeps_its_taps_on_the_face(rt3, renderer):
    n = 8
    w, h = n, 6 * n
    lenses = [a_lens(rt3, "cube"), perturbed(rt3, "cube", 0.004, 7)]
    kw = dict(normal_tolerance=-1.0, depth_tolerance=1e3)
    gh, wh, prev, aov = sequence(rt3, renderer, w, h, lenses, kw)
    view, ok, xp, yp = O.reproject(lenses[1], lenses[0], w, h, aov["depth"].astype(F))
    iy, fy = np.floor(yp), yp - np.floor(yp)
    with np.errstate(invalid="ignore"):
        inside = ok & (xp > -1) & (xp < w) & (yp > -1) & (yp < h)
        cut = inside & (fy != 0) & ((iy < view.face * n) | (iy + 1 >= (view.face + 1) * n))       # a tap on the neighbouring face is skipped
        inner = inside & (iy >= view.face * n) & (iy + 1 < (view.face + 1) * n)
    assert cut.any() and inner.any()
    assert (wh["length"][inner] == 2).any()
    moved_face = inside & (view.face != (np.arange(h)[:, None] // n))
    print("cube N = %d: %d pixels with a tap cut at a face edge, %d pixels reprojected onto another face" % (n, cut.sum(), moved_face.sum()))


# ------------------------------------------------------------------------------------------------ 2: no history, a still lens
@pytest.mark.parametrize("model", MODELS)
def test_no_history_is_rt3_denoise_bit_for_bit(rt3, renderer, model):
    w, h = (12, 72) if model == "cube" else (70, 45)
    colour, aov = synthetic(rt3, h, w, 9)
    lens = a_lens(rt3, model)
    for kw in ({}, dict(iterations=2, normal_power=4)):
        out, (hist, _) = renderer.denoise_temporal_lens(colour, aov, lens, None, **kw)
        assert np.array_equal(bits(out), bits(renderer.denoise(colour, aov, **kw)))
        assert (hist["length"] == 1).all()
        bad = hist.copy()
        bad["depth"] = np.where(np.isinf(bad["depth"]), np.float32(1.0), bad["depth"] + np.float32(1000.0))   # every tap inconsistent
        bad["colour"] = 1e6
        for prev_lens in (lens, perturbed(rt3, model, 0.002, 3)):
            out2, (hist2, _) = renderer.denoise_temporal_lens(colour, aov, lens, (bad, prev_lens), **kw)
            assert np.array_equal(bits(out2), bits(out)) and (hist2["length"] == 1).all()


@pytest.mark.parametrize("model", MODELS)
def test_a_still_lens_counts_up_and_averages(rt3, renderer, model):
    w, h = (6, 36) if model == "cube" else (40, 30)
    lens = a_lens(rt3, model)
    values = [1.0, 2.0, 3.0, 6.0, 0.5]
    prev = None
    for k, val in enumerate(values):
        colour = np.zeros((h, w, 4), np.float32)
        colour[..., :3] = val
        aov = np.zeros((h, w), rt3.AOV)
        aov["albedo"], aov["normal"], aov["depth"], aov["coverage"] = (1.0, 1.0, 1.0), (0.0, 0.0, 1.0), 7.0, 1.0
        out, prev = renderer.denoise_temporal_lens(colour, aov, lens, prev)
        assert (prev[0]["length"] == k + 1).all()
        assert np.allclose(out[..., :3], np.mean(values[: k + 1]), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ 3: the motion plane
FRAME = {"equirect": (96, 48), "fisheye": (64, 64), "ortho": (64, 48), "cube": (16, 96)}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("scene", ["weekend", "sphere_entity"])
def test_the_plane_equals_the_restatement_bit_for_bit(rt3, renderer, scene, model):
    w, h = FRAME[model]
    rng = np.random.default_rng(5)
    spheres = mesh = prev_cr = prev_v = None
    if scene == "weekend":
        prev_cr, mats = rt3.scene_weekend(42)
        cur_cr = slid(prev_cr, 1)                                        # half of the spheres moved
        cur_cr[5, 3] *= F(1.25)
        spheres = (cur_cr, prev_cr)
        set_spheres(rt3, renderer, cur_cr, mats)
        lens = orbit_lens(rt3, model, 2.0)
    else:
        faces, cur_v = tessellated_sphere(rt3, (0.0, 0.0, -3.0), 0.6)
        prev_v = cur_v.copy()
        moved = rng.random(len(cur_v)) < 0.5
        prev_v[moved, :3] += rng.normal(0.0, 0.03, (int(moved.sum()), 3)).astype(F)
        set_mesh(rt3, renderer, faces, cur_v, None)
        dl_faces, dl_verts = renderer.mesh_download()
        assert dl_verts.tobytes() == cur_v.tobytes()
        mesh = (dl_faces, cur_v, prev_v)
        lens = rt3.make_lens(model, (0.1, 0.05, 0.0), (0.0, 0.0, -3.0), fov_deg=90.0, extent=(2.0, 2.0))
    p = rt3.make_params(w, h, spp=1, max_depth=1, seed=3)
    aov = renderer.render_lens_aov(lens, p)
    got = renderer.motion_lens(aov, lens, prev_center_radius=prev_cr, prev_vertices=prev_v)
    want = O.motion_lens(lens, aov, spheres=spheres, mesh=mesh)
    assert got.shape == (h, w, 4) and got.dtype == np.float32
    differ = (bits(got) != bits(want)).any(-1)
    share = float((want[..., 3] != 0).mean())
    print("%s %s: %.4f of the pixels moved, %d pixels differ" % (scene, model, share, int(differ.sum())))
    assert not differ.any(), np.argwhere(differ)[:5]
    assert share > 0 and np.isfinite(got).all() and set(np.unique(got[..., 3])) <= {0.0, 1.0}


@pytest.mark.parametrize("model", ("equirect", "fisheye"))
def test_unchanged_geometry_gives_a_zero_plane_and_the_same_output(rt3, renderer, model):
    w, h = FRAME[model]
    cr, mats = rt3.scene_weekend(42)
    set_spheres(rt3, renderer, cr, mats)
    prev = None
    for k in range(2):
        lens = orbit_lens(rt3, model, 1.0 * k)
        p = rt3.make_params(w, h, spp=1, max_depth=8, seed=20 + k)
        lin, aov = renderer.render_lens(lens, p), renderer.render_lens_aov(lens, p)
        plane = renderer.motion_lens(aov, lens, prev_center_radius=cr.copy())
        assert not plane.view(np.uint32).any()
        assert not renderer.motion_lens(aov, lens).view(np.uint32).any()      # no previous arrays at all
        if k:
            a = renderer.denoise_temporal_lens(lin, aov, lens, prev, motion=plane)
            b = renderer.denoise_temporal_lens(lin, aov, lens, prev, motion=None)
            assert a[0].tobytes() == b[0].tobytes() and a[1][0].tobytes() == b[1][0].tobytes()
            assert (a[1][0]["length"] == 2).any()
        out, prev = renderer.denoise_temporal_lens(lin, aov, lens, prev)


@pytest.mark.parametrize("model", MODELS)
def test_the_denoiser_follows_the_plane_as_the_restatement_does(rt3, renderer, model):
    """A random plane (half of the pixels moved, by about a pixel) with an equal lens (moved pixels are projected, the others keep their place) and
    with a moved one."""
    w, h = (8, 48) if model == "cube" else (48, 30)
    rng = np.random.default_rng(11)
    lens0 = a_lens(rt3, model)
    for lens1 in (lens0, perturbed(rt3, model, 0.002, 1)):
        c0, a0 = synthetic(rt3, h, w, 41)
        c1, a1 = synthetic(rt3, h, w, 42)
        a1["depth"], a1["normal"] = a0["depth"], a0["normal"]
        plane = np.zeros((h, w, 4), F)
        plane[..., :3] = rng.normal(0.0, 0.05, (h, w, 3))
        plane[..., 3] = rng.random((h, w)) < 0.5
        g0, gh0 = renderer.denoise_temporal_lens(c0, a0, lens0, None, **KW)
        w0, wh0 = O.denoise_temporal_lens(c0, a0, lens0, None, **KW)
        got, gh = renderer.denoise_temporal_lens(c1, a1, lens1, gh0, motion=plane, **KW)
        want, wh = O.denoise_temporal_lens(c1, a1, lens1, (wh0, lens0), motion=plane, **KW)
        check_close(got, want)
        check_history(gh[0], wh)
        assert (wh["length"][plane[..., 3] != 0] == 2).any() and (wh["length"][plane[..., 3] == 0] == 2).any()


# ------------------------------------------------------------------------------------------------ 4: rendered sequences
@pytest.mark.parametrize("model,size", [("equirect", (64, 32)), ("fisheye", (48, 48))])
def test_agrees_with_the_restatement_on_rendered_sequences(rt3, renderer, model, size):
    w, h = size
    set_spheres(rt3, renderer, *rt3.scene_weekend(42))
    gpu_prev = ref_prev = None
    for k in range(3):
        lens = orbit_lens(rt3, model, 1.5 * k)
        p = rt3.make_params(w, h, spp=2, max_depth=8, seed=10 + k)
        lin, aov = renderer.render_lens(lens, p), renderer.render_lens_aov(lens, p)
        got, gh = renderer.denoise_temporal_lens(lin, aov, lens, gpu_prev)
        want, wh = O.denoise_temporal_lens(lin, aov, lens, ref_prev)
        check_close(got, want)
        check_history(gh[0], wh)
        gpu_prev, ref_prev = gh, (wh, lens)
    share, ref_share = float((gh[0]["length"] == 3).mean()), float((wh["length"] == 3).mean())
    print("%s %dx%d: %.3f of the pixels have 3 frames of history (the restatement: %.3f)" % (model, w, h, share, ref_share))
    assert share >= ref_share and share > 0


# ------------------------------------------------------------------------------------------------ 5: the forms
def test_host_device_and_torch_forms_are_equal(rt3, renderer):
    import torch
    L = rt3.lib()
    w, h = 61, 37
    lens0 = a_lens(rt3, "equirect")
    lens1 = perturbed(rt3, "equirect", 0.001, 5)
    c0, a0 = synthetic(rt3, h, w, 21)
    c1, a1 = synthetic(rt3, h, w, 22)
    a1["depth"], a1["normal"] = a0["depth"], a0["normal"]
    plane = np.zeros((h, w, 4), F)
    plane[::3, :, :3], plane[::3, :, 3] = 0.01, 1.0
    o0, h0 = renderer.denoise_temporal_lens(c0, a0, lens0, None, iterations=3, **KW)
    o1, h1 = renderer.denoise_temporal_lens(c1, a1, lens1, h0, motion=plane, iterations=3, **KW)
    assert (h1[0]["length"] == 2).any()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(h, w, -1)).cuda()    # noqa: E731
    t0, th0 = renderer.denoise_temporal_lens(t(c0), t(a0), lens0, None, iterations=3, **KW)
    t1, th1 = renderer.denoise_temporal_lens(t(c1), t(a1), lens1, th0, motion=t(plane), iterations=3, **KW)
    assert t1.shape == (h, w, 4) and t1.dtype == torch.float32 and t1.is_cuda
    assert t0.cpu().numpy().tobytes() == o0.tobytes() and t1.cpu().numpy().tobytes() == o1.tobytes()
    assert th1[0].cpu().numpy().tobytes() == h1[0].tobytes()
    s = torch.cuda.Stream()
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(3, 128, 4.0, 1.0), 0.2, 0.2, KW["depth_tolerance"], KW["normal_tolerance"])
    d_c, d_a, d_h, d_m = t(c1), t(a1), t(h0[0]), t(plane)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        hist = torch.zeros((h, w, 12), dtype=torch.float32, device="cuda")
        assert L.rt3_denoise_temporal_optic_device(renderer._ctx, w, h, C.byref(lens1), C.c_void_p(d_c.data_ptr()), C.c_void_p(d_a.data_ptr()),
                                                   C.byref(lens0), C.c_void_p(d_h.data_ptr()), C.c_void_p(d_m.data_ptr()), C.byref(p),
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(hist.data_ptr()), C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert out.cpu().numpy().tobytes() == o1.tobytes() and hist.cpu().numpy().tobytes() == h1[0].tobytes()
    with pytest.raises(rt3.Fatal, match="48-byte"):
        renderer.denoise_temporal_lens(t(c1), t(a1), lens1, (th0[0][:, :, :4].contiguous(), lens0))
    # the motion plane: numpy, torch and the device entry point on a stream
    cr, mats = rt3.scene_weekend(42)
    set_spheres(rt3, renderer, slid(cr, 1), mats)
    lens = orbit_lens(rt3, "fisheye", 0.0)
    pp = rt3.make_params(w, h, spp=1, max_depth=1, seed=3)
    aov = renderer.render_lens_aov(lens, pp)
    m0 = renderer.motion_lens(aov, lens, prev_center_radius=cr)
    assert m0[..., 3].any()
    m1 = renderer.motion_lens(t(aov), lens, prev_center_radius=torch.from_numpy(cr).cuda())
    assert m1.is_cuda and m1.cpu().numpy().tobytes() == m0.tobytes()
    d_aov, d_cr = t(aov), torch.from_numpy(cr).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        m2 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        assert L.rt3_motion_optic_device(renderer._ctx, w, h, C.byref(lens), C.c_void_p(d_aov.data_ptr()), C.c_void_p(d_cr.data_ptr()), len(cr), None, 0,
                                         C.c_void_p(m2.data_ptr()), C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert m2.cpu().numpy().tobytes() == m0.tobytes()


# ------------------------------------------------------------------------------------------------ 6: accumulation and stats untouched
def test_progressive_render_continues_across_both_calls(rt3, renderer):
    w, h = 48, 32
    cr, mats = rt3.scene_weekend(42)
    set_spheres(rt3, renderer, cr, mats)
    cam = rt3.weekend_camera(w, h)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=3, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_VARIANCE)
    one = renderer.render_path(cam.c, p)
    acc1, sq1, _ = renderer.accum_download(p, want_sq=True)
    renderer.render_path_range(cam.c, p, 0, 2)
    st = renderer.stats()
    colour, aov = synthetic(rt3, h + 5, w + 9, 4)
    lens = a_lens(rt3, "fisheye")
    _, prev = renderer.denoise_temporal_lens(colour, aov, lens, None)
    renderer.denoise_temporal_lens(colour, aov, lens, prev)
    renderer.motion_lens(aov, lens, prev_center_radius=slid(cr, 1))
    assert bytes(renderer.stats()) == bytes(st)
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 2), one)
    acc2, sq2, done = renderer.accum_download(p, want_sq=True)
    assert done == 4 and acc1.tobytes() == acc2.tobytes() and sq1.tobytes() == sq2.tobytes()


# ------------------------------------------------------------------------------------------------ 7: argument errors
def test_argument_errors(rt3, renderer):
    import torch
    L = rt3.lib()
    ctx = renderer._ctx
    w, h = 8, 4
    colour, aov = synthetic(rt3, h, w, 1)
    lens = a_lens(rt3, "equirect")
    out = np.zeros((h, w, 4), np.float32)
    hist = np.zeros((h, w), rt3.HISTORY)
    prev = np.zeros((h, w), rt3.HISTORY)
    plane = np.zeros((h, w, 4), np.float32)

    def P(*spatial, alpha=0.2, moments_alpha=0.2, dtol=2.0, ntol=0.9):
        return rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(*(spatial or (5, 128, 4.0, 1.0))), alpha, moments_alpha, dtol, ntol)

    good = P()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
    ref = lambda s: C.byref(s) if s is not None else None                         # noqa: E731

    def host(w_=w, h_=h, p=good, l=lens, pl=None, ph=None, m=None, o=out, oh=hist, col=colour, a=aov):
        return L.rt3_denoise_temporal_optic(ctx, w_, h_, ref(l), ptr(col), ptr(a), ref(pl), ptr(ph), ptr(m), ref(p), ptr(o), ptr(oh))

    assert host() == 0 and host(pl=lens, ph=prev) == 0 and host(pl=lens, ph=prev, m=plane) == 0 and host(m=plane) == 0
    assert host(p=None) == -1 and host(l=None) == -1 and host(col=None) == -1 and host(a=None) == -1
    assert host(o=None) == -1 and host(oh=None) == -1
    assert host(pl=lens) == -1 and host(ph=prev) == -1                   # prev_lens and prev_history: both or neither
    assert host(1, h) == -1 and host(w, 1) == -1 and host(8193, 8192) == -1
    for bad in (P(0, 128, 4.0, 1.0), P(5, 96, 4.0, 1.0), P(5, 128, 0.0, 1.0), P(alpha=0.0), P(alpha=1.5), P(moments_alpha=0.0),
                P(dtol=0.0), P(dtol=float("inf")), P(ntol=1.01), P(ntol=float("nan"))):
        assert host(p=bad) == -1
    # a lens rt3lens::refusal refuses for this W x H, as this frame's or as the previous one
    def broken(change):
        b = rt3.rt3_lens.from_buffer_copy(bytes(lens))
        change(b)
        return b
    refused = [broken(lambda b: setattr(b, "model", 0)), broken(lambda b: setattr(b, "model", 5)),
               broken(lambda b: b.origin.__setitem__(0, float("inf"))), broken(lambda b: b.up.__setitem__(1, float("nan"))),
               broken(lambda b: b.right.__setitem__(0, b.right[0] * 1.01)), broken(lambda b: [b.up.__setitem__(i, b.right[i]) for i in range(3)])]
    for b in refused:
        assert host(l=b) == -1 and host(pl=b, ph=prev) == -1
    fish = a_lens(rt3, "fisheye")
    assert host(l=fish) == 0 and host(l=fish, pl=fish, ph=prev) == 0
    assert host(l=fish, pl=lens, ph=prev) == -1 and host(l=lens, pl=fish, ph=prev) == -1        # the models differ
    assert b"model" in L.rt3_last_error(ctx)
    fish.half_fov_turns = 0.6
    assert host(l=fish) == -1
    ortho = a_lens(rt3, "ortho")
    assert host(l=ortho) == 0
    ortho.half_extent[1] = 0.0
    assert host(l=ortho) == -1
    cube = a_lens(rt3, "cube")
    assert host(l=cube) == -1                                            # 8 x 4 is not a cube frame
    c6, a6 = synthetic(rt3, 12, 2, 2)
    o6, h6 = np.zeros((12, 2, 4), np.float32), np.zeros((12, 2), rt3.HISTORY)
    assert host(2, 12, l=cube, col=c6, a=a6, o=o6, oh=h6) == 0 and host(2, 10, l=cube, col=c6, a=a6, o=o6, oh=h6) == -1
    assert host(o=colour) == -1 and host(oh=prev, pl=lens, ph=prev) == -1 and host(o=plane, m=plane) == -1     # an output aliases an input
    shared = np.zeros((h, w), rt3.HISTORY)
    assert host(o=shared.view(np.float32), oh=shared) == -1              # the two outputs share a buffer

    n = w * h
    d = torch.zeros(n * 4 * 20 + 64, dtype=torch.float32, device="cuda")
    base = d.data_ptr()
    c_, a_, ph_, o_, oh_, m_ = base, base + n * 16, base + n * 64, base + n * 112, base + n * 128, base + n * 176

    def dev(c=c_, a=a_, ph=ph_, o=o_, oh=oh_, pl=lens, m=m_):
        return L.rt3_denoise_temporal_optic_device(ctx, w, h, C.byref(lens), C.c_void_p(c), C.c_void_p(a), ref(pl),
                                                   C.c_void_p(ph) if ph is not None else None, C.c_void_p(m) if m is not None else None,
                                                   C.byref(good), C.c_void_p(o), C.c_void_p(oh), None)

    assert dev() == 0 and dev(pl=None, ph=None) == 0 and dev(m=None) == 0
    assert dev(c=c_ + 4) == -1 and dev(a=a_ + 8) == -1 and dev(ph=ph_ + 4) == -1 and dev(o=o_ + 4) == -1 and dev(oh=oh_ + 4) == -1 and dev(m=m_ + 4) == -1
    assert dev(o=c_) == -1 and dev(o=a_ + 32) == -1 and dev(o=ph_ + 16) == -1 and dev(o=m_ + 16) == -1      # the frame overlaps an input
    assert dev(oh=a_) == -1 and dev(oh=ph_) == -1 and dev(oh=c_ + 16) == -1                                 # the history overlaps an input
    assert dev(oh=o_ + 16) == -1 and dev(oh=o_ - 16) == -1                                                  # the outputs overlap each other
    assert dev(c=0) == -1 and dev(o=0) == -1 and dev(oh=0) == -1
    torch.cuda.synchronize()

    # rt3_motion_optic*: the frame, the lens, the previous arrays against the scene on the context
    cr, mats = rt3.scene_weekend(42)
    set_spheres(rt3, renderer, cr, mats)
    mo = np.zeros((h, w, 4), np.float32)

    def motion(w_=w, h_=h, l=lens, a=aov, ps=cr, ns=len(cr), pv=None, nv=0, o=mo):
        return L.rt3_motion_optic(ctx, w_, h_, ref(l), ptr(a), ptr(ps), ns, ptr(pv), nv, ptr(o))

    assert motion() == 0 and motion(ps=None, ns=0) == 0
    assert motion(l=None) == -1 and motion(a=None) == -1 and motion(o=None) == -1
    assert motion(1, h) == -1 and motion(w, 1) == -1 and motion(8193, 8192) == -1
    assert motion(l=refused[0]) == -1 and motion(l=refused[4]) == -1 and motion(l=cube) == -1
    assert motion(ps=None, ns=3) == -1 and motion(ns=len(cr) - 1) == -1
    assert motion(pv=np.zeros((3, 4), np.float32), nv=3) == -4            # RT3_E_STATE: no committed mesh on the context
    assert motion(o=aov.view(np.float32)) == -1                         # the output aliases an input
    dm = torch.zeros(n * 4 * 8 + 64, dtype=torch.float32, device="cuda")
    mb = dm.data_ptr()
    d_cr = torch.from_numpy(cr).cuda()

    def mdev(a=mb, o=mb + n * 48, ps=d_cr.data_ptr()):
        return L.rt3_motion_optic_device(ctx, w, h, C.byref(lens), C.c_void_p(a), C.c_void_p(ps), len(cr), None, 0, C.c_void_p(o), None)

    assert mdev() == 0
    assert mdev(a=mb + 4) == -1 and mdev(o=mb + n * 48 + 8) == -1 and mdev(ps=d_cr.data_ptr() + 4) == -1 and mdev(o=mb + 16) == -1
    torch.cuda.synchronize()
    with pytest.raises(rt3.Fatal, match="normal_tolerance"):
        renderer.denoise_temporal_lens(colour, aov, lens, None, normal_tolerance=2.0)
    with pytest.raises(rt3.Fatal, match="model"):
        renderer.denoise_temporal_lens(colour, aov, lens, (prev, a_lens(rt3, "ortho")))
    fresh = rt3.initialize_renderer(0)                                 # no scene needed for the denoiser
    try:
        assert fresh.denoise_temporal_lens(colour, aov, lens)[0].tobytes() == renderer.denoise_temporal_lens(colour, aov, lens)[0].tobytes()
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 8: the command line
def test_cli_writes_a_pfm_per_lens_frame(tmp_path):
    w, h = 64, 32
    args = [EXE, "--scene", "weekend", "--spp", "1", "-W", str(w), "-H", str(h), "--lens", "equirect", "--lens-frames", "3", "--orbit", "1",
            "--slide", "0.05,0,0", "--denoise", "P", "out.png"]
    subprocess.run(args, cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    frames = []
    for k in range(3):
        data = (tmp_path / ("P.%d.pfm" % k)).read_bytes()
        head = b"PF\n%d %d\n-1.0\n" % (w, h)
        assert data.startswith(head), data[:20]
        px = np.frombuffer(data[len(head):], "<f4")
        assert px.size == w * h * 3 and np.isfinite(px).all() and px.any()
        frames.append(px)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    assert (tmp_path / "out.png").exists() and not (tmp_path / "P").exists()
