"""The motion plane and the denoiser that reads it (rt3_motion*, rt3_denoise_temporal_motion*) on the GPU: the plane bit for
bit against the numpy restatement (tests/motion_ref.py), unchanged geometry = the camera-only denoiser byte for byte, agreement of the
motion-aware denoiser with the restatement, a history that follows a moving sphere, the host / device / torch forms, the accumulation and
the stats left alone, argument errors, a quality floor against a high-spp frame, and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_ref as M
from test_denoise_abi import synthetic
from test_gpu_denoise import bits, check_close, mse, set_mesh, set_spheres
from test_gpu_temporal import PARAMS, check_history, orbit_camera, perturbed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")
F = np.float32


def slid(cr, k, step=(0.1, 0.02, -0.05)):
    """The spheres of odd index translated by k * step."""
    out = cr.copy()
    out[1::2, :3] += (F(k) * np.array(step, F)).astype(F)
    return out


def tessellated_sphere(rt3, center, radius, n=16):
    return rt3.pre_render_entity(rt3.create_sphere(center, radius, n, n, (0.8, 0.3, 0.2)))


# ------------------------------------------------------------------------------------------------ 1: the plane, bit for bit
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("scene", ["weekend", "cornell", "sphere_entity", "mixed"])
def test_the_plane_equals_the_restatement_bit_for_bit(rt3, renderer, scene, spp):
    w, h = 160, 120
    rng = np.random.default_rng(5)
    spheres = mesh = prev_cr = prev_v = None
    lens, flags = 0.0, 0
    if scene in ("weekend", "mixed"):
        prev_cr, mats = rt3.scene_weekend(42)
        cur_cr = slid(prev_cr, 1)
        cur_cr[5, 3] *= F(1.25)                                          # one of the movers is also rescaled
        cur_cr[8, 3] *= F(0.75)                                          # and one sphere only changes its radius
        spheres = (cur_cr, prev_cr)
        cam = orbit_camera(rt3, w, h, 2.0)
        lens = 0.05 if spp > 1 else 0.0
    if scene == "cornell":
        faces, prev_v, fm = rt3.scene_cornell(16)
        cur_v = prev_v.copy()
        third = len(cur_v) // 3 // 3 * 3                                 # whole faces (3 vertices each): a third of them is displaced
        cur_v[third:2 * third, :3] += rng.normal(0.0, 0.02, (third, 3)).astype(F)
        set_mesh(rt3, renderer, faces, cur_v, fm)
        cam, flags = rt3.main_camera(w, h), rt3.FLAG_BLACK_BACKGROUND
    elif scene in ("sphere_entity", "mixed"):
        at = (6.0, 0.6, 2.0) if scene == "mixed" else (0.0, 0.0, -3.0)
        faces, cur_v = tessellated_sphere(rt3, at, 0.6)
        prev_v = cur_v.copy()
        moved = rng.random(len(cur_v)) < 0.5                             # half of the vertices were somewhere else: a morphing mesh
        prev_v[moved, :3] += rng.normal(0.0, 0.03, (int(moved.sum()), 3)).astype(F)
        if scene == "mixed":
            renderer.set_mesh(faces, cur_v)
            renderer.set_spheres(cur_cr, mats)
        else:
            set_mesh(rt3, renderer, faces, cur_v, None)
            cam = rt3.main_camera(w, h)
    else:
        set_spheres(rt3, renderer, cur_cr, mats)
    if prev_v is not None:
        dl_faces, dl_verts = renderer.mesh_download()
        assert dl_verts.tobytes() == cur_v.tobytes()
        mesh = (dl_faces, cur_v, prev_v)
    p = rt3.make_params(w, h, spp=spp, max_depth=1, seed=3, flags=flags, lens_radius=lens)
    aov = renderer.render_aov(cam.c, p)
    got = renderer.motion(aov, cam.c, prev_center_radius=prev_cr, prev_vertices=prev_v)
    want = M.motion(cam.c, aov, spheres=spheres, mesh=mesh)
    assert got.shape == (h, w, 4) and got.dtype == np.float32
    differ = (bits(got) != bits(want)).any(-1)
    share = float((want[..., 3] != 0).mean())
    print("%s %d spp: %.3f of the pixels moved, largest |m| %.3g, %d pixels differ" % (scene, spp, share, np.abs(want[..., :3]).max(),
                                                                                        int(differ.sum())))
    assert not differ.any(), np.argwhere(differ)[:5]
    assert 0.005 < share < 0.95 and np.isfinite(got).all()
    assert set(np.unique(got[..., 3])) <= {0.0, 1.0}
    hit_classes = set(np.unique(aov["kind"][want[..., 3] != 0]))
    assert hit_classes == ({1, 2} if scene == "mixed" else {2} if scene == "weekend" else {1})


# ------------------------------------------------------------------------------------------------ 2: nothing moved
def old_entry_point(rt3, renderer, colour, aov, cam, prev):
    h, w = aov.shape
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(5, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9)
    out, hist = np.zeros((h, w, 4), F), np.zeros((h, w), rt3.HISTORY)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                          # noqa: E731
    assert rt3.lib().rt3_denoise_temporal(renderer._ctx, w, h, C.byref(cam), ptr(colour), ptr(aov), C.byref(prev[1]), ptr(prev[0]),
                                          C.byref(p), ptr(out), ptr(hist)) == 0
    return out, hist


@pytest.mark.parametrize("scene", ["weekend", "mixed"])
def test_unchanged_geometry_gives_a_zero_plane_and_the_camera_only_output(rt3, renderer, scene):
    w, h = 96, 72
    cr, mats = rt3.scene_weekend(42)
    verts = None
    if scene == "mixed":
        faces, verts = tessellated_sphere(rt3, (6.0, 0.6, 2.0), 0.6)
        renderer.set_mesh(faces, verts)
        renderer.set_spheres(cr, mats)
    else:
        set_spheres(rt3, renderer, cr, mats)
    prev = None
    for k in range(2):
        cam = orbit_camera(rt3, w, h, 1.0 * k)
        p = rt3.make_params(w, h, spp=1, max_depth=8, seed=20 + k)
        renderer.render_path(cam.c, p)
        lin, aov = renderer.accum_resolve(p), renderer.render_aov(cam.c, p)
        plane = renderer.motion(aov, cam.c, prev_center_radius=cr.copy(), prev_vertices=None if verts is None else verts.copy())
        assert not plane.view(np.uint32).any()
        assert not renderer.motion(aov, cam.c).view(np.uint32).any()     # no previous arrays at all
        if k:
            a = renderer.denoise_temporal(lin, aov, cam.c, prev, motion=plane)
            b = renderer.denoise_temporal(lin, aov, cam.c, prev, motion=None)
            c = old_entry_point(rt3, renderer, lin, aov, cam.c, prev)
            assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes()
            assert a[1][0].tobytes() == b[1][0].tobytes() == c[1].tobytes()
            assert (a[1][0]["length"] == 2).mean() > 0.5
        out, prev = renderer.denoise_temporal(lin, aov, cam.c, prev)


# ------------------------------------------------------------------------------------------------ 3: the denoiser against the restatement
def random_plane(h, w, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w, 4), F)
    m[..., :3] = rng.normal(0.0, scale, (h, w, 3))
    m[..., 3] = rng.random((h, w)) < 0.5
    bad = rng.random((h, w)) < 0.02                                       # a non-finite m: that pixel loses its history
    m[bad, 0] = np.where(rng.random(int(bad.sum())) < 0.5, np.inf, np.nan)
    return m


@pytest.mark.parametrize("size", [(2, 2), (31, 17), (96, 64)])
@pytest.mark.parametrize("kw", PARAMS)
def test_agrees_with_the_restatement_on_synthetic_sequences_with_random_planes(rt3, renderer, size, kw):
    w, h = size
    cam = orbit_camera(rt3, w, h, 0.0).c
    gpu_prev = ref_prev = None
    seen_moved_valid = 0
    for k in range(4):
        colour, aov = synthetic(rt3, h, w, 1000 * k + w)
        if k:
            aov["depth"] = ref_prev[0]["depth"] * np.float32(1.0 + 1e-4 * k)     # mostly consistent with the last frame
            aov["normal"] = ref_prev[0]["normal"]
        c = cam if k % 2 else perturbed(rt3, cam, 0.002 * k, k)              # even frames move the camera, odd frames keep it
        plane = random_plane(h, w, 77 * k + h)
        got, gh = renderer.denoise_temporal(colour, aov, c, gpu_prev, motion=plane, **kw)
        want, wh = M.denoise_temporal(colour, aov, c, ref_prev, motion=plane, **kw)
        check_close(got, want)
        check_history(gh[0], wh)
        if k:
            seen_moved_valid += int(((wh["length"] > 1) & (plane[..., 3] != 0) & ~np.isinf(aov["depth"])).sum())
        gpu_prev, ref_prev = gh, (wh, c)
        cam = c
    if w * h >= 64:
        assert seen_moved_valid > 0                                       # some moved pixels found a consistent history


def test_agrees_with_the_restatement_on_a_rendered_moving_sequence(rt3, renderer):
    w, h = 96, 72
    base, mats = rt3.scene_weekend(42)
    gpu_prev = ref_prev = None
    moved_share = 0.0
    for k in range(3):
        cur = slid(base, k, (0.05, 0.0, 0.03))
        set_spheres(rt3, renderer, cur, mats)
        cam = orbit_camera(rt3, w, h, 1.5 * k)
        p = rt3.make_params(w, h, spp=2, max_depth=8, seed=10 + k, lens_radius=0.05)
        renderer.render_path(cam.c, p)
        lin, aov = renderer.accum_resolve(p), renderer.render_aov(cam.c, p)
        plane = renderer.motion(aov, cam.c, prev_center_radius=slid(base, k - 1, (0.05, 0.0, 0.03))) if k else None
        if k:
            assert plane.tobytes() == M.motion(cam.c, aov, spheres=(cur, slid(base, k - 1, (0.05, 0.0, 0.03)))).tobytes()
            moved_share = float((plane[..., 3] != 0).mean())
        got, gh = renderer.denoise_temporal(lin, aov, cam.c, gpu_prev, motion=plane)
        want, wh = M.denoise_temporal(lin, aov, cam.c, ref_prev, motion=plane)
        check_close(got, want)
        check_history(gh[0], wh)
        gpu_prev, ref_prev = gh, (wh, cam.c)
    on_movers = plane[..., 3] != 0
    print("weekend, odd spheres sliding: %.3f of the pixels moved; %.3f of those and %.3f of all have 3 frames of history"
          % (moved_share, float((wh["length"][on_movers] == 3).mean()), float((wh["length"] == 3).mean())))
    assert moved_share > 0.01 and (wh["length"][on_movers] == 3).mean() > 0.5


# ------------------------------------------------------------------------------------------------ 4: the history follows the object
def wire_camera(rt3, origin, horizontal, vertical, lower_left_corner):
    c = rt3.rt3_camera()
    for f, v in (("origin", origin), ("horizontal", horizontal), ("vertical", vertical), ("lower_left_corner", lower_left_corner)):
        for i in range(3):
            getattr(c, f)[i] = v[i]
    return c


def lambert(rt3, rgbs):
    m = np.zeros(len(rgbs), rt3.MATERIAL)
    m["rgb"], m["kind"] = rgbs, rt3.MAT_LAMBERT
    return m


@pytest.mark.parametrize("camera", ["still", "moving"])
def test_the_history_follows_a_sphere_that_moves_by_more_than_its_diameter(rt3, renderer, camera):
    """The analytic scene of tests/test_motion_abi.py, rendered: the caps are conditions (>= 90 % with the plane, <= 10 % without), the
    restatement alone gives 96 to 99 % and 0 %."""
    w, h = 320, 240
    prev_cr = np.array([[-0.8, 0.0, -4.0, 0.5], [0.0, -0.9, -5.0, 0.6], [0.0, -1001.5, -5.0, 1000.0]], F)
    cur_cr = prev_cr.copy()
    cur_cr[0] = (0.8, 0.1, -3.6, 0.55)
    mats = lambert(rt3, [(0.8, 0.2, 0.2), (0.2, 0.3, 0.8), (0.5, 0.5, 0.5)])
    dx = 0.05 if camera == "moving" else 0.0
    cams = [wire_camera(rt3, (0, 0, 0), (4, 0, 0), (0, 3, 0), (-2, -1.5, -1)), wire_camera(rt3, (dx, 0, 0), (4, 0, 0), (0, 3, 0), (dx - 2, -1.5, -1))]
    frames = []
    for k, cr in enumerate((prev_cr, cur_cr)):
        set_spheres(rt3, renderer, cr, mats)
        p = rt3.make_params(w, h, spp=1, max_depth=8, seed=40 + k)
        renderer.render_path(cams[k], p)
        frames.append((renderer.accum_resolve(p), renderer.render_aov(cams[k], p)))
    _, h0 = renderer.denoise_temporal(*frames[0], cams[0], None)
    lin, aov = frames[1]
    plane = renderer.motion(aov, cams[1], prev_center_radius=prev_cr)
    mover = (aov["kind"] == 2) & (aov["index"] == 0)
    assert mover.sum() > 300 and np.array_equal(plane[..., 3] != 0, mover)
    _, (with_m, _) = renderer.denoise_temporal(lin, aov, cams[1], h0, motion=plane)
    _, (without, _) = renderer.denoise_temporal(lin, aov, cams[1], h0)
    share_with, share_without = float((with_m["length"][mover] == 2).mean()), float((without["length"][mover] == 2).mean())
    print("%s camera: %d pixels show the mover; history length 2 with the motion plane %.3f, without %.3f"
          % (camera, int(mover.sum()), share_with, share_without))
    assert share_with >= 0.90 and share_without <= 0.10
    assert np.array_equal(with_m["length"][~mover], without["length"][~mover])


# ------------------------------------------------------------------------------------------------ 5: the forms, the accumulation, errors
def moving_pair(rt3, renderer, w, h):
    """Two frames of the weekend scene with the odd spheres moved in the second: (frames, cameras, current and previous spheres)."""
    base, mats = rt3.scene_weekend(42)
    out = []
    cams = [orbit_camera(rt3, w, h, 0.0).c, orbit_camera(rt3, w, h, 1.0).c]
    for k in range(2):
        set_spheres(rt3, renderer, slid(base, k), mats)
        p = rt3.make_params(w, h, spp=1, max_depth=4, seed=60 + k)
        renderer.render_path(cams[k], p)
        out.append((renderer.accum_resolve(p), renderer.render_aov(cams[k], p)))
    return out, cams, slid(base, 1), base


def test_host_device_and_torch_forms_are_equal(rt3, renderer):
    import torch
    L = rt3.lib()
    w, h = 61, 37
    frames, cams, cur, prev = moving_pair(rt3, renderer, w, h)
    (c0, a0), (c1, a1) = frames
    plane = renderer.motion(a1, cams[1], prev_center_radius=prev)
    assert (plane[..., 3] != 0).any()
    _, h0 = renderer.denoise_temporal(c0, a0, cams[0], None, iterations=3)
    o1, h1 = renderer.denoise_temporal(c1, a1, cams[1], h0, iterations=3, motion=plane)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(h, w, -1)).cuda()    # noqa: E731
    t_prev = torch.from_numpy(prev).cuda()
    t_plane = renderer.motion(t(a1), cams[1], prev_center_radius=t_prev)
    assert t_plane.shape == (h, w, 4) and t_plane.dtype == torch.float32 and t_plane.is_cuda
    assert t_plane.cpu().numpy().tobytes() == plane.tobytes()
    _, th0 = renderer.denoise_temporal(t(c0), t(a0), cams[0], None, iterations=3)
    t1, th1 = renderer.denoise_temporal(t(c1), t(a1), cams[1], th0, iterations=3, motion=t_plane)
    assert t1.cpu().numpy().tobytes() == o1.tobytes() and th1[0].cpu().numpy().tobytes() == h1[0].tobytes()
    s = torch.cuda.Stream()
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(3, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9)
    d_c, d_a, d_h = t(c1), t(a1), t(h0[0])
    v = lambda x: C.c_void_p(x.data_ptr())                                 # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d_m = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        hist = torch.zeros((h, w, 12), dtype=torch.float32, device="cuda")
        assert L.rt3_motion_device(renderer._ctx, w, h, C.byref(cams[1]), v(d_a), v(t_prev), len(prev), None, 0, v(d_m), C.c_void_p(s.cuda_stream)) == 0
        assert L.rt3_denoise_temporal_motion_device(renderer._ctx, w, h, C.byref(cams[1]), v(d_c), v(d_a), C.byref(cams[0]), v(d_h), v(d_m),
                                                    C.byref(p), v(out), v(hist), C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert d_m.cpu().numpy().tobytes() == plane.tobytes()
    assert out.cpu().numpy().tobytes() == o1.tobytes() and hist.cpu().numpy().tobytes() == h1[0].tobytes()
    with pytest.raises(rt3.Fatal, match="motion"):
        renderer.denoise_temporal(t(c1), t(a1), cams[1], th0, motion=t_plane[:, :, :3].contiguous())


def test_progressive_render_continues_across_both_calls(rt3, renderer):
    w, h = 48, 32
    cr, mats = rt3.scene_weekend(42)
    set_spheres(rt3, renderer, cr, mats)
    cam = orbit_camera(rt3, w, h, 0.0)
    p = rt3.make_params(w, h, spp=4, max_depth=8, seed=3, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_VARIANCE)
    one = renderer.render_path(cam.c, p)
    acc1, sq1, _ = renderer.accum_download(p, want_sq=True)
    renderer.render_path_range(cam.c, p, 0, 2)
    st = renderer.stats()
    w2, h2 = w + 9, h + 5
    colour, aov = synthetic(rt3, h2, w2, 4)
    aov["kind"], aov["index"] = 2, np.arange(h2 * w2).reshape(h2, w2) % (len(cr) + 3)      # some indices out of range
    c2 = orbit_camera(rt3, w2, h2, 0.0).c
    plane = renderer.motion(aov, c2, prev_center_radius=slid(cr, 1))
    assert (plane[..., 3] != 0).any()
    assert plane.tobytes() == M.motion(c2, aov, spheres=(cr, slid(cr, 1))).tobytes()
    _, prev = renderer.denoise_temporal(colour, aov, c2, None, motion=plane)
    renderer.denoise_temporal(colour, aov, c2, prev, motion=plane)
    assert bytes(renderer.stats()) == bytes(st)
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 2), one)
    acc2, sq2, done = renderer.accum_download(p, want_sq=True)
    assert done == 4 and acc1.tobytes() == acc2.tobytes() and sq1.tobytes() == sq2.tobytes()


def test_argument_errors(rt3, renderer):
    import torch
    L = rt3.lib()
    ctx = renderer._ctx
    w, h = 8, 4
    n = w * h
    cr, mats = rt3.scene_three_spheres()
    faces, verts = tessellated_sphere(rt3, (0.0, 0.0, -3.0), 0.5, 8)
    renderer.set_mesh(faces, verts)
    renderer.set_spheres(cr, mats)
    colour, aov = synthetic(rt3, h, w, 1)
    cam = orbit_camera(rt3, w, h, 0.0).c
    out = np.zeros((h, w, 4), F)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731

    def host(w_=w, h_=h, c=cam, a=aov, ps=cr, ns=None, pv=verts, nv=None, o=out):
        return L.rt3_motion(ctx, w_, h_, C.byref(c) if c is not None else None, ptr(a), ptr(ps), (0 if ps is None else len(ps)) if ns is None else ns,
                            ptr(pv), (0 if pv is None else len(pv)) if nv is None else nv, ptr(o))

    assert host() == 0 and host(ps=None) == 0 and host(pv=None) == 0 and host(ps=None, pv=None) == 0
    assert host(c=None) == -1 and host(a=None) == -1 and host(o=None) == -1
    assert host(1, h) == -1 and host(w, 1) == -1 and host(8193, 8192) == -1
    assert host(ns=len(cr) - 1) == -1 and host(ns=len(cr) + 1) == -1 and host(nv=len(verts) - 1) == -1 and host(nv=0) == -1
    assert host(ps=None, ns=3) == -1 and host(pv=None, nv=5) == -1        # a NULL array with a count
    bad = rt3.rt3_camera.from_buffer_copy(bytes(cam))
    bad.horizontal[1] = float("nan")
    flat = rt3.rt3_camera.from_buffer_copy(bytes(cam))
    for i in range(3):
        flat.vertical[i] = 2.0 * flat.horizontal[i]
    assert host(c=bad) == -1 and host(c=flat) == -1
    assert host(o=aov.view(np.float32)) == -1                            # the output aliases an input
    big = np.zeros(max(n, len(verts)) * 4, F)
    assert host(o=big, pv=big.reshape(-1, 4)[:len(verts)]) == -1

    # the temporal call checks the plane as an input
    p = rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(5, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9)
    hist, prev, plane = np.zeros((h, w), rt3.HISTORY), np.zeros((h, w), rt3.HISTORY), np.zeros((h, w, 4), F)

    def temporal(m=plane, o=out, oh=hist):
        return L.rt3_denoise_temporal_motion(ctx, w, h, C.byref(cam), ptr(colour), ptr(aov), C.byref(cam), ptr(prev), ptr(m), C.byref(p), ptr(o), ptr(oh))

    assert temporal() == 0 and temporal(m=None) == 0
    assert temporal(o=plane) == -1                                       # the frame overlaps the plane
    assert temporal(m=hist.view(np.float32)) == -1                       # the plane overlaps the history output

    d = torch.zeros(n * 4 * 14 + 64, dtype=torch.float32, device="cuda")
    base = d.data_ptr()
    a_, o_, c_, ph_, oh_, m_, r_ = base, base + n * 48, base + n * 64, base + n * 80, base + n * 128, base + n * 176, base + n * 192
    d_cr, d_v = torch.from_numpy(cr).cuda(), torch.from_numpy(verts).cuda()

    def dev(a=a_, ps=d_cr.data_ptr(), pv=d_v.data_ptr(), o=o_):
        return L.rt3_motion_device(ctx, w, h, C.byref(cam), C.c_void_p(a), C.c_void_p(ps), len(cr) if ps else 0, C.c_void_p(pv),
                                   len(verts) if pv else 0, C.c_void_p(o), None)

    assert dev() == 0 and dev(ps=None, pv=None) == 0
    assert dev(a=a_ + 4) == -1 and dev(o=o_ + 8) == -1 and dev(ps=d_cr.data_ptr() + 4) == -1 and dev(pv=d_v.data_ptr() + 8) == -1
    assert dev(o=a_ + 16) == -1 and dev(o=d_cr.data_ptr()) == -1 and dev(o=0) == -1 and dev(a=0) == -1

    def tdev(m=m_, o=r_, oh=oh_):
        return L.rt3_denoise_temporal_motion_device(ctx, w, h, C.byref(cam), C.c_void_p(c_), C.c_void_p(a_), C.byref(cam), C.c_void_p(ph_),
                                                    C.c_void_p(m) if m else None, C.byref(p), C.c_void_p(o), C.c_void_p(oh), None)

    assert tdev() == 0 and tdev(m=None) == 0
    assert tdev(m=m_ + 4) == -1 and tdev(o=m_) == -1 and tdev(oh=m_ - 16) == -1 and tdev(m=r_ + 16) == -1
    torch.cuda.synchronize()

    # RT3_E_STATE: a previous array for a class the context has no scene of; entity buffers changed after the commit
    renderer.set_spheres(np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))
    assert host(ps=cr) == -4 and host(ps=None) == 0
    renderer.set_spheres(cr, mats)
    assert L.rt3_mesh_begin(ctx, len(faces), len(verts)) == 0             # no commit
    assert host() == -4 and host(pv=None) == 0
    renderer.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    assert host() == -4 and host(pv=None) == 0
    renderer.set_mesh(faces, verts)
    assert host() == 0                                                    # the context is usable after every error above
    with pytest.raises(rt3.Fatal, match="n_prev_spheres"):
        renderer.motion(aov, cam, prev_center_radius=cr[:-1])
    fresh = rt3.initialize_renderer(0)                                    # no scene: a plane of zeros without previous arrays
    try:
        assert not fresh.motion(aov, cam).any()
        with pytest.raises(rt3.Fatal, match="no spheres"):
            fresh.motion(aov, cam, prev_center_radius=cr)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 6: quality floor
# A Lambert ground sphere and five Lambert spheres of distinct albedo under the sky, two of which move 0.1 units per frame; 320x240, 8 frames
# at 1 spp, max_depth 50; the last frame against a 1024-spp frame of its scene and camera.  MSE over the pixels that show a moving sphere
# in the last frame and over the whole frame, for rt3_denoise of the frame alone, rt3_denoise_temporal (camera-only reprojection) and the
# motion-aware call.  Measured on an MI355X (profiles/motion_bench_mi355x.log):
#                                       the 3696 pixels on the movers    the whole frame
#   rt3_denoise of the frame alone      0.0026402                        0.00051675
#   rt3_denoise_temporal (camera only)  0.0023788                        0.00040706
#   rt3_denoise_temporal_motion         0.00059743                       0.00032127
#   camera-only / motion-aware          3.982                            1.267
# The run is deterministic; each floor lies halfway between 1 and the measured ratio (headroom for a change of the filter's constants).  The
# whole-frame ratio measured above 1, so it is asserted too.
MASKED_FLOOR = 2.49
FRAME_FLOOR = 1.13

QUALITY_SPHERES = np.array([[0.0, -1000.5, -4.0, 1000.0], [-1.2, 0.0, -4.0, 0.5], [0.0, 0.0, -4.5, 0.5], [1.2, 0.0, -4.0, 0.5],
                            [-0.6, -0.2, -3.0, 0.3], [0.9, -0.2, -3.0, 0.3]], F)
QUALITY_RGB = [(0.5, 0.5, 0.5), (0.8, 0.2, 0.2), (0.2, 0.7, 0.3), (0.2, 0.3, 0.8), (0.8, 0.7, 0.2), (0.7, 0.3, 0.7)]
QUALITY_STEPS = {4: (0.1, 0.0, 0.0), 5: (-0.04, 0.09, 0.0)}                  # the two small spheres in front move about 0.1 per frame


def quality_spheres(k):
    cr = QUALITY_SPHERES.copy()
    for i, step in QUALITY_STEPS.items():
        cr[i, :3] += (F(k) * np.array(step, F)).astype(F)
    return cr


def quality_mses(rt3, renderer):
    w, h = 320, 240
    mats = lambert(rt3, QUALITY_RGB)
    cam = rt3.main_camera(w, h)
    prev_m = prev_c = None
    for k in range(8):
        set_spheres(rt3, renderer, quality_spheres(k), mats)
        p = rt3.make_params(w, h, spp=1, max_depth=50, seed=200 + k)
        renderer.render_path(cam.c, p)
        lin, aov = renderer.accum_resolve(p), renderer.render_aov(cam.c, p)
        plane = renderer.motion(aov, cam.c, prev_center_radius=quality_spheres(k - 1)) if k else None
        out_m, prev_m = renderer.denoise_temporal(lin, aov, cam.c, prev_m, motion=plane)
        out_c, prev_c = renderer.denoise_temporal(lin, aov, cam.c, prev_c)
    spatial = renderer.denoise(lin, aov)
    pr = rt3.make_params(w, h, spp=1024, max_depth=50, seed=7)
    renderer.render_path(cam.c, pr)
    ref = renderer.accum_resolve(pr)
    mask = (aov["kind"] == 2) & np.isin(aov["index"], list(QUALITY_STEPS))
    assert mask.sum() > 1000 and np.array_equal(mask, plane[..., 3] != 0)
    res = {}
    for name, img in (("spatial", spatial), ("camera_only", out_c), ("motion", out_m)):
        res[name] = (mse(img[mask], ref[mask]), mse(img, ref))
    return res, int(mask.sum())


def test_motion_aware_output_is_closer_to_a_high_spp_frame_on_the_moving_spheres(rt3, renderer):
    res, n = quality_mses(rt3, renderer)
    masked = res["camera_only"][0] / res["motion"][0]
    whole = res["camera_only"][1] / res["motion"][1]
    for name, (m_mask, m_all) in res.items():
        print("two Lambert spheres moving, 320x240 1 spp, frame 8, %-11s: MSE over the %d pixels on the movers %.5g, over the frame %.5g"
              % (name, n, m_mask, m_all))
    print("camera-only / motion-aware: movers %.3f, whole frame %.3f" % (masked, whole))
    assert MASKED_FLOOR >= 1.0 and FRAME_FLOOR >= 1.0
    assert masked >= MASKED_FLOOR, (res, masked)
    assert whole >= FRAME_FLOOR, (res, whole)


# ------------------------------------------------------------------------------------------------ 7: the command line
def test_cli_writes_a_pfm_per_frame_of_a_slide_sequence(tmp_path):
    w, h = 64, 48
    args = [EXE, "--scene", "weekend", "--spp", "1", "-W", str(w), "-H", str(h), "--frames", "3", "--slide", "-0.1,0,0.05", "--denoise", "P",
            "out.png"]
    subprocess.run(args, cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    for k in range(3):
        data = (tmp_path / ("P.%d.pfm" % k)).read_bytes()
        head = b"PF\n%d %d\n-1.0\n" % (w, h)
        assert data.startswith(head), data[:20]
        px = np.frombuffer(data[len(head):], "<f4")
        assert px.size == w * h * 3 and np.isfinite(px).all() and px.any()
    assert (tmp_path / "out.png").exists() and not (tmp_path / "P").exists()
    still = tmp_path / "still"
    still.mkdir()
    subprocess.run(args[:11] + args[13:], cwd=str(still), check=True, capture_output=True, timeout=300)
    assert (still / "P.0.pfm").read_bytes() == (tmp_path / "P.0.pfm").read_bytes()          # frame 0 is the unmoved scene
    assert (still / "P.2.pfm").read_bytes() != (tmp_path / "P.2.pfm").read_bytes()


# ------------------------------------------------------------------------------------------------ host form = device form, optional inputs present and absent
def test_motion_with_each_previous_array_present_and_absent(rt3, renderer):
    from test_gpu_host_forms import F, H, W, dev, host, mixed_scene, records
    cr, faces, verts, cam, p = mixed_scene(rt3, renderer)
    aov = renderer.render_aov(cam.c, p)
    prev_cr, prev_v = cr.copy(), verts.copy()
    prev_cr[:, :3] += F(0.05)
    prev_v[:, :3] -= F(0.03)
    for ps, pv in ((None, None), (prev_cr, None), (None, prev_v), (prev_cr, prev_v)):
        plane = renderer.motion(aov, cam.c, prev_center_radius=ps, prev_vertices=pv)
        t = renderer.motion(records(aov, H, W), cam.c, prev_center_radius=None if ps is None else dev(ps),
                            prev_vertices=None if pv is None else dev(pv))
        assert host(t) == plane.tobytes(), (ps is not None, pv is not None)


def test_temporal_denoise_with_motion_and_history_present_and_absent(rt3, renderer):
    from test_gpu_host_forms import F, H, W, host, mixed_scene, records
    cr, _, _, cam, p = mixed_scene(rt3, renderer)
    colour, aov = synthetic(rt3, H, W, 3)
    plane = np.zeros((H, W, 4), F)
    plane[1:3, 2:6] = (0.2, -0.1, 0.05, 1.0)
    _, h0 = renderer.denoise_temporal(colour, aov, cam.c, None, iterations=2)
    _, t0 = renderer.denoise_temporal(records(colour, H, W), records(aov, H, W), cam.c, None, iterations=2)
    assert host(t0[0]) == h0[0].tobytes()
    outs = []
    for prev, tprev in ((None, None), (h0, t0)):
        for mo in (None, plane):
            out, hist = renderer.denoise_temporal(colour, aov, cam.c, prev, iterations=2, motion=mo)
            t_out, t_hist = renderer.denoise_temporal(records(colour, H, W), records(aov, H, W), cam.c, tprev, iterations=2,
                                                      motion=None if mo is None else records(mo, H, W))
            assert host(t_out) == out.tobytes() and host(t_hist[0]) == hist[0].tobytes(), (prev is not None, mo is not None)
            outs.append(out.tobytes() + hist[0].tobytes())
    assert outs[0] == outs[1]                                           # without a previous frame the plane is checked and not read
