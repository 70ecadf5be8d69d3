"""First-hit AOVs, camera rays and the linear frame (rt3_render_aov*, rt3_camera_rays*, rt3_accum_resolve*) on the GPU.

The AOV albedo of an all-flat scene is tied bit for bit to the depth-1 render (itself pinned to the oracle); every other field is checked
against a numpy composition of camera_rays + intersect; the camera rays are checked against the oracle's own law.  Kernel forms: those of
test_gpu_ray_query.FORMS plus the unfiltered kernel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_denoise_abi import synthetic
from test_gpu_brute import random_soup
from test_gpu_ray_query import FORMS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEDDY = os.path.join(ROOT, "tests", "golden", "teddy.obj")
ALL_FORMS = list(FORMS.items()) + [("brute", None)]
W, H = 40, 30


# ------------------------------------------------------------------------------------------------ helpers
def set_scene(rt3, r, spheres=None, smats=None, faces=None, verts=None, fmats=None):
    if faces is not None and len(faces):
        r.set_mesh(faces, verts, fmats)
    else:
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    if spheres is not None and len(spheres):
        r.set_spheres(spheres, smats)
    else:
        r.set_spheres(np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))


class Form:
    """Context manager: the environment of a kernel form, or the unfiltered kernel (env None)."""

    def __init__(self, r, env, monkeypatch):
        self.r, self.env, self.mp = r, env, monkeypatch

    def __enter__(self):
        if self.env is None:
            self.r.force_brute(True)
        else:
            for k, v in self.env.items():
                self.mp.setenv(k, v)

    def __exit__(self, *exc):
        if self.env is None:
            self.r.force_brute(False)
        else:
            for k in self.env:
                self.mp.delenv(k)


def pack(rgb):
    """pack_pixel of k_resolve (no gamma) on (..., 3) float32."""
    m = np.clip(rgb.astype(np.float32), np.float32(0.0), np.float32(1.0))
    v = np.floor((m * np.float32(255.0)).astype(np.float64) + 0.5).astype(np.uint32) & 0xFF
    return (0xFF | (v[..., 2] << 8) | (v[..., 1] << 16) | (v[..., 0] << 24)).astype(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def flat(mats):
    m = mats.copy()
    m["kind"] = 0
    return m


def scene(rt3, name, flat_mats):
    """(kwargs for set_scene, camera, lens radius) of the test scenes."""
    if name == "weekend":
        sph, sm = rt3.scene_weekend(42)
        return dict(spheres=sph, smats=flat(sm) if flat_mats else sm), rt3.weekend_camera(W, H), 0.1
    if name == "cornell":
        faces, verts, fm = rt3.scene_cornell(16)
        return dict(faces=faces, verts=verts, fmats=flat(fm) if flat_mats else fm), rt3.Camera().update(W, H, 2.0, 2.0, 2.0), 0.05
    if name == "teddy":
        e = rt3.create_object(TEDDY, (0.0, 0.0, -3.0), 1.0 / 17.0, (1.0, 0.0, 0.0))
        faces, verts = rt3.merge_entities([rt3.pre_render_entity(e)])
        return dict(faces=faces, verts=verts), rt3.main_camera(W, H), 0.05
    rng = np.random.default_rng(17)
    faces, verts, fm, cr, sm = random_soup(rng, 300, 200, 1.0, rt3)
    if flat_mats:
        fm, sm = flat(fm), flat(sm)
    return dict(spheres=cr, smats=sm, faces=faces, verts=verts, fmats=fm), rt3.main_camera(W, H), 0.05


def sky(d):
    """sky() of the kernels in float32 (unfused, left to right)."""
    d = d.astype(np.float32)
    ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    t = np.float32(0.5) * (d[..., 1] / ln + np.float32(1.0))
    a = np.float32(1.0) - t
    return np.stack([a * np.float32(1.0) + t * np.float32(c) for c in (0.5, 0.7, 1.0)], axis=-1).astype(np.float32)


def expected_aov(rt3, rays, hits, spp, flags, spheres=None, smats=None, faces=None, fmats=None):
    """The AOVs of DESIGN.md 4.10 composed in numpy from camera_rays + intersect: (aov, pixels where a sphere was hit)."""
    n = len(rays) // spp
    rays, hits = rays.reshape(spp, n), hits.reshape(spp, n)
    alb = np.zeros((n, 3), np.float32)
    nor = np.zeros((n, 3), np.float32)
    dsum = np.zeros(n, np.float32)
    nh = np.zeros(n, np.uint32)
    any_sph = np.zeros(n, bool)
    for s in range(spp):
        k, i, t = hits[s]["kind"], hits[s]["index"], hits[s]["t"]
        d, o = rays[s]["direction"], rays[s]["origin"]
        a = np.zeros((n, 3), np.float32)
        nv = np.zeros((n, 3), np.float32)
        miss = k == 0
        if not (flags & rt3.FLAG_BLACK_BACKGROUND):
            a[miss] = sky(d[miss])
        for kind, mats in ((1, fmats), (2, smats)):
            m = k == kind
            if not m.any():
                continue
            if mats is None:                                          # (faces without materials: flat with the GFace colour)
                rgb, mk = faces["color"][i[m]], np.zeros(int(m.sum()), np.uint32)
            else:
                rgb, mk = mats["rgb"][i[m]], mats["kind"][i[m]]
            a[m] = np.where((mk == 3)[:, None], np.float32(1.0), rgb)
            if kind == 1:
                nv[m] = faces["normal"][i[m]]
            else:
                c = spheres[i[m]]
                p = (t[m, None].astype(np.float64) * d[m] + o[m]).astype(np.float32)
                nv[m] = (p - c[:, :3]) * (np.float32(1.0) / c[:, 3:4])
                any_sph |= m
            dn = (nv[m].astype(np.float64) * d[m]).sum(axis=1)
            nv[m] = np.where((dn < 0.0)[:, None], nv[m], -nv[m])
        hit = (k == 1) | (k == 2)
        alb = (alb + a).astype(np.float32)
        nor = (nor + nv).astype(np.float32)
        dsum = (dsum + np.where(hit, t, np.float32(0.0))).astype(np.float32)
        nh += hit
    out = np.zeros(n, rt3.AOV)
    fs = np.float32(spp)
    out["albedo"] = alb / fs
    out["normal"] = nor / fs
    out["coverage"] = nh.astype(np.float32) / fs
    with np.errstate(invalid="ignore", divide="ignore"):
        out["depth"] = np.where(nh > 0, dsum / nh.astype(np.float32), np.float32(np.inf))
    out["kind"], out["index"] = hits[0]["kind"], hits[0]["index"]
    return out, any_sph


# ------------------------------------------------------------------------------------------------ 1: albedo == the depth-1 render
@pytest.mark.parametrize("name", ["weekend", "cornell", "teddy", "soup"])
def test_albedo_equals_the_depth1_render_on_flat_scenes(rt3, renderer, name, monkeypatch):
    kw, cam, lens = scene(rt3, name, True)
    set_scene(rt3, renderer, **kw)
    for form, env in ALL_FORMS:
        with Form(renderer, env, monkeypatch):
            for spp in (1, 4, 7):
                for lr in (0.0, lens):
                    for flags in (0, rt3.FLAG_BLACK_BACKGROUND):
                        p = rt3.make_params(W, H, spp=spp, max_depth=1, seed=5 + spp, flags=flags, lens_radius=lr)
                        frame = renderer.render_path(cam.c, p)
                        lin = renderer.accum_resolve(p)
                        aov = renderer.render_aov(cam.c, p)
                        what = "%s %s spp %d lens %g flags %d" % (name, form, spp, lr, flags)
                        assert np.array_equal(bits(aov["albedo"]), bits(lin[..., :3])), what
                        assert np.array_equal(pack(aov["albedo"]), frame), what
                        assert (aov["_pad"] == 0).all() and (lin[..., 3] == 0).all()


def test_albedo_equals_the_oracle_depth1_render(rt3, renderer, oracle):
    kw, cam, lens = scene(rt3, "soup", True)
    set_scene(rt3, renderer, **kw)
    p = rt3.make_params(W, H, spp=4, max_depth=1, seed=3, lens_radius=lens)
    aov = renderer.render_aov(cam.c, p)
    op = oracle.make_params(W, H, spp=4, max_depth=1, seed=3, lens_radius=lens)
    ref, _ = oracle.render_path(oracle.copy_camera(cam.c), op, spheres=kw["spheres"], smats=kw["smats"].view(oracle.MATERIAL),
                                faces=kw["faces"], verts=kw["verts"], fmats=kw["fmats"].view(oracle.MATERIAL))
    assert np.array_equal(pack(aov["albedo"]), ref)


# ------------------------------------------------------------------------------------------------ 2: every field == camera_rays + intersect
@pytest.mark.parametrize("name", ["weekend", "soup", "teddy"])
def test_fields_equal_a_composition_of_camera_rays_and_intersect(rt3, renderer, name, monkeypatch):
    kw, cam, lens = scene(rt3, name, False)
    set_scene(rt3, renderer, **kw)
    for form, env in ALL_FORMS:
        with Form(renderer, env, monkeypatch):
            for spp, lr, flags in ((1, 0.0, 0), (4, lens, rt3.FLAG_BLACK_BACKGROUND), (7, lens, rt3.FLAG_GAMMA2)):
                p = rt3.make_params(W, H, spp=spp, max_depth=8, seed=11, flags=flags, lens_radius=lr)
                rays = renderer.camera_rays(cam.c, p)
                assert len(rays) == W * H * spp and (rays["_pad"] == 0).all() and np.isinf(rays["t_max"]).all()
                hits = renderer.intersect(rays, p.t_min)
                got = renderer.render_aov(cam.c, p).reshape(-1)
                want, sph = expected_aov(rt3, rays, hits, spp, flags, kw.get("spheres"), kw.get("smats"), kw.get("faces"), kw.get("fmats"))
                what = "%s %s spp %d" % (name, form, spp)
                for f in ("kind", "index"):
                    assert np.array_equal(got[f], want[f]), what + " " + f
                for f in ("depth", "coverage", "albedo"):
                    assert np.array_equal(bits(got[f]), bits(want[f])), what + " " + f
                assert np.array_equal(bits(got["normal"][~sph]), bits(want["normal"][~sph])), what + " face normals"
                assert np.abs(got["normal"][sph] - want["normal"][sph]).max(initial=0.0) <= 2.0 ** -20, what + " sphere normals"
                assert (got["coverage"] > 0).mean() > 0.2


def test_dielectric_albedo_is_one_not_the_packed_record(rt3, renderer):
    cr = np.array([[0.0, 0.0, -3.0, 1.0]], np.float32)
    m = rt3.dielectric(1.5)
    m["rgb"] = (0.2, 0.3, 0.4)                                        # ignored: a dielectric's attenuation is 1
    set_scene(rt3, renderer, spheres=cr, smats=m)
    cam = rt3.main_camera(W, H)
    aov = renderer.render_aov(cam.c, rt3.make_params(W, H, spp=1))
    hit = aov["kind"] == rt3.HIT_SPHERE
    assert hit.sum() > 20 and (aov["albedo"][hit] == 1.0).all()


# ------------------------------------------------------------------------------------------------ 3: camera rays == the oracle's law
def test_camera_rays_follow_the_oracle(rt3, renderer, oracle):
    kw, cam, lens = scene(rt3, "soup", True)
    set_scene(rt3, renderer, **kw)
    w, h, spp = 24, 16, 4
    cam = rt3.main_camera(w, h)
    p = rt3.make_params(w, h, spp=spp, max_depth=1, seed=23, lens_radius=lens)
    rays = renderer.camera_rays(cam.c, p).reshape(spp, h * w)
    acc = np.zeros((h * w, 3), np.float32)
    for s in range(spp):
        col = np.zeros((h * w, 3), np.float32)
        for i, r in enumerate(rays[s]):
            kind, t, j = oracle.nearest(r["origin"], r["direction"], spheres=kw["spheres"], faces=kw["faces"], verts=kw["verts"], tmin=p.t_min)
            col[i] = oracle.sky(r["direction"]) if kind == 0 else (kw["fmats"] if kind == 1 else kw["smats"])["rgb"][j]
        acc = (acc + col).astype(np.float32)
    got = pack(acc / np.float32(spp)).reshape(h, w)
    op = oracle.make_params(w, h, spp=spp, max_depth=1, seed=23, lens_radius=lens)
    ref, _ = oracle.render_path(oracle.copy_camera(cam.c), op, spheres=kw["spheres"], smats=kw["smats"].view(oracle.MATERIAL),
                                faces=kw["faces"], verts=kw["verts"], fmats=kw["fmats"].view(oracle.MATERIAL))
    assert np.array_equal(got, ref)
    # a sub-range of samples is the matching slice of the whole
    part = renderer.camera_rays(cam.c, p, 1, 2)
    assert part.tobytes() == rays[1:3].reshape(-1).tobytes()


# ------------------------------------------------------------------------------------------------ 4 / 5: tiles and sample batches
def test_tiles_place_rows_like_the_full_frame(rt3, renderer):
    kw, cam, lens = scene(rt3, "soup", False)
    set_scene(rt3, renderer, **kw)
    full = rt3.make_params(W, H, spp=4, max_depth=3, seed=2, lens_radius=lens, tile_rows=4)
    aov = renderer.render_aov(cam.c, full)
    renderer.render_path(cam.c, full)
    lin = renderer.accum_resolve(full)
    for ti in range(3):
        p = rt3.make_params(W, H, spp=4, max_depth=3, seed=2, lens_radius=lens, tile_rows=4, tile_index=ti, tile_count=3)
        rows = [rt3.row_of_local(p, r) for r in range(rt3.rows_owned(p))]
        assert renderer.render_aov(cam.c, p).tobytes() == aov[rows].tobytes()
        renderer.render_path(cam.c, p)
        assert renderer.accum_resolve(p).tobytes() == lin[rows].tobytes()


def test_sample_batches_give_the_same_bytes(rt3, renderer):
    kw, cam, lens = scene(rt3, "soup", False)
    set_scene(rt3, renderer, **kw)
    w, h = 128, 96                                                    # 48 B x 12288 pixels: one sample per MiB batch
    cam = rt3.main_camera(w, h)
    p = rt3.make_params(w, h, spp=7, max_depth=2, seed=4, lens_radius=lens)
    whole = renderer.render_aov(cam.c, p)
    assert renderer.stats().launches == 1
    renderer.set_sample_storage_cap(1 << 20)
    try:
        batched = renderer.render_aov(cam.c, p)
        assert renderer.stats().launches == 7
    finally:
        renderer.set_sample_storage_cap(16 << 30)
    assert batched.tobytes() == whole.tobytes()


# ------------------------------------------------------------------------------------------------ 6 / 7: accumulation, stats, resolve
def test_aov_between_progressive_calls_changes_nothing(rt3, renderer):
    kw, cam, lens = scene(rt3, "soup", False)
    set_scene(rt3, renderer, **kw)
    p = rt3.make_params(W, H, spp=6, max_depth=6, seed=9, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_VARIANCE, lens_radius=lens)
    one = renderer.render_path(cam.c, p)
    acc1, sq1, _ = renderer.accum_download(p, want_sq=True)
    renderer.render_path_range(cam.c, p, 0, 2)
    q = rt3.make_params(W, H, spp=3, max_depth=1, seed=1)
    renderer.render_aov(cam.c, q)
    st = renderer.stats()
    assert st.samples == W * H * 3 and st.ray_casts == W * H * 3 and st.launches == 1 and st.trace_ms > 0.0
    assert st.prim_tests == st.ray_casts * (len(kw["spheres"]) + len(kw["faces"]))
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 4), one)
    acc2, sq2, done = renderer.accum_download(p, want_sq=True)
    assert done == 6 and acc1.tobytes() == acc2.tobytes() and sq1.tobytes() == sq2.tobytes()


@pytest.mark.parametrize("flags", [0, 8])
def test_resolve_is_the_sum_over_samples_done(rt3, renderer, flags):
    kw, cam, lens = scene(rt3, "weekend", False)
    set_scene(rt3, renderer, **kw)
    p = rt3.make_params(W, H, spp=5, max_depth=10, seed=6, flags=flags | rt3.FLAG_GAMMA2, lens_radius=lens)
    for begin, count in ((0, 3), (3, 2)):
        renderer.render_path_range(cam.c, p, begin, count)
        acc, _, done = renderer.accum_download(p)
        want = acc / np.float32(done)
        want[..., 3] = 0.0
        assert done == begin + count
        assert np.array_equal(bits(renderer.accum_resolve(p)), bits(want))
    q = rt3.make_params(W, H, spp=5, max_depth=10, seed=6, flags=flags, lens_radius=lens)    # without gamma: pack(resolve) == frame
    frame = renderer.render_path(cam.c, q)
    assert np.array_equal(pack(renderer.accum_resolve(q)[..., :3]), frame)


# ------------------------------------------------------------------------------------------------ 8 / 9: device forms, argument errors
def test_device_forms_equal_the_host_forms(rt3, renderer):
    import torch
    kw, cam, lens = scene(rt3, "soup", False)
    set_scene(rt3, renderer, **kw)
    p = rt3.make_params(W, H, spp=4, max_depth=4, seed=8, lens_radius=lens)
    aov = renderer.render_aov(cam.c, p)
    rays = renderer.camera_rays(cam.c, p, 1, 3)
    renderer.render_path(cam.c, p)
    lin = renderer.accum_resolve(p)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_aov = torch.zeros(W * H * 12, dtype=torch.float32, device="cuda")
        d_rays = torch.zeros(W * H * 3 * 8, dtype=torch.float32, device="cuda")
        d_lin = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        renderer.render_aov_device(cam.c, p, d_aov.data_ptr(), s.cuda_stream)
        renderer.camera_rays_device(cam.c, p, 1, 3, d_rays.data_ptr(), s.cuda_stream)
        renderer.accum_resolve_device(d_lin.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert d_aov.cpu().numpy().tobytes() == aov.tobytes()
    assert d_rays.cpu().numpy().tobytes() == rays.tobytes()
    assert d_lin.cpu().numpy().tobytes() == lin.tobytes()


def test_host_forms_share_one_staging_buffer(rt3, renderer):
    """The host forms copy through one device buffer of the context: interleaved on one context with different sizes, each call returns
    what it returns on a context of its own."""
    kw, cam, lens = scene(rt3, "soup", False)
    big = rt3.make_params(4 * W, 4 * H, spp=2, max_depth=1, seed=3, lens_radius=lens)
    small = rt3.make_params(W // 2, H // 2, spp=3, max_depth=1, seed=4, lens_radius=lens)
    p = rt3.make_params(W, H, spp=4, max_depth=4, seed=5, lens_radius=lens)
    g = np.linspace(-0.3, 0.3, 3, dtype=np.float32)
    rays = rt3.make_rays(np.zeros((9, 3), np.float32), np.stack([np.repeat(g, 3), np.tile(g, 3), -np.ones(9, np.float32)], axis=-1))
    colour, aov = synthetic(rt3, 12, 16, 5)
    calls = [lambda r: r.render_aov(cam.c, big), lambda r: r.intersect(rays), lambda r: r.denoise(colour, aov),
             lambda r: r.render_aov(cam.c, small), lambda r: r.render_path_range(cam.c, p, 0, 3)]
    set_scene(rt3, renderer, **kw)
    together = [call(renderer) for call in calls]
    for i, call in enumerate(calls):
        alone = rt3.initialize_renderer(0)
        try:
            set_scene(rt3, alone, **kw)
            assert call(alone).tobytes() == together[i].tobytes(), "call %d" % i
        finally:
            alone.close()


def test_argument_errors(rt3, renderer):
    import torch
    L = rt3.lib()
    kw, cam, lens = scene(rt3, "teddy", False)
    set_scene(rt3, renderer, **kw)
    ref = rt3.make_params(W, H, spp=1, flags=rt3.FLAG_REFERENCE_PRIMARY)
    with pytest.raises(rt3.Fatal, match="REFERENCE_PRIMARY"):
        renderer.render_aov(cam.c, ref)
    with pytest.raises(rt3.Fatal, match="REFERENCE_PRIMARY"):
        renderer.camera_rays(cam.c, ref)
    zero = rt3.make_params(W, H, spp=1)
    zero.spp = 0
    out = np.zeros((H, W), rt3.AOV)
    assert L.rt3_render_aov(renderer._ctx, C.byref(cam.c), C.byref(zero), out.ctypes.data_as(C.c_void_p)) == -1
    p = rt3.make_params(W, H, spp=2)
    with pytest.raises(rt3.Fatal, match="sample range"):
        renderer.camera_rays(cam.c, p, 1, 2)
    buf = torch.zeros(W * H * 12 + 16, dtype=torch.float32, device="cuda")
    bad = C.c_void_p(buf.data_ptr() + 4)
    assert L.rt3_render_aov_device(renderer._ctx, C.byref(cam.c), C.byref(p), bad, None) == -1
    assert L.rt3_camera_rays_device(renderer._ctx, C.byref(cam.c), C.byref(p), 0, 1, bad, None) == -1
    renderer.render_path(cam.c, p)
    assert L.rt3_accum_resolve_device(renderer._ctx, bad, None) == -1
    torch.cuda.synchronize()
    fresh = rt3.initialize_renderer(0)
    try:
        assert L.rt3_render_aov(fresh._ctx, C.byref(cam.c), C.byref(p), out.ctypes.data_as(C.c_void_p)) == -4      # no scene
        lin = np.zeros((H, W, 4), np.float32)
        assert L.rt3_accum_resolve(fresh._ctx, lin.ctypes.data_as(C.c_void_p)) == -4                               # nothing rendered
        assert L.rt3_camera_rays(fresh._ctx, C.byref(cam.c), C.byref(p), 0, 1, np.zeros(W * H, rt3.RAY).ctypes.data_as(C.c_void_p)) == 0
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 10: the command line
def test_cli_writes_the_python_results(rt3, renderer, tmp_path):
    exe = os.path.join(ROOT, "raytracer-3_amd", "rt3")
    w, h = 64, 48
    args = [exe, "--scene", "cornell", "--spp", "4", "-W", str(w), "-H", str(h), "--aov", "P", "--hdr", "X.pfm", "out.png"]
    subprocess.run(args, cwd=str(tmp_path), check=True, capture_output=True, timeout=300)
    faces, verts, fm = rt3.scene_cornell(64)
    set_scene(rt3, renderer, faces=faces, verts=verts, fmats=fm)
    cam = rt3.main_camera(w, h)
    p = rt3.make_params(w, h, spp=4, max_depth=50, seed=1, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND)
    renderer.render_path(cam.c, p)
    lin = renderer.accum_resolve(p)
    aov = renderer.render_aov(cam.c, p)
    want = {"X.pfm": rt3.pfm_bytes(lin[..., :3]), "P.albedo.pfm": rt3.pfm_bytes(aov["albedo"]),
            "P.normal.pfm": rt3.pfm_bytes(aov["normal"]), "P.depth.pfm": rt3.pfm_bytes(aov["depth"])}
    for f, b in want.items():
        assert (tmp_path / f).read_bytes() == b, f
    two = tmp_path / "two"
    two.mkdir()
    env = dict(os.environ, RT3_DEVICE_LIST="0,0")
    subprocess.run(args[:1] + ["--gpus", "2"] + args[1:], cwd=str(two), env=env, check=True, capture_output=True, timeout=300)
    for f, b in want.items():
        assert (two / f).read_bytes() == b, "--gpus 2: " + f
