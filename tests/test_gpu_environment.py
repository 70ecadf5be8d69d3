"""Environment-map lighting (rt3_set_environment*) on the GPU.

Every comparison is by bit pattern.  oracle/ has no environment map, so nothing here is compared with it: the lookup is pinned to the numpy
restatement of the law (tests/environment_ref.py) through paths that end at their first miss, and deep paths are pinned by exact algebraic
identities — a zero map is a black background, an all-ones map returns the escaping throughput, a one-face map returns it for the paths that leave
through that face, a face colour multiplies it with one rounding, a map times 4 gives the result times 4 — under every kernel form."""
import os

import numpy as np
import pytest

import environment_ref as E
from test_cli import run
from test_gpu_radiance import DEPTH, H, SEED, SPP, W, bits, params_of, same, scene, set_scene, soup, with_form
from test_gpu_ray_query import FORMS

pytestmark = pytest.mark.gpu

E_ARG = -1
SIZES = [1, 2, 5, 16]
SCENES = ["three", "weekend", "stress3000", "cornell4", "cornell4+spheres"]
ALL_FORMS = dict(FORMS, brute={"RT3_BRUTE": "1"})


@pytest.fixture(autouse=True)
def no_map_afterwards(renderer):
    """The session's renderer is shared: whatever a test of this file did, and however it ended, no later test sees a map."""
    yield
    renderer.clear_environment()


def same_words(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d of %d words differ" % (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size)


def frame_rays(rt3, r, cam, p, s=0):
    return r.camera_rays(cam.c, p, s, 1)


def no_flat(rt3, kw):
    """The scene with every FLAT primitive made Lambert: nothing in it emits, so all light comes from the map."""
    kw = dict(kw)
    for k in ("smats", "fmats"):
        if kw.get(k) is not None:
            m = kw[k].copy()
            m["kind"][m["kind"] == rt3.MAT_FLAT] = rt3.MAT_LAMBERT
            kw[k] = m
    return kw


# ------------------------------------------------------------------------------------------------ 1: the lookup law, bit for bit
@pytest.mark.parametrize("n", SIZES)
def test_a_first_miss_is_the_lookup_law(rt3, renderer, n):
    """One sphere of radius 0.01 at (0, 0, -1000), rays from the origin, max_depth 1, one sample: a miss at cast 0 returns env(d) itself.  The -Z
    axis (and, for odd n, the centre of face -Z) points at that sphere; t_min = 1e4 lies behind it, so these rays miss as all others do."""
    cr = np.array([[0.0, 0.0, -1000.0, 0.01]], np.float32)
    sm = np.zeros(1, rt3.MATERIAL)
    sm["kind"], sm["rgb"] = rt3.MAT_LAMBERT, 0.5
    set_scene(rt3, renderer, cr, sm)
    d = E.directions(n)
    rays = np.zeros(len(d), rt3.RAY)                                   # (not make_rays: it normalises again, and the law sees the bits it is given)
    rays["direction"], rays["t_max"] = d, np.inf
    cube = E.random_cube(n, seed=1)
    renderer.set_environment(cube)
    assert renderer.environment_size() == n
    got = renderer.radiance(rays, samples=1, max_depth=1, seed=3, t_min=1e4)
    assert renderer.stats().ray_casts == len(d) and not np.isnan(got).any()
    want = E.lookup(cube, d)
    bad = (bits(got[:, :3]) != bits(want)).any(axis=1)
    assert not bad.any(), "n = %d: %d of %d directions differ, first %s: %s vs %s" % (n, bad.sum(), len(d), d[bad][:3], got[bad][:3], want[bad][:3])
    assert (bits(got[:, 3]) == 0).all()
    renderer.set_environment(cube[..., :3])                            # three channels in: the same map
    same(renderer.radiance(rays, samples=1, max_depth=1, seed=3, t_min=1e4), got, "(6, n, n, 3)")


# ------------------------------------------------------------------------------------------------ 2: a zero map is RT3_FLAG_BLACK_BACKGROUND
def three_results(rt3, r, cam, p, rays):
    pixels = r.render_path(cam.c, p)
    linear = r.accum_resolve(p)
    rad = r.radiance(rays, samples=SPP, max_depth=DEPTH, seed=SEED, flags=p.flags & rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)
    return pixels, linear, rad


@pytest.mark.parametrize("name", SCENES)
def test_a_zero_map_is_a_black_background(rt3, renderer, name, monkeypatch):
    kw, cam, lens, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    black, lit = params_of(rt3, 3, lens), params_of(rt3, 1, lens)
    rays = frame_rays(rt3, renderer, cam, lit)
    want = three_results(rt3, renderer, cam, black, rays)              # no map, the flag
    sky = renderer.render_path(cam.c, lit)
    assert (sky != want[0]).any()                                      # the background matters in this frame
    zero = np.zeros((6, 2, 2, 4), np.float32)
    for form, env in ALL_FORMS.items():
        def run_form():
            renderer.set_environment(zero)
            got = three_results(rt3, renderer, cam, lit, rays)         # the zero map, no flag
            st = renderer.stats()
            renderer.clear_environment()
            return got, three_results(rt3, renderer, cam, black, rays), st
        got, ref, st = with_form(renderer, env, monkeypatch, run_form)
        assert (st.mfma_instructions == 0) == (form == "brute"), form
        for g, w_, r_, what in zip(got, want, ref, ("pixels", "accum_resolve", "radiance")):
            same_words(g, w_, "%s %s: zero map vs the flag" % (form, what))
            same_words(r_, w_, "%s %s: the flag under this form" % (form, what))


# ------------------------------------------------------------------------------------------------ 3: deep paths, exactly
@pytest.mark.parametrize("name", ["three", "weekend", "stress3000"])
def test_deep_paths_obey_the_exact_identities(rt3, renderer, name):
    kw, cam, lens, _ = scene(rt3, name)
    kw = no_flat(rt3, kw)
    assert (kw["smats"]["kind"] != rt3.MAT_FLAT).all()
    set_scene(rt3, renderer, **kw)
    p = params_of(rt3, 1, lens)
    rays = frame_rays(rt3, renderer, cam, p)
    call = lambda: renderer.radiance(rays, samples=1, max_depth=DEPTH, seed=SEED, t_min=0.001)[:, :3]      # noqa: E731
    renderer.set_environment(np.ones((6, 2, 2, 4), np.float32))
    L1 = call()                                                        # the escaping throughput; 0 for a path that was absorbed or ran out of depth
    casts = renderer.stats().ray_casts
    deep = ((L1 > 0) & (L1 < 1)).any(axis=1)                           # escaped after at least one bounce off an albedo below 1
    assert casts >= len(rays) + 100 and deep.sum() >= 50 and (L1 != 0).any(axis=1).mean() > 0.5, (casts, deep.sum())
    escaped = (L1 != 0).any(axis=1)
    face_of = np.full(len(rays), -1)
    for f in range(6):
        one = np.zeros((6, 2, 2, 4), np.float32)
        one[f] = 1.0
        renderer.set_environment(one)
        Lf = call()
        assert renderer.stats().ray_casts == casts                     # the map changes no path
        lit = (Lf != 0).any(axis=1)
        assert not (lit & ~escaped).any() and not (lit & (face_of >= 0)).any(), f
        assert np.array_equal(bits(Lf[lit]), bits(L1[lit])), f
        face_of[lit] = f
    assert (face_of[escaped] >= 0).all() and len(set(face_of[escaped])) >= 2       # exactly one of the six, and more than one face is met
    colours = np.random.default_rng(7).uniform(0.25, 3.0, (6, 3)).astype(np.float32)
    cube = np.zeros((6, 2, 2, 4), np.float32)
    cube[..., :3] = colours[:, None, None, :]
    renderer.set_environment(cube)
    L = call()
    want = np.zeros_like(L1)
    want[escaped] = L1[escaped] * colours[face_of[escaped]]            # float32(L1 * c_f): fma(T, c, 0) rounds once
    assert np.array_equal(bits(L), bits(want))
    rnd = E.random_cube(5, seed=3)
    renderer.set_environment(rnd)
    La = call()
    renderer.set_environment(rnd * np.float32(4.0))
    assert np.array_equal(bits(call()), bits(La * np.float32(4.0))) and (La != 0).any()


# ------------------------------------------------------------------------------------------------ 4: forms agree
@pytest.mark.parametrize("n_faces,n_sph", [(0, 480), (900, 0), (1301, 707)])
def test_every_kernel_form_equals_the_unfiltered_form(rt3, renderer, n_faces, n_sph, monkeypatch):
    rng = np.random.default_rng(161 + n_faces + n_sph)
    rays, _ = soup(rt3, renderer, rng, n_faces, n_sph, 2048)
    renderer.set_environment(E.random_cube(5, seed=4))
    call = lambda: renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=5)      # noqa: E731
    ref = with_form(renderer, {"RT3_BRUTE": "1"}, monkeypatch, call)
    st = renderer.stats()
    assert st.mfma_instructions == 0 and st.ray_casts > 2 * 2048 and not np.isnan(ref).any()
    renderer.clear_environment()
    assert (bits(call()) != bits(ref)).any()                           # the map reaches the result
    renderer.set_environment(E.random_cube(5, seed=4))
    forms = dict(FORMS)
    if n_sph and not n_faces:
        forms.update({"tiled_" + k: dict(v, RT3_FORCE_TILED="1") for k, v in FORMS.items()})     # default = k_trace_mfma32 (<= 512 spheres)
    for name, env in forms.items():
        same(with_form(renderer, env, monkeypatch, call), ref, name)
        assert renderer.stats().mfma_instructions > 0 and renderer.stats().ray_casts == st.ray_casts, name
    for env in ({"RT3_NO_MFMA": "1"}, {"RT3_NO_GROUPS": "1"}, {"RT3_MFMA_K64": "1"}):              # switches of families without such a form: ignored
        same(with_form(renderer, env, monkeypatch, call), ref, str(env))
        assert renderer.stats().mfma_instructions > 0


# ------------------------------------------------------------------------------------------------ 5: render, list and rays forms tie together
@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_radiance_over_camera_rays_is_the_render(rt3, renderer, name):
    kw, cam, lens, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    renderer.set_environment(E.random_cube(5, seed=5))
    p = params_of(rt3, 1, lens)
    keys = np.arange(W * H, dtype=np.uint32)                           # the pixel index: the defining property of rt3.h
    total = np.zeros((W * H, 3), np.float32)
    for s in range(SPP):
        rays = renderer.camera_rays(cam.c, p, s, 1)
        total = total + renderer.radiance(rays, keys=keys, sample_begin=s, samples=1, max_depth=DEPTH, seed=SEED, t_min=0.001)[:, :3]
    want = np.concatenate([total / np.float32(SPP), np.zeros((W * H, 1), np.float32)], axis=1)
    renderer.render_path(cam.c, p)
    same(renderer.accum_resolve(p).reshape(-1, 4), want, "%s: render vs summed single samples" % name)


def test_switches_a_map_ignores(rt3, renderer, monkeypatch):
    for name in ("weekend", "cornell4+spheres"):
        kw, cam, lens, _ = scene(rt3, name)
        set_scene(rt3, renderer, **kw)
        renderer.set_environment(E.random_cube(5, seed=5))
        p = params_of(rt3, 1, lens)
        want = renderer.render_path(cam.c, p)
        for env in ({"RT3_NO_MFMA": "1"}, {"RT3_NO_GROUPS": "1"}, {"RT3_MFMA_K64": "1"}):
            same_words(with_form(renderer, env, monkeypatch, lambda: renderer.render_path(cam.c, p)), want, name + str(env))
            assert renderer.stats().mfma_instructions > 0
        renderer.force_flat_filter(True)
        try:
            same_words(renderer.render_path(cam.c, p), want, name + " force_flat_filter")
        finally:
            renderer.force_flat_filter(False)


@pytest.mark.parametrize("name", ["weekend", "stress3000", "cornell4", "cornell4+spheres"])
def test_adaptive_pixels_are_their_own_sample_range(rt3, renderer, name, monkeypatch):
    kw, cam, lens, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    renderer.set_environment(E.random_cube(5, seed=6))
    p = rt3.make_params(W, H, spp=8, max_depth=DEPTH, seed=SEED, flags=1, lens_radius=lens, t_min=0.001)
    adaptive = lambda: renderer.render_adaptive(cam.c, p, threshold=0.02, min_spp=2, step_spp=2)     # noqa: E731
    pixels, counts = adaptive()
    assert set(np.unique(counts)) <= {2, 4, 6, 8} and len(np.unique(counts)) >= 2 and (counts > 2).sum() > 64       # list rounds ran
    for n in np.unique(counts):
        whole = renderer.render_path_range(cam.c, p, 0, int(n))
        assert np.array_equal(pixels[counts == n], whole[counts == n]), n
    for form, env in ALL_FORMS.items():
        px, ct = with_form(renderer, env, monkeypatch, adaptive)
        assert np.array_equal(ct, counts) and np.array_equal(px, pixels), form


@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_a_shard_union_is_the_whole_frame(rt3, renderer, name):
    kw, cam, lens, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    renderer.set_environment(E.random_cube(5, seed=7))
    whole = renderer.render_path(cam.c, params_of(rt3, 1, lens))
    ps = [params_of(rt3, 1, lens, tile_rows=4, tile_index=i, tile_count=3) for i in range(3)]
    tiles = [renderer.render_path(cam.c, q) for q in ps]
    assert np.array_equal(rt3.deinterleave(tiles, ps, H, W), whole)


# ------------------------------------------------------------------------------------------------ 6: AOVs
@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_aov_miss_albedo_is_the_lookup(rt3, renderer, name):
    kw, cam, lens, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    p = rt3.make_params(W, H, spp=1, max_depth=DEPTH, seed=SEED, flags=1, lens_radius=lens, t_min=0.001)
    before = renderer.render_aov(cam.c, p)
    cube = E.random_cube(16, seed=8)
    renderer.set_environment(cube)
    aov = renderer.render_aov(cam.c, p)
    d = renderer.camera_rays(cam.c, p, 0, 1)["direction"].reshape(H, W, 3)
    miss = aov["kind"] == rt3.HIT_NONE
    assert 50 < miss.sum() < W * H - 50
    assert np.array_equal(bits(aov["albedo"][miss]), bits(E.lookup(cube, d[miss])))
    assert np.array_equal(aov[~miss].tobytes(), before[~miss].tobytes())
    for f in ("coverage", "normal", "depth", "kind", "index"):
        assert np.array_equal(aov[f].tobytes(), before[f].tobytes()), f
    pb = rt3.make_params(W, H, spp=1, max_depth=DEPTH, seed=SEED, flags=3, lens_radius=lens, t_min=0.001)
    assert (renderer.render_aov(cam.c, pb)["albedo"][miss] == 0).all()       # the flag comes first, as in the path law


# ------------------------------------------------------------------------------------------------ 7: state
def test_state(rt3, renderer):
    import ctypes as C
    import torch
    L = rt3.lib()
    kw, cam, lens, _ = scene(rt3, "weekend")
    set_scene(rt3, renderer, **kw)
    p = params_of(rt3, 1, lens)
    assert renderer.environment_size() == 0
    sky = renderer.render_path(cam.c, p)
    cube = E.random_cube(5, seed=9)
    renderer.set_environment(cube)
    assert renderer.environment_size() == 5
    lit = renderer.render_path(cam.c, p)
    assert (lit != sky).any()
    renderer.clear_environment()
    assert renderer.environment_size() == 0
    same_words(renderer.render_path(cam.c, p), sky, "set, then clear")
    renderer.clear_environment()                                       # clearing nothing is no error
    # the map survives scene uploads, updates and regroups
    renderer.set_environment(cube)
    renderer.set_spheres(kw["spheres"], kw["smats"])
    renderer.update_spheres(kw["spheres"])
    renderer.regroup()
    assert renderer.environment_size() == 5
    same_words(renderer.render_path(cam.c, p), lit, "after set_spheres, update_spheres and regroup")
    # a progressive render continues across set_environment of the same map, and of another size and back
    renderer.render_path_range(cam.c, p, 0, 2)
    renderer.set_environment(cube)
    same_words(renderer.render_path_range(cam.c, p, 2, 2), lit, "continued across set_environment")
    # RT3_FLAG_REFERENCE_PRIMARY
    faces, verts, fm = rt3.scene_cornell(4)
    set_scene(rt3, renderer, faces=faces, verts=verts, fmats=fm)
    cam0 = rt3.main_camera(W, H)
    pr = rt3.make_params(W, H, spp=1, max_depth=1, seed=1, flags=rt3.FLAG_REFERENCE_PRIMARY, t_min=0.0)
    out = np.zeros((H, W), np.uint32)
    vp = C.c_void_p
    assert L.rt3_render_path(renderer._ctx, C.byref(cam0.c), C.byref(pr), out.ctypes.data_as(vp)) == E_ARG
    assert b"environment" in L.rt3_last_error(renderer._ctx)
    renderer.clear_environment()
    assert L.rt3_render_path(renderer._ctx, C.byref(cam0.c), C.byref(pr), out.ctypes.data_as(vp)) == 0
    set_scene(rt3, renderer, **kw)
    # refusals leave the previous map in place
    renderer.set_environment(cube)
    rgba = np.ascontiguousarray(np.concatenate([cube[..., :3], np.zeros((6, 5, 5, 1), np.float32)], axis=3))
    bad = rgba.copy()
    bad[3, 2, 1, 1] = np.nan                                           # texel (3 * 5 + 2) * 5 + 1 = 86
    bad[4, 0, 0, 0] = np.inf
    bad[0, 0, 0, 3] = np.nan                                           # the fourth channel is ignored
    assert L.rt3_set_environment(renderer._ctx, bad.ctypes.data_as(vp), 5) == E_ARG
    assert b"texel 86 " in L.rt3_last_error(renderer._ctx)
    with pytest.raises(rt3.Fatal, match="texel 86 "):
        renderer.set_environment(bad)
    assert L.rt3_set_environment(renderer._ctx, None, 5) == E_ARG
    assert L.rt3_set_environment(renderer._ctx, rgba.ctypes.data_as(vp), 2049) == E_ARG
    dev = torch.zeros(6 * 5 * 5 * 4 + 4, dtype=torch.float32, device="cuda")
    dev[:600].copy_(torch.from_numpy(rgba.reshape(-1)))
    assert L.rt3_set_environment_device(renderer._ctx, vp(dev[1:].data_ptr()), 5, None) == E_ARG        # 4 bytes off
    assert L.rt3_set_environment_device(renderer._ctx, None, 5, None) == E_ARG
    assert L.rt3_set_environment_device(renderer._ctx, vp(dev.data_ptr()), 2049, None) == E_ARG
    assert renderer.environment_size() == 5
    same_words(renderer.render_path(cam.c, p), lit, "after the refused calls")
    bad[0, 0, 0, 3] = 0.0
    ok = rgba.copy()
    ok[0, 0, 0, 3] = np.nan
    renderer.set_environment(ok)                                       # a NaN in the ignored channel is no error and changes nothing
    same_words(renderer.render_path(cam.c, p), lit, "NaN in the fourth channel")
    # n_face 0 clears, with a NULL pointer too
    assert L.rt3_set_environment(renderer._ctx, None, 0) == 0 and renderer.environment_size() == 0
    renderer.set_environment(cube)
    assert L.rt3_set_environment_device(renderer._ctx, None, 0, None) == 0 and renderer.environment_size() == 0
    same_words(renderer.render_path(cam.c, p), sky, "cleared by n_face 0")
    # the torch device form equals the host form, on a side stream, replacing a map of another size
    renderer.set_environment(E.random_cube(2, seed=9))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(rgba).to("cuda")
        renderer.set_environment(t)
        t.zero_()                                                      # queued behind the copy: the context owns its own
    s.synchronize()
    assert renderer.environment_size() == 5
    same_words(renderer.render_path(cam.c, p), lit, "torch device form")
    with pytest.raises(rt3.Fatal):
        renderer.set_environment(torch.zeros((6, 5, 5, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(rt3.Fatal):
        renderer.set_environment(np.zeros((6, 5, 4, 4), np.float32))


# ------------------------------------------------------------------------------------------------ 8: the command line
def test_cli_env_gives_the_frame_of_the_api_render(rt3, renderer, tmp_path):
    n, w, h = 5, 32, 18
    cube = E.random_cube(n, seed=10)
    (tmp_path / "env.pfm").write_bytes(rt3.pfm_bytes(np.ascontiguousarray(cube[..., :3].reshape(6 * n, n, 3))))      # the six faces, top to bottom
    rc, out, err = run("-f", "ppm", "-W", str(w), "-H", str(h), "--scene", "three", "--spp", "4", "--depth", "6", "--seed", "9",
                       "--env", str(tmp_path / "env.pfm"), "--hdr", str(tmp_path / "lin.pfm"), "--aov", str(tmp_path / "A"), str(tmp_path / "three.ppm"))
    assert rc == 0, err
    sph, sm = rt3.scene_three_spheres()
    set_scene(rt3, renderer, sph, sm)
    renderer.set_environment(cube)
    cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=6, seed=9, flags=rt3.FLAG_GAMMA2, t_min=0.001)
    frame = rt3.Frame(w, h)
    frame.data[:] = renderer.render_path(cam.c, p)
    assert (tmp_path / "three.ppm").read_bytes() == frame.ppm_bytes()
    assert (tmp_path / "lin.pfm").read_bytes() == rt3.pfm_bytes(renderer.accum_resolve(p)[..., :3])
    assert (tmp_path / "A.albedo.pfm").read_bytes() == rt3.pfm_bytes(renderer.render_aov(cam.c, p)["albedo"])
    renderer.clear_environment()
    assert (renderer.render_path(cam.c, p) != frame.data).any()
    (tmp_path / "bad.pfm").write_bytes(rt3.pfm_bytes(np.zeros((29, 5, 3), np.float32)))                  # 5 x 29: not N x 6N
    rc, out, err = run("-f", "ppm", "-W", str(w), "-H", str(h), "--scene", "three", "--spp", "4", "--env", str(tmp_path / "bad.pfm"),
                       str(tmp_path / "no.ppm"))
    assert rc == -1 and "fatal:" in err and "5 x 29" in err and not os.path.exists(tmp_path / "no.ppm")
    rc, out, err = run("-f", "ppm", "--scene", "three", "--spp", "4", "--env", str(tmp_path / "none.pfm"), str(tmp_path / "no.ppm"))
    assert rc == -1 and "Could not open" in err
