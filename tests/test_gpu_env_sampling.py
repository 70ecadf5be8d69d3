"""Importance sampling of the environment map with shadow rays (RT3_FLAG_ENV_SAMPLING) on the GPU.

The device's table is compared with the Python-integer restatement cell for cell; the flagged render with the plain environment render bit for
bit wherever the two laws must coincide; one bounce with a float64 restatement built from rt3_intersect, the numpy sampler and the numpy lookup;
the estimator's mean with the plain estimator's, by bounds derived from the samples' range (furnace) or from the measured sample variances of
both renders, with a control that holds two plain renders to the same criterion; every kernel route with the unfiltered kernel bit for bit."""
import ctypes as C

import numpy as np
import pytest

import environment_ref as E
import environment_sample_ref as S
from test_cli import run
from test_gpu_radiance import DEPTH, H, SEED, SPP, W, bits, params_of, same, scene, set_scene, soup, with_form
from test_gpu_ray_query import FORMS

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
F32 = np.float32


@pytest.fixture(autouse=True)
def no_map_afterwards(renderer):
    """The session's renderer is shared: whatever a test of this file did, and however it ended, no later test sees a map."""
    yield
    renderer.clear_environment()


def same_words(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d of %d words differ" % (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size)


def one_sphere(rt3, r, albedo=0.5, kind=None, centre=(0.0, 0.0, -3.0), radius=1.0):
    cr = np.array([list(centre) + [radius]], F32)
    sm = np.zeros(1, rt3.MATERIAL)
    sm["kind"], sm["rgb"] = rt3.MAT_LAMBERT if kind is None else kind, albedo
    set_scene(rt3, r, cr, sm)
    return cr, sm


def smooth_cube(n):
    """A smooth bounded map: every channel in [0.2, 1.0], a slow function of the direction."""
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    s, t = np.meshgrid(c, c)
    cube = np.zeros((6, n, n, 4), F32)
    for f in range(6):
        d = E.face_direction(f, s, t)
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        cube[f, ..., 0] = 0.6 + 0.4 * d[..., 1]
        cube[f, ..., 1] = 0.6 + 0.4 * d[..., 0] * d[..., 2]
        cube[f, ..., 2] = 0.6 + 0.4 * np.sin(3.0 * d[..., 0])
    return cube


# ------------------------------------------------------------------------------------------------ 1: the table
@pytest.mark.parametrize("n", [1, 5, 64, 300])
def test_the_device_table_is_the_integer_restatement(rt3, renderer, n):
    import torch
    cube = E.random_cube(n, seed=21)
    cube[..., :3] *= (np.random.default_rng(n).uniform(0, 1, (6, n, n, 1)) < 0.7)       # some dark texels: cells with q = 0 where a whole ring is dark
    cube[0, 0, 0, :3] = 37.0                                                           # one maximum
    T = S.Table(cube)
    renderer.set_environment(cube)
    q, cdf = renderer.environment_table()
    assert q.shape == (6, T.m, T.m) and np.array_equal(q, T.q) and np.array_equal(cdf, T.cdf) and int(cdf.ravel()[-1]) == T.total
    assert q.max() == 2 ** 24
    renderer.set_environment(E.random_cube(max(n - 1, 1), seed=2))                     # another map in between: the table follows the map
    renderer.set_environment(torch.from_numpy(cube).to("cuda"))
    torch.cuda.synchronize()
    q2, cdf2 = renderer.environment_table()
    assert np.array_equal(q2, T.q) and np.array_equal(cdf2, T.cdf)
    zero = np.zeros((6, n, n, 4), F32)
    renderer.set_environment(zero)                                                     # the same size: the copy in place
    q0, cdf0 = renderer.environment_table()
    assert not q0.any() and not cdf0.any()


# ------------------------------------------------------------------------------------------------ 2: exact identities
def frames(rt3, r, cam, lens, flag):
    p = rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=SEED, flags=rt3.FLAG_GAMMA2 | flag, lens_radius=lens, t_min=0.001)
    px = r.render_path(cam.c, p)
    return px, r.accum_resolve(p), r.stats().ray_casts


def test_without_a_lambert_material_the_flag_changes_nothing(rt3, renderer):
    kw, cam, lens, _ = scene(rt3, "weekend")
    sm = kw["smats"].copy()
    lam = sm["kind"] == rt3.MAT_LAMBERT
    sm["kind"][lam] = rt3.MAT_METAL
    sm["param"][lam] = 0.3
    set_scene(rt3, renderer, kw["spheres"], sm)
    renderer.set_environment(E.random_cube(5, seed=22))
    plain, flagged = frames(rt3, renderer, cam, lens, 0), frames(rt3, renderer, cam, lens, rt3.FLAG_ENV_SAMPLING)
    same_words(flagged[0], plain[0], "pixels")
    same_words(flagged[1], plain[1], "linear frame")
    assert flagged[2] == plain[2] and (plain[1] != 0).any()


def test_inside_a_closed_lambert_room_the_flag_changes_nothing(rt3, renderer):
    """The camera inside one large Lambert sphere with objects in it: every shadow ray is blocked and no ray escapes, so L must stay what it was, to
    the bit (a blocked shadow ray adds nothing, it does not add 0) — while the shadow rays are cast and counted.  A second Lambert shell around the
    room keeps "no ray escapes" true in float32: a ray that leaves a point of the room's wall at a grazing angle can miss the wall's far root (the
    hit point lies 1e-5 outside it, the discriminant goes negative), about 3 in 10 000 shadow rays do, and without the shell they reach the map."""
    rng = np.random.default_rng(23)
    cr = np.zeros((14, 4), F32)
    cr[0] = (0.0, 0.0, -3.0, 30.0)
    cr[13] = (0.0, 0.0, -3.0, 45.0)
    cr[1:13, :3] = rng.uniform([-2.0, -1.5, -6.0], [2.0, 1.5, -2.0], (12, 3))
    cr[1:13, 3] = rng.uniform(0.2, 0.6, 12)
    sm = np.zeros(14, rt3.MATERIAL)
    sm["kind"] = [rt3.MAT_LAMBERT] + [k % 4 for k in range(12)] + [rt3.MAT_LAMBERT]      # flat emitters, Lambert, metal, glass inside
    sm["rgb"] = rng.uniform(0.3, 0.9, (14, 3))
    sm["param"] = np.where(sm["kind"] == rt3.MAT_DIELECTRIC, 1.5, 0.1).astype(F32)
    set_scene(rt3, renderer, cr, sm)
    cam = rt3.main_camera(W, H)
    renderer.set_environment(E.random_cube(5, seed=24))
    plain, flagged = frames(rt3, renderer, cam, 0.0, 0), frames(rt3, renderer, cam, 0.0, rt3.FLAG_ENV_SAMPLING)
    same_words(flagged[0], plain[0], "pixels")
    same_words(flagged[1], plain[1], "linear frame")
    assert flagged[2] > plain[2] and (plain[1][..., :3] != 0).any()


@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_an_all_zero_map_changes_nothing(rt3, renderer, name):
    kw, cam, lens, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    renderer.set_environment(np.zeros((6, 5, 5, 4), F32))
    plain, flagged = frames(rt3, renderer, cam, lens, 0), frames(rt3, renderer, cam, lens, rt3.FLAG_ENV_SAMPLING)
    same_words(flagged[0], plain[0], "pixels")
    same_words(flagged[1], plain[1], "linear frame")
    assert flagged[2] == plain[2]                                                      # total == 0: no shadow ray is cast


# ------------------------------------------------------------------------------------------------ 3: one bounce, restated
def rng_base(key, s, seed):
    """hash2(key, hash2(s, seed)) of rays_path / start_path."""
    h = S.hash_u32
    return h(np.asarray(key, np.uint32) ^ h(h(np.uint32(s) ^ h(np.uint32(seed)))))


@pytest.mark.parametrize("n", [5, 300])
def test_one_bounce_equals_the_float64_restatement(rt3, renderer, n):
    """A single Lambert sphere, max_depth 2, one sample: a ray that meets the sphere returns exactly its shadow ray's contribution, albedo c / (pi pdf)
    env(w) — the sphere is convex, so the shadow ray is free whenever c > 0, and the continuation ends at the depth cut-off or at a miss that adds
    nothing.  The normal is formed as the device forms it, in float32 ((fma(t, d, o) - C) * (1 / r)); everything behind it is float64."""
    albedo = np.array([0.7, 0.5, 0.3], F32)
    cr, sm = one_sphere(rt3, renderer, albedo=albedo)
    rng = np.random.default_rng(31 + n)
    k = 1000
    o = (E.unit(rng.normal(0, 1, (k, 3))).astype(np.float64) * rng.uniform(2.0, 4.0, (k, 1)) + cr[0, :3]).astype(F32)
    aim = cr[0, :3] + rng.uniform(-0.75, 0.75, (k, 3))
    aim[:50] = cr[0, :3] + E.unit(rng.normal(0, 1, (50, 3))) * 3.0                     # some that miss
    rays = np.zeros(k, rt3.RAY)
    rays["origin"], rays["direction"], rays["t_max"] = o, E.unit(aim - o), np.inf
    cube = E.random_cube(n, seed=32)
    renderer.set_environment(cube)
    seed = 77
    got = renderer.radiance(rays, samples=1, max_depth=2, seed=seed, flags=rt3.FLAG_ENV_SAMPLING, t_min=0.001)[:, :3]
    hits = renderer.intersect(rays, 0.001)
    hit = hits["kind"] == rt3.HIT_SPHERE
    assert 800 < hit.sum() < k
    same(got[~hit], E.lookup(cube, rays["direction"][~hit]), "a primary miss reads the map")
    d32, t32 = rays["direction"][hit], hits["t"][hit]
    p32 = np.stack([S.fma32(t32, d32[:, i], o[hit][:, i]) for i in range(3)], axis=1)
    n32 = ((p32 - cr[0, :3]) * (F32(1.0) / cr[0, 3])).astype(F32)
    assert ((n32.astype(np.float64) * d32).sum(axis=1) < 0).all()                      # hit from outside: the normal stays
    T = S.Table(cube)
    cell, a, b, w, pdf = S.sample(T, rng_base(np.arange(k, dtype=np.uint32)[hit], 0, seed), 0)
    c = (n32.astype(np.float64) * w.astype(np.float64)).sum(axis=1)
    env = E.lookup(cube, w).astype(np.float64)
    want = np.where((c > 0)[:, None], albedo.astype(np.float64) * (c / (np.pi * pdf.astype(np.float64)))[:, None] * env, 0.0)
    keep = np.abs(c) >= 1e-4
    assert (~keep).mean() <= 0.01, (~keep).sum()
    err = np.abs(got[hit].astype(np.float64) - want)
    bad = keep[:, None] & (err > 1e-4 * np.abs(want) + 1e-6)
    assert not bad.any(), (bad.sum(), err[bad][:4], want[bad][:4])
    assert (want[keep] > 0).any(axis=1).mean() > 0.3 and (c[keep] < 0).sum() > 50     # both branches are met


# ------------------------------------------------------------------------------------------------ 4: furnace
@pytest.mark.parametrize("depth", [2, 6])
def test_furnace_mean(rt3, renderer, depth):
    """One Lambert sphere of albedo a under a constant map c.  The plain estimator returns a c in every sample (the sphere is convex: one bounce, one
    miss).  With the flag a sample is a c cos / (pi pdf); tests/test_environment_sample_ref.py shows pdf within 10 % of 1 / (4 pi) on this map, so a
    sample lies in [0, 4.4 a c] and its standard deviation is at most half that range, 2.2 a c.  The mean of P pixels x 1024 independent samples must
    therefore lie within 6 x 2.2 a c / sqrt(1024 P) of a c."""
    a, c, spp, w, h = 0.5, 0.75, 1024, 64, 48
    one_sphere(rt3, renderer, albedo=a)
    renderer.set_environment(np.full((6, 64, 64, 4), c, F32))
    cam = rt3.main_camera(w, h)
    inside = renderer.render_aov(cam.c, rt3.make_params(w, h, spp=spp, max_depth=depth, seed=5, t_min=0.001))["coverage"] == 1.0
    P = int(inside.sum())
    assert P > 100
    plain = rt3.make_params(w, h, spp=spp, max_depth=depth, seed=5, t_min=0.001)
    renderer.render_path(cam.c, plain)
    ref = renderer.accum_resolve(plain)[..., :3][inside].astype(np.float64)
    assert np.abs(ref - a * c).max() < 1e-5 * a * c                                    # the plain render: a c in every sample
    flagged = rt3.make_params(w, h, spp=spp, max_depth=depth, seed=5, flags=rt3.FLAG_ENV_SAMPLING, t_min=0.001)
    renderer.render_path(cam.c, flagged)
    got = renderer.accum_resolve(flagged)[..., :3][inside].astype(np.float64)
    bound = 6.0 * 2.2 * a * c / np.sqrt(spp * P)
    for ch in range(3):
        mean = got[:, ch].mean()
        print("furnace depth %d channel %d: mean %.6f, a c = %.6f, bound %.6f, P = %d" % (depth, ch, mean, a * c, bound, P))
        assert abs(mean - a * c) <= bound, (mean, a * c, bound)
    assert got.std() > 0                                                               # the flagged samples do vary: it is another estimator


# ------------------------------------------------------------------------------------------------ 5: unbiased with occlusion and interreflection
def moments(rt3, r, cam, p):
    r.render_path(cam.c, p)
    acc, sq, done = r.accum_download(p, want_sq=True)
    assert done == p.spp
    m = acc[..., :3].astype(np.float64) / done
    v = np.maximum(sq[..., :3].astype(np.float64) / done - m * m, 0.0)
    return m, v


def agree(m1, v1, m2, v2, n, what):
    """|m1 - m2| <= 6 sqrt((v1 + v2) / n) + 1e-4 per pixel-channel, at most 0.5 % outside; the frame mean per channel by the same rule with the
    variances summed."""
    out = np.abs(m1 - m2) > 6.0 * np.sqrt((v1 + v2) / n) + 1e-4
    print("%s: %d of %d pixel-channels outside (%.3f %%)" % (what, out.sum(), out.size, 100.0 * out.mean()))
    assert out.mean() <= 0.005, (what, out.mean())
    P = m1.shape[0] * m1.shape[1]
    for ch in range(3):
        M1, M2 = m1[..., ch].mean(), m2[..., ch].mean()
        bound = 6.0 * np.sqrt((v1[..., ch].sum() + v2[..., ch].sum()) / n) / P + 1e-4
        print("%s channel %d: frame means %.6f %.6f, bound %.6f" % (what, ch, M1, M2, bound))
        assert abs(M1 - M2) <= bound, (what, ch, M1, M2, bound)


def test_the_flagged_estimator_has_the_plain_mean(rt3, renderer):
    w, h, spp = 64, 48, 256
    sph = np.array([[0.0, -100.5, -1.0, 100.0], [0.0, 0.0, -1.2, 0.5], [-1.0, 0.0, -1.0, 0.5], [1.0, 0.0, -1.0, 0.5]], F32)
    sm = np.zeros(4, rt3.MATERIAL)                                                     # a ground, a Lambert, a glass and a metal sphere
    sm["kind"] = (rt3.MAT_LAMBERT, rt3.MAT_LAMBERT, rt3.MAT_DIELECTRIC, rt3.MAT_METAL)
    sm["rgb"] = ((0.8, 0.8, 0.0), (0.1, 0.2, 0.5), (1.0, 1.0, 1.0), (0.8, 0.6, 0.2))
    sm["param"] = (0.0, 0.0, 1.5, 0.2)
    set_scene(rt3, renderer, sph, sm)
    renderer.set_environment(smooth_cube(32))
    cam = rt3.Camera().update(w, h, 1.0, F32(w) / F32(h) * F32(2.0), 2.0)
    par = lambda seed, flag: rt3.make_params(w, h, spp=spp, max_depth=6, seed=seed, flags=rt3.FLAG_VARIANCE | flag, t_min=0.001)     # noqa: E731
    m1, v1 = moments(rt3, renderer, cam, par(3, 0))
    m2, v2 = moments(rt3, renderer, cam, par(4, 0))
    agree(m1, v1, m2, v2, spp, "control: two plain renders")                           # the criterion is fair: the reference itself meets it
    m3, v3 = moments(rt3, renderer, cam, par(3, rt3.FLAG_ENV_SAMPLING))
    assert (m3 != m1).any()
    agree(m1, v1, m3, v3, spp, "plain against flagged")


# ------------------------------------------------------------------------------------------------ 6: forms agree
@pytest.mark.parametrize("n_faces,n_sph", [(0, 480), (900, 0), (1301, 707)])
def test_every_kernel_route_equals_the_unfiltered_kernel(rt3, renderer, n_faces, n_sph, monkeypatch):
    rng = np.random.default_rng(261 + n_faces + n_sph)
    rays, _ = soup(rt3, renderer, rng, n_faces, n_sph, 2048)
    renderer.set_environment(E.random_cube(5, seed=26))
    cam = rt3.main_camera(W, H)
    p = rt3.make_params(W, H, spp=2, max_depth=DEPTH, seed=9, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_ENV_SAMPLING, t_min=0.001)

    def call():
        rad = renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=5, flags=rt3.FLAG_ENV_SAMPLING)
        st = renderer.stats()
        px = renderer.render_path(cam.c, p)
        return rad, px, renderer.accum_resolve(p), st, renderer.stats()

    ref = with_form(renderer, {"RT3_BRUTE": "1"}, monkeypatch, call)
    assert ref[3].mfma_instructions == 0 and ref[4].mfma_instructions == 0 and not np.isnan(ref[0]).any()
    plain = renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=5)
    assert ref[3].ray_casts > renderer.stats().ray_casts and (bits(plain) != bits(ref[0])).any()      # shadow rays were cast and reach the result
    forms = dict(FORMS)
    if n_sph and not n_faces:
        forms.update({"tiled_" + k: dict(v, RT3_FORCE_TILED="1") for k, v in FORMS.items()})      # default = k_trace_mfma32 (<= 512 spheres)
    for name, env in forms.items():
        got = with_form(renderer, env, monkeypatch, call)
        same(got[0], ref[0], name + " radiance")
        same_words(got[1], ref[1], name + " pixels")
        same_words(got[2], ref[2], name + " linear frame")
        assert got[3].mfma_instructions > 0 and got[4].mfma_instructions > 0, name
        assert got[3].ray_casts == ref[3].ray_casts and got[4].ray_casts == ref[4].ray_casts, name


# ------------------------------------------------------------------------------------------------ 7: composition
@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_radiance_ranges_and_shards_compose(rt3, renderer, name):
    kw, cam, lens, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    renderer.set_environment(E.random_cube(5, seed=27))
    flag = rt3.FLAG_ENV_SAMPLING
    p = params_of(rt3, rt3.FLAG_GAMMA2 | flag, lens)
    keys = np.arange(W * H, dtype=np.uint32)
    total = np.zeros((W * H, 3), F32)
    for s in range(SPP):
        rays = renderer.camera_rays(cam.c, p, s, 1)
        total = total + renderer.radiance(rays, keys=keys, sample_begin=s, samples=1, max_depth=DEPTH, seed=SEED, flags=flag, t_min=0.001)[:, :3]
    want = np.concatenate([total / F32(SPP), np.zeros((W * H, 1), F32)], axis=1)
    whole = renderer.render_path(cam.c, p)
    linear = renderer.accum_resolve(p)
    same(linear.reshape(-1, 4), want, "%s: render vs summed single samples" % name)
    renderer.render_path_range(cam.c, p, 0, 1)
    renderer.render_path_range(cam.c, p, 1, 2)
    same_words(renderer.render_path_range(cam.c, p, 3, 1), whole, "a partition of the sample range")
    same_words(renderer.accum_resolve(p), linear, "... and its accumulation")
    ps = [params_of(rt3, rt3.FLAG_GAMMA2 | flag, lens, tile_rows=4, tile_index=i, tile_count=2) for i in range(2)]
    tiles = [renderer.render_path(cam.c, q) for q in ps]
    assert np.array_equal(rt3.deinterleave(tiles, ps, H, W), whole)
    renderer.render_path(cam.c, params_of(rt3, rt3.FLAG_GAMMA2, lens))
    assert (renderer.accum_resolve(p) != linear).any()                                 # the flag does change this frame


# ------------------------------------------------------------------------------------------------ 8: variance falls
def test_a_small_bright_block_is_found(rt3, renderer):
    """A map that is zero except one bright 2 x 2 block overhead, a Lambert ground under it: the summed per-pixel sample variance over the ground's
    pixels is lower with the flag (the ratio is a measurement: tools/bench_env_sampling.py logs it)."""
    w, h, spp, n = 64, 48, 64, 32
    cr = np.array([[0.0, -1000.5, -3.0, 1000.0]], F32)
    sm = np.zeros(1, rt3.MATERIAL)
    sm["kind"], sm["rgb"] = rt3.MAT_LAMBERT, 0.6
    set_scene(rt3, renderer, cr, sm)
    cube = np.zeros((6, n, n, 4), F32)
    cube[2, 20:22, 9:11, :3] = 400.0
    renderer.set_environment(cube)
    cam = rt3.Camera().look_at(w, h, (0.0, 1.0, 1.0), (0.0, -0.5, -3.0), (0.0, 1.0, 0.0), 50.0, 4.0)
    ground = renderer.render_aov(cam.c, rt3.make_params(w, h, spp=4, max_depth=4, seed=2, t_min=0.001))["coverage"] == 1.0
    assert ground.sum() > 1000
    var = {}
    for flag in (0, rt3.FLAG_ENV_SAMPLING):
        m, v = moments(rt3, renderer, cam, rt3.make_params(w, h, spp=spp, max_depth=4, seed=2, flags=rt3.FLAG_VARIANCE | flag, t_min=0.001))
        var[flag] = v[ground].sum()
        assert m[ground].sum() > 0
    print("summed variance over %d ground pixels: plain %.4g, flagged %.4g, ratio %.1f" % (ground.sum(), var[0], var[16], var[0] / var[16]))
    assert var[16] < var[0]


# ------------------------------------------------------------------------------------------------ 9: state and errors
def test_state_and_refusals(rt3, renderer):
    L = rt3.lib()
    vp = C.c_void_p
    kw, cam, lens, _ = scene(rt3, "weekend")
    set_scene(rt3, renderer, **kw)
    flag = rt3.FLAG_ENV_SAMPLING
    p = params_of(rt3, rt3.FLAG_GAMMA2 | flag, lens)
    out = np.zeros((H, W), np.uint32)
    rays = renderer.camera_rays(cam.c, p, 0, 1)
    rad = np.zeros((len(rays), 4), F32)

    def render_rc(q):
        return L.rt3_render_path(renderer._ctx, C.byref(cam.c), C.byref(q), out.ctypes.data_as(vp))

    def radiance_rc(flags):
        rp = rt3.RADIANCE_PARAMS(DEPTH, SEED, flags, 0, 1, 0.001)
        return L.rt3_radiance(renderer._ctx, rays.ctypes.data_as(vp), None, len(rays), C.byref(rp), rad.ctypes.data_as(vp))

    # no map: RT3_E_STATE
    assert renderer.environment_size() == 0
    assert render_rc(p) == E_STATE and b"environment map" in L.rt3_last_error(renderer._ctx)
    assert radiance_rc(flag) == E_STATE
    m = C.c_uint32(0)
    q8, c8 = np.zeros(8, np.uint32), np.zeros(8, np.uint64)
    assert L.rt3_debug_environment_table(renderer._ctx, q8.ctypes.data_as(vp), c8.ctypes.data_as(vp), 8, C.byref(m)) == E_STATE
    cube = E.random_cube(5, seed=28)
    renderer.set_environment(cube)
    # flags that exclude it: RT3_E_ARG
    for extra in (rt3.FLAG_BLACK_BACKGROUND, rt3.FLAG_REFERENCE_PRIMARY):
        assert render_rc(params_of(rt3, flag | extra, lens)) == E_ARG, extra
        assert b"RT3_FLAG_ENV_SAMPLING cannot be combined" in L.rt3_last_error(renderer._ctx), extra      # the flag's own refusal, not an older one
    assert radiance_rc(flag | rt3.FLAG_BLACK_BACKGROUND) == E_ARG and radiance_rc(flag | 4) == E_ARG
    with pytest.raises(rt3.Fatal, match="adaptive"):
        renderer.render_adaptive(cam.c, rt3.make_params(W, H, spp=8, max_depth=DEPTH, seed=SEED, flags=flag, t_min=0.001), min_spp=2, step_spp=2)
    assert L.rt3_debug_environment_table(renderer._ctx, q8.ctypes.data_as(vp), c8.ctypes.data_as(vp), 8, C.byref(m)) == E_ARG and m.value == 5
    # the AOV pass ignores the flag
    plain_p = params_of(rt3, rt3.FLAG_GAMMA2, lens)
    assert renderer.render_aov(cam.c, p).tobytes() == renderer.render_aov(cam.c, plain_p).tobytes()
    # the render; ray_casts >= the plain count
    lit = renderer.render_path(cam.c, p)
    casts = renderer.stats().ray_casts
    plain = renderer.render_path(cam.c, plain_p)
    assert casts >= renderer.stats().ray_casts and (lit != plain).any()
    # the table survives scene uploads, updates and regroups
    table = renderer.environment_table()
    renderer.set_spheres(kw["spheres"], kw["smats"])
    renderer.update_spheres(kw["spheres"])
    renderer.regroup()
    after = renderer.environment_table()
    assert np.array_equal(after[0], table[0]) and np.array_equal(after[1], table[1])
    same_words(renderer.render_path(cam.c, p), lit, "after set_spheres, update_spheres and regroup")
    # replacing the map rebuilds the table, and the results follow; back again gives the first frame
    other = E.random_cube(7, seed=29)
    renderer.set_environment(other)
    lit2 = renderer.render_path(cam.c, p)
    assert (lit2 != lit).any() and np.array_equal(renderer.environment_table()[0], S.Table(other).q)
    renderer.set_environment(cube * F32(1.0))
    same_words(renderer.render_path(cam.c, p), lit, "the first map again")
    renderer.clear_environment()
    assert render_rc(p) == E_STATE
    renderer.set_environment(cube)
    # a progressive accumulation is untouched by a flagged rt3_radiance
    renderer.render_path_range(cam.c, p, 0, 2)
    renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=3, flags=flag)
    same_words(renderer.render_path_range(cam.c, p, 2, 2), lit, "continued across a flagged rt3_radiance")


def test_cli_env_sampling_gives_the_frame_of_the_api_render(rt3, renderer, tmp_path):
    n, w, h = 5, 32, 18
    cube = E.random_cube(n, seed=30)
    (tmp_path / "env.pfm").write_bytes(rt3.pfm_bytes(np.ascontiguousarray(cube[..., :3].reshape(6 * n, n, 3))))
    rc, out, err = run("-f", "ppm", "-W", str(w), "-H", str(h), "--scene", "three", "--spp", "4", "--depth", "6", "--seed", "9",
                       "--env", str(tmp_path / "env.pfm"), "--env-sampling", "--hdr", str(tmp_path / "lin.pfm"), str(tmp_path / "three.ppm"))
    assert rc == 0, err
    sph, sm = rt3.scene_three_spheres()
    set_scene(rt3, renderer, sph, sm)
    renderer.set_environment(cube)
    cam = rt3.Camera().update(w, h, 1.0, F32(w) / F32(h) * F32(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=6, seed=9, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_ENV_SAMPLING, t_min=0.001)
    frame = rt3.Frame(w, h)
    frame.data[:] = renderer.render_path(cam.c, p)
    assert (tmp_path / "three.ppm").read_bytes() == frame.ppm_bytes()
    assert (tmp_path / "lin.pfm").read_bytes() == rt3.pfm_bytes(renderer.accum_resolve(p)[..., :3])
    plain = renderer.render_path(cam.c, rt3.make_params(w, h, spp=4, max_depth=6, seed=9, flags=rt3.FLAG_GAMMA2, t_min=0.001))
    assert (plain != frame.data).any()
    rc, out, err = run("-f", "ppm", "--scene", "cornell", "--spp", "4", "--env", str(tmp_path / "env.pfm"), "--env-sampling", str(tmp_path / "no.ppm"))
    assert rc == -1 and "RT3_FLAG_BLACK_BACKGROUND" in err                             # the box's background is black: the library refuses
