"""Importance sampling of the emissive primitives with shadow rays (RT3_FLAG_LIGHT_SAMPLING) on the GPU.

The device's table is compared with the Python-integer restatement entry for entry; the flagged render with the plain render bit for bit wherever
the two laws must coincide; one bounce with a float64 restatement built from rt3_intersect and the numpy sampler; the estimator's mean with the
plain estimator's, by bounds derived from the samples' range (furnace) or from the measured sample variances of both renders, with a control that
holds two plain renders to the same criterion; every kernel route with the unfiltered kernel bit for bit; the defining property of rt3_radiance."""
import ctypes as C

import numpy as np
import pytest

import environment_ref as E
import light_sample_ref as S
from environment_sample_ref import fma32
from test_cli import run
from test_gpu_env_sampling import agree, moments, rng_base, same_words
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


def table_of(kw):
    return S.Table(kw.get("faces"), kw.get("verts"), kw.get("fmats"), kw.get("spheres"), kw.get("smats"))


def check_table(r, kw, what):
    T = table_of(kw)
    q, cdf = r.light_table()
    assert len(q) == len(T.q), what
    assert np.array_equal(q, T.q), "%s: %d entries of q differ" % (what, (q != T.q).sum())
    assert np.array_equal(cdf, T.cdf) and int(cdf[-1]) == T.total, what
    return T


def frames(rt3, r, cam, lens, flags, depth=DEPTH):
    p = rt3.make_params(W, H, spp=SPP, max_depth=depth, seed=SEED, flags=rt3.FLAG_GAMMA2 | flags, lens_radius=lens, t_min=0.001)
    px = r.render_path(cam.c, p)
    return px, r.accum_resolve(p), r.stats().ray_casts


# ------------------------------------------------------------------------------------------------ 1: the table
def test_the_device_table_is_the_integer_restatement(rt3, renderer):
    rng = np.random.default_rng(401)
    _, (faces, verts, fm, cr, sm) = soup(rt3, renderer, rng, 301, 207, 16)
    kw = dict(faces=faces, verts=verts, fmats=fm, spheres=cr, smats=sm)
    T = check_table(renderer, kw, "a mixed soup")
    assert T.q.max() == 2 ** 24 and (T.q[:301] > 0).any() and (T.q[301:] > 0).any() and (T.q == 0).any()
    assert (T.q[[3, 7]] == 0).all()                                                    # the soup's faces with coincident vertices
    # it follows the scene: changed radii, moved vertices, other materials
    cr2 = cr.copy()
    cr2[:, 3] *= rng.uniform(0.5, 1.5, len(cr)).astype(F32)
    renderer.update_spheres(cr2)
    kw["spheres"] = cr2
    T2 = check_table(renderer, kw, "after update_spheres")
    assert (T2.q != T.q).any()
    verts2 = verts.copy()
    verts2[:, :3] += rng.normal(0, 0.05, (len(verts), 3)).astype(F32)
    renderer.update_mesh(verts2)
    kw["verts"] = verts2
    T3 = check_table(renderer, kw, "after update_mesh")
    assert (T3.q != T2.q).any()
    sm2 = sm.copy()
    sm2["kind"] = (sm["kind"] + 1) % 4
    renderer.set_spheres(cr2, sm2)
    kw["smats"] = sm2
    T4 = check_table(renderer, kw, "after a material re-upload")
    assert (T4.q != T3.q).any()
    # ... and stays through what leaves the scene alone
    before = renderer.light_table()
    renderer.regroup()
    renderer.set_environment(E.random_cube(5, seed=41))
    after = renderer.light_table()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_the_table_of_the_box_and_of_a_scene_without_an_emitter(rt3, renderer):
    kw, cam, lens, _ = scene(rt3, "cornell4+spheres")
    set_scene(rt3, renderer, **kw)
    T = check_table(renderer, kw, "cornell4+spheres")
    assert T.total > 0 and (T.q[:len(kw["faces"])] > 0).sum() >= 2 and (T.q[len(kw["faces"]):] > 0).sum() == 10
    kw, cam, lens, _ = scene(rt3, "weekend")
    set_scene(rt3, renderer, **kw)
    q, cdf = renderer.light_table()
    assert len(q) == len(kw["spheres"]) and not q.any() and not cdf.any()


# ------------------------------------------------------------------------------------------------ 2: exact identities
def identical(rt3, r, cam, lens, flags=0, depth=DEPTH, more_casts=False):
    plain, flagged = frames(rt3, r, cam, lens, flags, depth), frames(rt3, r, cam, lens, flags | rt3.FLAG_LIGHT_SAMPLING, depth)
    same_words(flagged[0], plain[0], "pixels")
    same_words(flagged[1], plain[1], "linear frame")
    assert (plain[1][..., :3] != 0).any()
    if more_casts:
        assert flagged[2] > plain[2]
    else:
        assert flagged[2] == plain[2]


def test_without_an_emitter_the_flag_changes_nothing(rt3, renderer):
    kw, cam, lens, _ = scene(rt3, "weekend")
    sm = kw["smats"].copy()
    sm["kind"][5], sm["rgb"][5] = rt3.MAT_FLAT, (0.0, 0.0, 0.0)                        # a FLAT sphere of brightness 0 is no emitter
    set_scene(rt3, renderer, kw["spheres"], sm)
    assert not renderer.light_table()[0].any()
    identical(rt3, renderer, cam, lens)                                                # total == 0: no shadow ray is cast


def test_without_a_lambert_material_the_flag_changes_nothing(rt3, renderer):
    kw, cam, lens, _ = scene(rt3, "weekend")
    sm = kw["smats"].copy()
    lam = np.nonzero(sm["kind"] == rt3.MAT_LAMBERT)[0]
    sm["kind"][lam] = rt3.MAT_METAL
    sm["param"][lam] = 0.3
    sm["kind"][lam[1::3]] = rt3.MAT_FLAT                                               # ... and emitters among them
    set_scene(rt3, renderer, kw["spheres"], sm)
    assert renderer.light_table()[0].any()
    identical(rt3, renderer, cam, lens, rt3.FLAG_BLACK_BACKGROUND)


def test_at_depth_one_the_flag_changes_nothing(rt3, renderer):
    kw, cam, lens, _ = scene(rt3, "cornell4+spheres")
    set_scene(rt3, renderer, **kw)
    identical(rt3, renderer, cam, lens, rt3.FLAG_BLACK_BACKGROUND, depth=1)


def test_emitters_inside_a_closed_lambert_shell_change_nothing(rt3, renderer):
    """Every emitter — two spheres and a triangle — sits inside a closed opaque Lambert shell that the camera looks at from outside: every shadow ray
    is blocked by the shell and no continuation reaches an emitter, so L must stay what it was, to the bit (a blocked shadow ray adds nothing, it does
    not add 0) — while the shadow rays are cast and counted.  Two nested shells, for the reason given in
    test_inside_a_closed_lambert_room_the_flag_changes_nothing of test_gpu_env_sampling.py: a ray that leaves a point of the outer shell at a grazing
    angle can miss the shell's far root in float32 and get inside it; the inner shell stops it."""
    cr = np.array([[0.0, -100.5, -3.0, 100.0], [0.0, 0.35, -3.0, 0.8], [0.0, 0.35, -3.0, 0.7], [0.1, 0.4, -3.0, 0.2], [-0.2, 0.2, -3.1, 0.1],
                   [1.3, 0.0, -2.5, 0.4], [-1.3, 0.0, -2.5, 0.4]], F32)
    sm = np.zeros(7, rt3.MATERIAL)
    sm["kind"] = (rt3.MAT_LAMBERT, rt3.MAT_LAMBERT, rt3.MAT_LAMBERT, rt3.MAT_FLAT, rt3.MAT_FLAT, rt3.MAT_METAL, rt3.MAT_DIELECTRIC)
    sm["rgb"] = ((0.6, 0.6, 0.5), (0.7, 0.4, 0.4), (0.5, 0.5, 0.5), (4.0, 3.0, 2.0), (1.0, 5.0, 1.0), (0.8, 0.8, 0.8), (1.0, 1.0, 1.0))
    sm["param"] = (0, 0, 0, 0, 0, 0.1, 1.5)
    faces = np.zeros(1, rt3.GFACE)
    faces["v2"], faces["v3"] = 1, 2
    verts = np.array([[-0.2, 0.1, -2.8, 0], [0.2, 0.1, -2.8, 0], [0.0, 0.5, -2.9, 0]], F32)
    n = np.cross(verts[2, :3] - verts[0, :3], verts[1, :3] - verts[0, :3])
    faces["normal"] = n / np.linalg.norm(n)
    fm = np.zeros(1, rt3.MATERIAL)
    fm["rgb"] = (2.0, 2.0, 6.0)
    set_scene(rt3, renderer, cr, sm, faces, verts, fm)
    assert (renderer.light_table()[0] > 0).sum() == 3
    identical(rt3, renderer, rt3.main_camera(W, H), 0.0, more_casts=True)              # under the sky: the plain miss is the flagged miss


# ------------------------------------------------------------------------------------------------ 3: one bounce, restated
@pytest.mark.parametrize("case", ["lamp outside", "inside an emissive sphere"])
def test_one_bounce_equals_the_float64_restatement(rt3, renderer, case):
    """One Lambert sphere, one emissive sphere, one emissive triangle, max_depth 2, black background, one sample: a ray that meets the Lambert sphere
    returns exactly its shadow ray's contribution, albedo k rgb_light where the shadow ray's nearest hit is the chosen light and 0 elsewhere — the
    continuation ends at the depth cut-off, at a miss under the black background, or at an emitter of the table, which adds nothing behind a Lambert
    scatter.  The hit point and the normal are formed as the device forms them, in float32; the light, the sampled point and which samples are dropped
    come from the numpy restatement of the law (float32, bit for bit the device's); visibility from rt3_intersect along the restated shadow ray; the
    value of k in float64.  The criterion is test_gpu_env_sampling.py's: 1e-4 relative + 1e-6, the samples with a cosine below 1e-4 left out (here
    either of the two cosines of the law), at most 1 % of them.  In the second case the emissive sphere encloses the scene: every hit point lies inside
    it, and every point of it counts."""
    albedo = np.array([0.7, 0.5, 0.3], F32)
    big = case != "lamp outside"
    cr = np.array([[0.0, 0.0, -3.0, 1.0], [0.3, 0.2, -2.5, 25.0] if big else [1.2, 1.6, -2.2, 0.4]], F32)
    sm = np.zeros(2, rt3.MATERIAL)
    sm["kind"], sm["rgb"] = (rt3.MAT_LAMBERT, rt3.MAT_FLAT), (albedo, (0.5, 0.25, 1.0) if big else (9.0, 6.0, 3.0))
    faces = np.zeros(1, rt3.GFACE)
    faces["v2"], faces["v3"] = 1, 2
    verts = np.array([[1.03, 0.79, -2.5, 0], [0.47, 1.21, -2.5, 0], [0.86, 1.15, -2.965, 0]], F32)     # between the lamp and the sphere: it shadows
    nrm = np.cross(verts[2, :3] - verts[0, :3], verts[1, :3] - verts[0, :3])
    faces["normal"] = nrm / np.linalg.norm(nrm)
    fm = np.zeros(1, rt3.MATERIAL)
    fm["rgb"] = (3000.0, 8000.0, 5000.0) if big else (3.0, 8.0, 5.0)              # (bright enough to be drawn beside 7854 units of area)
    set_scene(rt3, renderer, cr, sm, faces, verts, fm)
    T = S.Table(faces, verts, fm, cr, sm)
    assert (T.q > 0).sum() == 2
    rng = np.random.default_rng(33)
    k = 1000
    o = (E.unit(rng.normal(0, 1, (k, 3))).astype(np.float64) * rng.uniform(2.0, 4.0, (k, 1)) + cr[0, :3]).astype(F32)
    aim = cr[0, :3] + rng.uniform(-0.75, 0.75, (k, 3))
    aim[:50] = cr[0, :3] + E.unit(rng.normal(0, 1, (50, 3))) * 3.0                     # some that miss the Lambert sphere
    rays = np.zeros(k, rt3.RAY)
    rays["origin"], rays["direction"], rays["t_max"] = o, E.unit(aim - o), np.inf
    seed = 78
    flags = rt3.FLAG_LIGHT_SAMPLING | rt3.FLAG_BLACK_BACKGROUND
    got = renderer.radiance(rays, samples=1, max_depth=2, seed=seed, flags=flags, t_min=0.001)[:, :3]
    hits = renderer.intersect(rays, 0.001)
    hit = (hits["kind"] == rt3.HIT_SPHERE) & (hits["index"] == 0)
    assert 700 < hit.sum() < k
    first = np.where((hits["kind"] == rt3.HIT_SPHERE)[:, None], sm["rgb"][np.minimum(hits["index"], 1)],
                     np.where((hits["kind"] == rt3.HIT_FACE)[:, None], fm["rgb"][0], 0.0)).astype(F32)
    same(got[~hit], first[~hit], "a primary ray that meets an emitter, or nothing")
    o32, d32, t32 = o[hit], rays["direction"][hit], hits["t"][hit]
    p32 = np.stack([fma32(t32, d32[:, i], o32[:, i]) for i in range(3)], axis=1)
    n32 = ((p32 - cr[0, :3]) * (F32(1.0) / cr[0, 3])).astype(F32)
    assert ((n32.astype(np.float64) * d32).sum(axis=1) < 0).all()                      # hit from outside: the normal stays
    light, point, normal, area, pl, a, b = S.sample(T, rng_base(np.arange(k, dtype=np.uint32)[hit], 0, seed), 0)
    keep, w32, k32 = S.connect(T, light, point, normal, area, pl, p32, n32)
    assert 100 <= keep.sum() < len(keep) and (light == 0).any() and (light == 2).any()      # not vacuous: kept and dropped samples, both lights
    shadow = np.zeros(int(keep.sum()), rt3.RAY)
    shadow["origin"], shadow["direction"], shadow["t_max"] = p32[keep], w32[keep], np.inf
    sh = renderer.intersect(shadow, 0.001)
    assert (sh["kind"] != rt3.HIT_INVALID).all()
    entry = np.where(sh["kind"] == rt3.HIT_FACE, sh["index"], np.where(sh["kind"] == rt3.HIT_SPHERE, sh["index"] + 1, 0xFFFFFFFF))
    seen = np.zeros(len(keep), bool)
    seen[keep] = entry == light[keep]
    assert seen.sum() >= 50 and (keep & ~seen).any()                                  # lit, and in shadow
    D = point.astype(np.float64) - p32
    d2 = (D * D).sum(axis=1)
    w = D / np.sqrt(d2)[:, None]
    c = (n32.astype(np.float64) * w).sum(axis=1)
    dl = (normal.astype(np.float64) * w).sum(axis=1)
    k64 = c * np.abs(dl) * area.astype(np.float64) / (np.pi * d2 * pl.astype(np.float64))
    want = np.where(seen[:, None], albedo.astype(np.float64) * k64[:, None] * T.rgb[light].astype(np.float64), 0.0)
    sure = (np.abs(c) >= 1e-4) & (np.abs(dl) >= 1e-4)
    assert (~sure).mean() <= 0.01, (~sure).sum()
    err = np.abs(got[hit].astype(np.float64) - want)
    bad = sure[:, None] & (err > 1e-4 * np.abs(want) + 1e-6)
    assert not bad.any(), (bad.sum(), err[bad][:4], want[bad][:4])
    if big:                                                                            # from inside the sphere no sample is dropped for its side
        on_big = light == 2
        assert (on_big & keep).sum() >= 50 and (dl[on_big & keep] > 0).all()        # v . w > 0: the side a hit point outside the sphere would not get


# ------------------------------------------------------------------------------------------------ 4: the estimator's mean
@pytest.mark.parametrize("depth", [2, 6])
def test_furnace_mean(rt3, renderer, depth):
    """A Lambert sphere of albedo a and radius 1 at the centre of one FLAT sphere of radius R = 10 and radiance 1, the camera inside.  The plain estimator
    returns a in every sample of a pixel on the Lambert sphere (convex: one bounce, then the emitter).  With the flag the continuation's hit on the emitter
    adds nothing and a sample is a (c cl A) / (pi d2 pl) with pl = 1, A = 4 pi R^2 and d >= R - 1: a sample lies in [0, 4 a R^2 / (R - 1)^2] and its
    standard deviation is at most half that range.  The mean of P pixels x 1024 independent samples must therefore lie within 6 half-ranges /
    sqrt(1024 P) of a (the emitter encloses the hemisphere of every hit point: the integral of c cl / (pi d2) over it is 1)."""
    a, R, spp, w, h = 0.5, 10.0, 1024, 64, 48
    cr = np.array([[0.0, 0.0, -3.0, 1.0], [0.0, 0.0, -3.0, R]], F32)
    sm = np.zeros(2, rt3.MATERIAL)
    sm["kind"], sm["rgb"] = (rt3.MAT_LAMBERT, rt3.MAT_FLAT), ((a, a, a), (1.0, 1.0, 1.0))
    set_scene(rt3, renderer, cr, sm)
    cam = rt3.main_camera(w, h)
    plain = rt3.make_params(w, h, spp=spp, max_depth=depth, seed=5, t_min=0.001)
    renderer.render_path(cam.c, plain)
    ref = renderer.accum_resolve(plain)[..., :3].astype(np.float64)
    inside = (np.abs(ref - a) < 1e-5 * a).all(axis=-1)                                  # the plain render: a in every sample of a pixel on the sphere
    P = int(inside.sum())
    assert P > 100 and (np.abs(ref[~inside] - 1.0) < 1e-5).all(axis=-1).sum() > 100
    flagged = rt3.make_params(w, h, spp=spp, max_depth=depth, seed=5, flags=rt3.FLAG_LIGHT_SAMPLING, t_min=0.001)
    renderer.render_path(cam.c, flagged)
    got = renderer.accum_resolve(flagged)[..., :3].astype(np.float64)
    assert np.array_equal(got[(np.abs(ref - 1.0) < 1e-5).all(axis=-1)], ref[(np.abs(ref - 1.0) < 1e-5).all(axis=-1)])      # a primary hit on the emitter adds as always
    got = got[inside]
    half_range = 0.5 * 4.0 * a * R * R / (R - 1.0) ** 2
    bound = 6.0 * half_range / np.sqrt(spp * P)
    for ch in range(3):
        mean = got[:, ch].mean()
        print("furnace depth %d channel %d: mean %.6f, a = %.6f, bound %.6f, P = %d" % (depth, ch, mean, a, bound, P))
        assert abs(mean - a) <= bound, (mean, a, bound)
    assert got.std() > 0                                                               # the flagged samples do vary: it is another estimator


def test_the_flagged_estimator_has_the_plain_mean_in_the_box(rt3, renderer):
    """cornell4+spheres under a black background: the box's light and ten flat spheres emit, walls and spheres of every kind occlude and interreflect.
    The criterion and its control are test_gpu_env_sampling.py's (agree): bounds from the measured sample variances of both renders."""
    w, h, spp = 64, 48, 256
    kw, _, _, _ = scene(rt3, "cornell4+spheres")
    set_scene(rt3, renderer, **kw)
    cam = rt3.Camera().look_at(w, h, (0.3, 0.2, 0.5), (0.0, -0.1, -3.0), (0.0, 1.0, 0.0), 50.0, 3.5)
    par = lambda seed, flag: rt3.make_params(w, h, spp=spp, max_depth=6, seed=seed, flags=rt3.FLAG_VARIANCE | rt3.FLAG_BLACK_BACKGROUND | flag,     # noqa: E731
                                             t_min=0.001)
    m1, v1 = moments(rt3, renderer, cam, par(3, 0))
    m2, v2 = moments(rt3, renderer, cam, par(4, 0))
    agree(m1, v1, m2, v2, spp, "control: two plain renders")                           # the criterion is fair: the reference itself meets it
    m3, v3 = moments(rt3, renderer, cam, par(3, rt3.FLAG_LIGHT_SAMPLING))
    assert (m3 != m1).any()
    agree(m1, v1, m3, v3, spp, "plain against flagged")


# ------------------------------------------------------------------------------------------------ 5: noise falls
def test_a_small_lamp_is_found(rt3, renderer):
    """A Lambert floor and one emissive sphere of radius 0.05 above it, black background: the summed per-pixel sample variance over the floor's pixels
    is lower with the flag (the ratio is a measurement: tools/bench_light_sampling.py logs it).  The floor's pixels: those whose every sample's primary
    ray meets the floor."""
    w, h, spp = 64, 48, 64
    cr = np.array([[0.0, -1000.5, -3.0, 1000.0], [0.0, 0.5, -3.0, 0.05]], F32)
    sm = np.zeros(2, rt3.MATERIAL)
    sm["kind"], sm["rgb"] = (rt3.MAT_LAMBERT, rt3.MAT_FLAT), ((0.6, 0.6, 0.6), (400.0, 400.0, 400.0))
    set_scene(rt3, renderer, cr, sm)
    cam = rt3.Camera().look_at(w, h, (0.0, 1.0, 1.0), (0.0, -0.5, -3.0), (0.0, 1.0, 0.0), 50.0, 4.0)
    par = lambda flag: rt3.make_params(w, h, spp=spp, max_depth=4, seed=2, flags=rt3.FLAG_VARIANCE | rt3.FLAG_BLACK_BACKGROUND | flag, t_min=0.001)      # noqa: E731
    first = renderer.intersect(renderer.camera_rays(cam.c, par(0)), 0.001)             # every sample's primary ray (sample-major)
    floor = ((first["kind"] == rt3.HIT_SPHERE) & (first["index"] == 0)).reshape(spp, h, w).all(axis=0)
    assert 1000 < floor.sum() < h * w                                                  # the pixels that see the lamp itself are left out: 400 or 0 there, either way
    var = {}
    for flag in (0, rt3.FLAG_LIGHT_SAMPLING):
        m, v = moments(rt3, renderer, cam, par(flag))
        var[flag] = v[floor].sum()
        assert m[floor].sum() > 0
    print("summed variance over %d floor pixels: plain %.4g, flagged %.4g, ratio %.1f" % (floor.sum(), var[0], var[32], var[0] / var[32]))
    assert var[32] < var[0]


# ------------------------------------------------------------------------------------------------ 6: routes agree
@pytest.mark.parametrize("n_faces,n_sph", [(0, 480), (900, 0), (1301, 707)])
def test_every_kernel_route_equals_the_unfiltered_kernel(rt3, renderer, n_faces, n_sph, monkeypatch):
    rng = np.random.default_rng(361 + n_faces + n_sph)
    rays, _ = soup(rt3, renderer, rng, n_faces, n_sph, 2048)
    assert renderer.light_table()[0].any()
    flag = rt3.FLAG_LIGHT_SAMPLING
    cam = rt3.main_camera(W, H)
    p = rt3.make_params(W, H, spp=2, max_depth=DEPTH, seed=9, flags=rt3.FLAG_GAMMA2 | flag, t_min=0.001)

    def call():
        rad = renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=5, flags=flag | rt3.FLAG_BLACK_BACKGROUND)
        st = renderer.stats()
        px = renderer.render_path(cam.c, p)
        return rad, px, renderer.accum_resolve(p), st, renderer.stats()

    ref = with_form(renderer, {"RT3_BRUTE": "1"}, monkeypatch, call)
    assert ref[3].mfma_instructions == 0 and ref[4].mfma_instructions == 0 and not np.isnan(ref[0]).any()
    plain = renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=5, flags=rt3.FLAG_BLACK_BACKGROUND)
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
    renderer.set_environment(E.random_cube(5, seed=46))                                # with a map set: the same forms, the miss reads the map
    ref = with_form(renderer, {"RT3_BRUTE": "1"}, monkeypatch, call)
    got = call()
    same_words(got[1], ref[1], "with a map: pixels")
    same_words(got[2], ref[2], "with a map: linear frame")
    same(got[0], ref[0], "with a map: radiance")


# ------------------------------------------------------------------------------------------------ 7: the defining property of rt3_radiance
@pytest.mark.parametrize("name,black", [("cornell4+spheres", True), ("cornell4+spheres", False), ("weekend+lamps", False)])
def test_radiance_ranges_and_shards_compose(rt3, renderer, name, black):
    kw, cam, lens, _ = scene(rt3, name.split("+lamps")[0])
    if name.endswith("+lamps"):
        kw = dict(kw, smats=kw["smats"].copy())
        kw["smats"]["kind"][3::7] = rt3.MAT_FLAT
    set_scene(rt3, renderer, **kw)
    assert renderer.light_table()[0].any()
    flag = rt3.FLAG_LIGHT_SAMPLING | (rt3.FLAG_BLACK_BACKGROUND if black else 0)
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
    same_words(renderer.render_path_range(cam.c, p, 1, 3), whole, "a range split into two calls")
    same_words(renderer.accum_resolve(p), linear, "... and its accumulation")
    # a shard: the frame's pixel indices as keys
    ps = [params_of(rt3, rt3.FLAG_GAMMA2 | flag, lens, tile_rows=4, tile_index=i, tile_count=3) for i in range(3)]
    q = ps[1]
    rows = rt3.rows_owned(q)
    assert 0 < rows < H
    skeys = np.concatenate([rt3.row_of_local(q, lr) * W + np.arange(W) for lr in range(rows)]).astype(np.uint32)
    stotal = np.zeros((rows * W, 3), F32)
    for s in range(SPP):
        rays = renderer.camera_rays(cam.c, q, s, 1)
        stotal = stotal + renderer.radiance(rays, keys=skeys, sample_begin=s, samples=1, max_depth=DEPTH, seed=SEED, flags=flag, t_min=0.001)[:, :3]
    tiles = [renderer.render_path(cam.c, t) for t in ps]
    renderer.render_path(cam.c, q)
    same(renderer.accum_resolve(q).reshape(-1, 4), np.concatenate([stotal / F32(SPP), np.zeros((rows * W, 1), F32)], axis=1), "shard")
    assert np.array_equal(rt3.deinterleave(tiles, ps, H, W), whole)
    renderer.render_path(cam.c, params_of(rt3, rt3.FLAG_GAMMA2 | (flag & rt3.FLAG_BLACK_BACKGROUND), lens))
    assert (renderer.accum_resolve(p) != linear).any()                                 # the flag does change this frame


# ------------------------------------------------------------------------------------------------ 8: state and errors
def test_state_and_refusals(rt3, renderer):
    L = rt3.lib()
    vp = C.c_void_p
    kw, cam, lens, _ = scene(rt3, "cornell4+spheres")
    flag = rt3.FLAG_LIGHT_SAMPLING
    p = params_of(rt3, rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND | flag, lens)
    out = np.zeros((H, W), np.uint32)
    set_scene(rt3, renderer, **kw)
    rays = renderer.camera_rays(cam.c, p, 0, 1)
    rad = np.zeros((len(rays), 4), F32)

    def render_rc(q):
        return L.rt3_render_path(renderer._ctx, C.byref(cam.c), C.byref(q), out.ctypes.data_as(vp))

    def radiance_rc(flags):
        rp = rt3.RADIANCE_PARAMS(DEPTH, SEED, flags, 0, 1, 0.001)
        return L.rt3_radiance(renderer._ctx, rays.ctypes.data_as(vp), None, len(rays), C.byref(rp), rad.ctypes.data_as(vp))

    # no scene: RT3_E_STATE
    set_scene(rt3, renderer)
    n = C.c_uint32(0)
    q8, c8 = np.zeros(8, np.uint32), np.zeros(8, np.uint64)
    assert render_rc(p) == E_STATE and radiance_rc(flag) == E_STATE
    assert L.rt3_debug_light_table(renderer._ctx, q8.ctypes.data_as(vp), c8.ctypes.data_as(vp), 8, C.byref(n)) == E_STATE
    set_scene(rt3, renderer, **kw)
    # flags that exclude it: RT3_E_ARG, the flag's own messages, before the older refusals (no map is set; the scene has spheres)
    assert render_rc(params_of(rt3, flag | rt3.FLAG_ENV_SAMPLING, lens)) == E_ARG
    assert b"RT3_FLAG_LIGHT_SAMPLING cannot be combined with RT3_FLAG_ENV_SAMPLING" in L.rt3_last_error(renderer._ctx)
    assert render_rc(params_of(rt3, flag | rt3.FLAG_REFERENCE_PRIMARY, lens)) == E_ARG
    assert b"RT3_FLAG_LIGHT_SAMPLING cannot be combined with RT3_FLAG_REFERENCE_PRIMARY" in L.rt3_last_error(renderer._ctx)
    assert radiance_rc(flag | rt3.FLAG_ENV_SAMPLING) == E_ARG
    assert b"RT3_FLAG_LIGHT_SAMPLING cannot be combined with RT3_FLAG_ENV_SAMPLING" in L.rt3_last_error(renderer._ctx)
    assert radiance_rc(flag | rt3.FLAG_REFERENCE_PRIMARY) == E_ARG
    with pytest.raises(rt3.Fatal, match="RT3_FLAG_LIGHT_SAMPLING is not available to the adaptive render"):
        renderer.render_adaptive(cam.c, rt3.make_params(W, H, spp=8, max_depth=DEPTH, seed=SEED, flags=flag, t_min=0.001), min_spp=2, step_spp=2)
    assert L.rt3_debug_light_table(renderer._ctx, q8.ctypes.data_as(vp), c8.ctypes.data_as(vp), 8, C.byref(n)) == E_ARG
    assert n.value == len(kw["faces"]) + len(kw["spheres"])
    assert radiance_rc(flag) == 0 and radiance_rc(flag | rt3.FLAG_BLACK_BACKGROUND) == 0
    # the AOV pass ignores the flag
    plain_p = params_of(rt3, rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND, lens)
    assert renderer.render_aov(cam.c, p).tobytes() == renderer.render_aov(cam.c, plain_p).tobytes()
    # the render; more casts than the plain one
    lit = renderer.render_path(cam.c, p)
    casts = renderer.stats().ray_casts
    plain = renderer.render_path(cam.c, plain_p)
    assert casts > renderer.stats().ray_casts and (lit != plain).any()
    # regroups and the environment calls leave the table and the frame; a scene upload of the same scene gives it again
    renderer.regroup()
    same_words(renderer.render_path(cam.c, p), lit, "after regroup")
    renderer.set_environment(E.random_cube(5, seed=47))
    same_words(renderer.render_path(cam.c, p), lit, "with a map, under a black background")
    renderer.clear_environment()
    set_scene(rt3, renderer, **kw)
    same_words(renderer.render_path(cam.c, p), lit, "the same scene again")
    # other materials: the table is rebuilt and the frame follows
    sm = kw["smats"].copy()
    sm["rgb"][sm["kind"] == rt3.MAT_FLAT] *= F32(3.0)
    renderer.set_spheres(kw["spheres"], sm)
    assert (renderer.render_path(cam.c, p) != lit).any()
    renderer.set_spheres(kw["spheres"], kw["smats"])
    # a progressive accumulation is untouched by a flagged rt3_radiance
    renderer.render_path_range(cam.c, p, 0, 2)
    renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=3, flags=flag)
    same_words(renderer.render_path_range(cam.c, p, 2, 2), lit, "continued across a flagged rt3_radiance")


def test_cli_light_sampling_gives_the_frame_of_the_api_render(rt3, renderer, tmp_path):
    w, h = 32, 18
    rc, out, err = run("-f", "ppm", "-W", str(w), "-H", str(h), "--scene", "cornell", "--spp", "4", "--depth", "6", "--seed", "9",
                       "--light-sampling", "--hdr", str(tmp_path / "lin.pfm"), str(tmp_path / "box.ppm"))
    assert rc == 0, err
    faces, verts, fm = rt3.scene_cornell(64)
    set_scene(rt3, renderer, faces=faces, verts=verts, fmats=fm)
    cam = rt3.Camera().update(w, h, 2.0, F32(w) / F32(h) * F32(2.0), 2.0)
    flags = rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND
    p = rt3.make_params(w, h, spp=4, max_depth=6, seed=9, flags=flags | rt3.FLAG_LIGHT_SAMPLING, t_min=0.001)
    frame = rt3.Frame(w, h)
    frame.data[:] = renderer.render_path(cam.c, p)
    assert (tmp_path / "box.ppm").read_bytes() == frame.ppm_bytes()
    assert (tmp_path / "lin.pfm").read_bytes() == rt3.pfm_bytes(renderer.accum_resolve(p)[..., :3])
    plain = renderer.render_path(cam.c, rt3.make_params(w, h, spp=4, max_depth=6, seed=9, flags=flags, t_min=0.001))
    assert (plain != frame.data).any()
