"""The kernels against tests/truth_ref.py, the float64 truth of Mode X's geometry and scattering laws.

Every other GPU test compares the kernels with the CPU oracle or with each other, all written by the same hand from the same formulas; these
compare them with the geometry itself: (a) rt3_intersect / rt3_occluded with a brute-force float64 nearest hit, (b) rt3_camera_rays with the
float64 camera ray and the documented key layout, (c) rt3_render_aov with the float64 hit and normal, (d) the Lambert scatter with the
cosine law, (e) the metal scatter with the mirror law, (f) the dielectric with Snell and Schlick, (g) the path loop over many bounces with
the closed form of an integrating sphere (also through rt3_radiance and RT3_FLAG_LIGHT_SAMPLING), (h) metal fuzz with its absorption law,
(i) a glass sphere with its enumerated path tree, (j) the sky and the RGBA8 pack.  Tolerances are the derived float32 error
bounds of truth_ref.py or statistical; rays the bounds cannot decide are left out and counted.  The same checks run against the oracle,
without a GPU, in tests/test_truth_ref.py, which also shows that each helper used here rejects the fault it guards against."""
import numpy as np
import pytest

import truth_cases as K
import truth_ref as T

pytestmark = pytest.mark.gpu

REGIME_IDS = ["s1_o0", "s1_o300", "s1000_o0", "s0.01_o30"]
LEVELS4 = {"RT3_LEVELS": "4", "RT3_NO_RESIDENT": "1"}


# ------------------------------------------------------------------------------------------------ the product as a source
def source(rt3):
    """The product's own pre-render: the stored normals are its own."""
    return (lambda a, b, c: rt3.pre_render_entity(rt3.create_triangle(a, b, c, (1.0, 1.0, 1.0)))), rt3.merge_entities


def upload(rt3, r, sc):
    if sc["faces"] is not None:
        fm = sc.get("fmats")
        r.set_mesh(sc["faces"], sc["verts"], None if fm is None else np.ascontiguousarray(fm).view(rt3.MATERIAL))
    else:
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    if sc["spheres"] is not None:
        sm = sc.get("smats")
        r.set_spheres(sc["spheres"], np.zeros(len(sc["spheres"]), rt3.MATERIAL) if sm is None else np.ascontiguousarray(sm).view(rt3.MATERIAL))
    else:
        r.set_spheres(np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))


def params(rt3, p):
    return rt3.make_params(**p.kwargs())


def render(rt3, r, sc, cam, p):
    upload(rt3, r, sc)
    return r.render_path(cam.struct(rt3.rt3_camera), params(rt3, p))


# ------------------------------------------------------------------------------------------------ (a) rt3_intersect / rt3_occluded
@pytest.mark.parametrize("regime", range(4), ids=REGIME_IDS)
@pytest.mark.parametrize("scene,env", [("spheres300", None), ("mixed64", None), ("mixed700", None), ("mixed700", LEVELS4)],
                         ids=["spheres300", "mixed64", "mixed700", "mixed700_levels4_tiled"])
def test_intersect_equals_the_float64_nearest_hit(rt3, renderer, scene, env, regime, monkeypatch):
    sc, o, d, cls, t_min, ref = K.hit_case(*source(rt3), scene, regime)
    upload(rt3, renderer, sc)
    rays = np.zeros(len(o), rt3.RAY)
    rays["origin"], rays["direction"], rays["t_max"] = o, d, ref["t_max"].astype(np.float32)
    if env:                                                          # the default form first: the switch must reach another kernel
        renderer.intersect(rays, t_min)
        default_filter_tests = renderer.stats().filter_tests
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    hits = renderer.intersect(rays, t_min)
    assert not env or renderer.stats().filter_tests != default_filter_tests
    occ = renderer.occluded(rays, t_min)
    st = renderer.stats()
    assert (hits["kind"] != rt3.HIT_INVALID).all() and (hits["_pad"] == 0).all()
    fig = K.check_hits(ref, hits["kind"], hits["index"], hits["t"], occ)
    print("kernel", scene, "levels4" if env else "", K.REGIMES[regime], fig)
    assert st.filter_tests > 0 and st.mfma_instructions > 0          # a matrix-filter form ran
    assert fig["hits"] > 1000 and (ref["kind"] == T.NONE).sum() > 500
    assert ((cls == 2) & (ref["kind"] == T.SPHERE) & ~ref["ambiguous"]).sum() > 300           # rays from inside a sphere: the far root


# ------------------------------------------------------------------------------------------------ (b) rt3_camera_rays
def exported_hash(rt3):
    L = rt3.lib()
    return lambda words: np.array([L.rt3_hash_u32(int(w)) for w in words], np.uint32)


@pytest.mark.parametrize("w,h,spp,lens,tile", K.CAMERA_CASES)
def test_camera_rays_equal_the_float64_camera_ray(rt3, renderer, w, h, spp, lens, tile):
    cam, p = K.camera_case(w, h, spp, lens, tile)
    exp = K.expected_camera_rays(cam, p, exported_hash(rt3))
    rays = renderer.camera_rays(cam.struct(rt3.rt3_camera), params(rt3, p))
    assert np.isposinf(rays["t_max"]).all() and (rays["_pad"] == 0).all()
    fig = K.check_camera_rays(cam, p, rays["origin"], rays["direction"], exp)
    print("kernel camera rays", (w, h, spp, lens, tile), fig)
    assert fig["compared"] == len(T.owned_rows(p)) * w * spp


def test_exported_random_float_is_the_documented_u01(rt3):
    L = rt3.lib()
    words = np.concatenate([np.random.default_rng(5).integers(0, 2 ** 32, 500, dtype=np.uint64).astype(np.uint32),
                            np.array([0, 1, 0x7FFFFF, 0x800000, 0xFFFFFFFF], np.uint32)])
    assert np.array_equal(np.array([L.rt3_random_float(int(x)) for x in words], np.float64), T.u01(words))


# ------------------------------------------------------------------------------------------------ (c) rt3_render_aov
@pytest.mark.parametrize("regime", range(4), ids=REGIME_IDS)
def test_aov_equals_the_float64_first_hit(rt3, renderer, regime):
    """The cap on ambiguous pixels is 2 %, twice (a)'s: every ray of this camera crosses the box, where half of (a)'s rays start in it."""
    sc, cam, p = K.aov_case(*source(rt3), regime)
    upload(rt3, renderer, sc)
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    rays = renderer.camera_rays(c, pp)
    print("kernel aov camera rays", K.REGIMES[regime], K.check_camera_rays(cam, p, rays["origin"], rays["direction"], K.expected_camera_rays(cam, p)))
    ref = K.aov_truth(sc, p, rays["origin"], rays["direction"])
    aov = renderer.render_aov(c, pp).reshape(-1)
    depth = np.where(aov["kind"] == rt3.HIT_NONE, np.inf, aov["depth"].astype(np.float64))
    fig = K.check_hits(ref, aov["kind"], aov["index"], depth, cap=0.02)
    hit = ref["kind"] != T.NONE
    ok = ~ref["ambiguous"]
    assert np.array_equal(aov["coverage"][ok], hit[ok].astype(np.float32)) and np.isposinf(aov["depth"][ok & ~hit]).all()
    assert (aov["normal"][ok & ~hit] == 0).all()
    nfig = K.check_normals(ref, aov["normal"], rays["direction"])
    print("kernel aov", K.REGIMES[regime], fig, "normals", nfig)
    assert (ref["kind"][ok] == T.FACE).sum() > 200 and (ref["kind"][ok] == T.SPHERE).sum() > 400 and (~hit[ok]).sum() > 500


# ------------------------------------------------------------------------------------------------ (d) the cosine law
@pytest.mark.parametrize("ground", ["sphere", "triangles"])
def test_lambert_scatter_obeys_the_cosine_law(rt3, renderer, ground):
    """Measured on the MI355X: the worst pixel of 144 is 2.7 sigma off in both variants (the oracle's figure, as the frames are its frames)."""
    sc = K.cosine_scene(ground, *source(rt3))
    cam, p = K.cosine_camera()
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    upload(rt3, renderer, sc)
    rays = renderer.camera_rays(c, pp)                                # each pixel's own samples
    F = K.cosine_expectation(sc, rays["origin"], rays["direction"], p.spp)
    renderer.render_path(c, pp)
    mean = renderer.accum_resolve(pp)                                 # the linear frame: no 8-bit quantisation
    assert np.array_equal(mean[..., 0], mean[..., 1]) and np.array_equal(mean[..., 0], mean[..., 2]) and (mean[..., 3] == 0).all()
    fig = K.check_cosine(mean[..., 0].reshape(-1), F, K.COSINE["albedo"] * K.COSINE["c"], p.spp)
    print("kernel cosine law,", ground, fig)


# ------------------------------------------------------------------------------------------------ (e) the mirror law
def test_metal_scatter_obeys_the_mirror_law(rt3, renderer):
    """The reference's own share of skipped pixels: 9 of 2304 (0.4 %)."""
    sc, cam, p = K.mirror_scene()
    ex = K.specular_frame(sc, cam, p)
    px = render(rt3, renderer, sc, cam, p)
    K.check_frame(px, ex["allowed"], ex["skip"])
    seen = ex["specular"] & ~ex["skip"]
    print("kernel mirror: %d pixels compared, %d skipped, %d through the mirror" % ((~ex["skip"]).sum(), ex["skip"].sum(), seen.sum()))
    assert seen.sum() > 1000 and (ex["allowed"][0][seen] != K.BLACK).sum() > 300


# ------------------------------------------------------------------------------------------------ (f) Snell and Schlick
@pytest.mark.parametrize("back", [False, True], ids=["front", "back"])
def test_dielectric_obeys_snell_and_schlick(rt3, renderer, back):
    """The reference's own share of skipped pixels: front 14 of 2304 (0.6 %), back 7 of 2304 (0.3 %)."""
    sc, cam, p = K.glass_scene(*source(rt3), back)
    ex = K.specular_frame(sc, cam, p)
    px = render(rt3, renderer, sc, cam, p)
    fig = K.check_glass(px, ex, need_tir=back)
    print("kernel glass,", "back" if back else "front", fig)
    assert fig["counted"] > 500


# ------------------------------------------------------------------------------------------------ (g) the integrating sphere
def first_hits_meet_the_wall(rt3, renderer, c, pp, spp, step=256):
    """rt3_intersect over rt3_camera_rays, every sample of every pixel: the wall and nothing else."""
    for s in range(0, spp, step):
        first = renderer.intersect(renderer.camera_rays(c, pp, s, min(step, spp - s)), 0.001)
        if not K.all_meet_the_wall(first["kind"], first["index"]):
            return False
    return True


@pytest.mark.parametrize("case", range(len(K.INTEGRATING)), ids=K.INTEGRATING_IDS)
def test_multi_bounce_transport_in_the_integrating_sphere(rt3, renderer, case):
    """Mean, every pixel and ray_casts per sample of a depth-D render against the closed form (truth_ref.integrating_sphere), 6 sigma with
    the exact sigma.  Figures: DESIGN.md 5.2k."""
    r, R, a, E, D = K.INTEGRATING[case]
    sc = K.integrating_scene(r, R, a, E)
    cam, p = K.integrating_camera(r, R, D)
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    upload(rt3, renderer, sc)
    assert first_hits_meet_the_wall(rt3, renderer, c, pp, p.spp)
    renderer.render_path(c, pp)
    casts = renderer.stats().ray_casts
    mean = renderer.accum_resolve(pp)
    assert np.array_equal(mean[..., 0], mean[..., 1]) and np.array_equal(mean[..., 0], mean[..., 2])
    fig = K.check_integrating(T.integrating_sphere(r, R, a, E, D), mean[..., 0], p.spp, casts / (p.width * p.height * p.spp), D)
    print("kernel integrating sphere", K.INTEGRATING_IDS[case], fig)


def test_radiance_in_the_integrating_sphere(rt3, renderer):
    """rt3_radiance along 2^14 rays that start in the gap and meet the wall, 64 samples each, depth 8: the same mean, the same bound."""
    r, R, a, E, D = K.INTEGRATING[2]
    upload(rt3, renderer, K.integrating_scene(r, R, a, E))
    o, d = K.integrating_rays(r, R, 1 << 14)
    rays = np.zeros(len(o), rt3.RAY)
    rays["origin"], rays["direction"], rays["t_max"] = o, d, np.inf
    first = renderer.intersect(rays, 0.001)
    assert K.all_meet_the_wall(first["kind"], first["index"])
    rad = renderer.radiance(rays, samples=64, max_depth=D, seed=13, flags=rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)
    assert np.array_equal(rad[:, 0], rad[:, 1]) and np.array_equal(rad[:, 0], rad[:, 2])
    fig = K.check_integrating(T.integrating_sphere(r, R, a, E, D), rad[:, 0], 64, each=False)
    print("kernel rt3_radiance in the integrating sphere", fig)


@pytest.mark.parametrize("depth", [2, 12])
def test_light_sampling_in_the_integrating_sphere(rt3, renderer, depth):
    """RT3_FLAG_LIGHT_SAMPLING, which the oracle does not implement, against the same closed form: a shadow ray at every wall hit gives a
    sample within [0, light_sample_range], so its sigma is at most half that range (the furnace test's derivation); 6 half-ranges /
    sqrt(samples).  The measured z in units of the exact plain sigma is printed beside it."""
    r, R, a, E, _ = K.INTEGRATING[4]
    w, h, spp = 64, 48, 1024
    upload(rt3, renderer, K.integrating_scene(r, R, a, E))
    cam, p = K.integrating_camera(r, R, depth, size=(w, h, spp), seed=9, flags=K.FLAG_BLACK | rt3.FLAG_LIGHT_SAMPLING)
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    assert first_hits_meet_the_wall(rt3, renderer, c, pp, spp)
    renderer.render_path(c, pp)
    mean = renderer.accum_resolve(pp)[..., 0].astype(np.float64).mean()
    law = T.integrating_sphere(r, R, a, E, depth)
    fig = K.check_range_mean(mean, law["mean"], 0.0, K.light_sample_range(r, R, a, E, depth), w * h * spp)
    print("kernel light sampling in the integrating sphere, depth", depth, fig, "z in plain sigmas %.2f" % (
        (mean - law["mean"]) / (law["sigma"] / np.sqrt(w * h * spp))))


def test_light_sampling_leaves_the_pixels_on_the_emitter(rt3, renderer):
    """The camera turned to the emitter: a pixel whose every primary ray meets it shows E exactly, flag or not."""
    r, R, a, E, D = K.INTEGRATING[4]
    upload(rt3, renderer, K.integrating_scene(r, R, a, E))
    cam, p = K.integrating_camera(r, R, D, size=(64, 48, 16), flags=K.FLAG_BLACK | rt3.FLAG_LIGHT_SAMPLING, inward=True)
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    first = renderer.intersect(renderer.camera_rays(c, pp), 0.001)
    on = ((first["kind"] == rt3.HIT_SPHERE) & (first["index"] == K.EMITTER)).reshape(p.spp, -1).all(axis=0)
    assert on.sum() > 500 and (~on).sum() > 500
    renderer.render_path(c, pp)
    mean = renderer.accum_resolve(pp).reshape(-1, 4)
    assert (mean[on, :3] == np.float32(E)).all() and (mean[~on, :3] != np.float32(E)).any()


# ------------------------------------------------------------------------------------------------ (h) metal fuzz
_fuzz_cos = {}


def fuzz_cosines(rt3, ground):
    """The float64 cosines of incidence of every sample, once per ground: they do not depend on f."""
    if ground not in _fuzz_cos:
        cam, p = K.fuzz_camera(ground)
        o, d, _ = K.expected_camera_rays(cam, p)
        _fuzz_cos[ground] = K.fuzz_cosines(K.fuzz_scene(ground, 1.0, *source(rt3)), o, d, p.spp)
    return _fuzz_cos[ground]


@pytest.mark.parametrize("f", K.FUZZ["fs"])
@pytest.mark.parametrize("ground", ["triangles", "sphere"])
def test_metal_fuzz_obeys_the_absorption_law(rt3, renderer, ground, f):
    sc = K.fuzz_scene(ground, f, *source(rt3))
    cam, p = K.fuzz_camera(ground)
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    upload(rt3, renderer, sc)
    renderer.render_path(c, pp)
    mean = renderer.accum_resolve(pp)
    assert (mean[..., 3] == 0).all()
    fig = K.check_fuzz(mean[..., :3].reshape(-1, 3), fuzz_cosines(rt3, ground), f)
    print("kernel fuzz", ground, f, fig)
    assert fig["statistical"] > 100 and (f == 1.0 or fig["exact"] > 100)


# ------------------------------------------------------------------------------------------------ (i) a glass sphere
def test_glass_sphere_follows_the_path_tree(rt3, renderer):
    """The reference's own share of skipped pixels: 34 of 2304 (1.5 %)."""
    sc, cam, p = K.glass_sphere_scene()
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    upload(rt3, renderer, sc)
    rays = renderer.camera_rays(c, pp)
    K.check_camera_rays(cam, p, rays["origin"], rays["direction"], K.expected_camera_rays(cam, p))
    tree = K.glass_tree(sc, p, rays["origin"], rays["direction"])      # behind the rays the kernel really traced
    fig = K.check_glass_tree(renderer.render_path(c, pp), tree)
    print("kernel glass sphere", fig)
    assert fig["through_glass"] >= 500 and fig["reflected"] >= 20 and fig["counted"] >= 100


# ------------------------------------------------------------------------------------------------ (j) sky and pack
def test_sky(rt3, renderer):
    sc, cam, p = K.sky_scene()
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    upload(rt3, renderer, sc)
    renderer.render_path(c, pp)
    assert renderer.stats().ray_casts == p.width * p.height
    fig = K.check_sky(renderer.accum_resolve(pp)[..., :3], cam, p)
    print("kernel sky", fig)
    assert fig["t_range"][0] < 0.4 and fig["t_range"][1] > 0.8       # below and above the horizon


@pytest.mark.parametrize("gamma2", [False, True], ids=["linear", "gamma2"])
def test_pack(rt3, renderer, gamma2):
    sc, cam, p = K.pack_scene(gamma2)
    rgb, amb, hit = K.pack_expectation(sc, cam, p)
    assert not amb.any()
    c, pp = cam.struct(rt3.rt3_camera), params(rt3, p)
    upload(rt3, renderer, sc)
    px = renderer.render_path(c, pp)
    linear = renderer.accum_resolve(pp)                                # of the same call
    assert np.array_equal(linear[..., :3].reshape(-1, 3), rgb), "the linear frame is the material's colour, bit for bit"
    fig = K.check_pack(px, linear[..., :3], gamma2)
    print("kernel pack", "gamma2" if gamma2 else "linear", fig)
    assert fig["ties"] == 0 and fig["bytes_seen"] == 256 and fig["clamped"] > 20 and fig["zeros"] > 1000
