"""The kernels against tests/truth_ref.py, the float64 truth of Mode X's geometry and scattering laws.

Every other GPU test compares the kernels with the CPU oracle or with each other, all written by the same hand from the same formulas; these
compare them with the geometry itself: (a) rt3_intersect / rt3_occluded with a brute-force float64 nearest hit, (b) rt3_camera_rays with the
float64 camera ray and the documented key layout, (c) rt3_render_aov with the float64 hit and normal, (d) the Lambert scatter with the
cosine law, (e) the metal scatter with the mirror law, (f) the dielectric with Snell and Schlick.  Tolerances are the derived float32 error
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
