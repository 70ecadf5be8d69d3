"""tests/truth_ref.py, the float64 truth of Mode X's geometry and scattering laws, without a GPU.

1. Known answers of the reference itself.  2. Mutants: each comparison helper of tests/truth_cases.py rejects a deliberately wrong
answer set built from the reference's own output, so the suite is known to notice that fault.  3. The CPU oracle against truth: the checks
of tests/test_gpu_truth.py with oracle_nearest / oracle_render_path in the kernels' place (the kernels equal the oracle bit for bit, so what
holds here is what they can pass).  The oracle exports neither camera rays nor AOVs; (b) and (c) have their self-checks here and their
comparison on the GPU.  4.-6. The same three steps for the closed forms and enumerable laws behind multi-bounce transport (the integrating
sphere), metal fuzz, a glass sphere's path tree, the sky and the RGBA8 pack.

Figures of this file's run (rays or pixels compared / skipped as ambiguous / largest error over bound or |z|): see DESIGN.md 5.2k."""
import json
import os

import numpy as np
import pytest

import truth_cases as K
import truth_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ====================================================================================================================== 1. known answers
UNIT_SPHERE = np.array([[0.0, 0.0, 0.0, 1.0]], np.float32)
TRI_V = np.array([[0, 0, 0, 0], [3, 0, 0, 0], [0, 3, 0, 0]], np.float32)
TRI_F = np.array([[0, 1, 2]])


def one(rec, i=0):
    return int(rec["kind"][i]), int(rec["index"][i]), float(rec["t"][i]), bool(rec["ambiguous"][i])


def test_axis_ray_against_the_unit_sphere_from_outside_and_inside():
    rec = T.nearest_hit([[0, 0, -3], [0, 0, 0], [0, 0, 3]], [[0, 0, 1]] * 3, 0.001, np.inf, UNIT_SPHERE)
    assert one(rec, 0) == (T.SPHERE, 0, 2.0, False)                  # the near root
    assert one(rec, 1) == (T.SPHERE, 0, 1.0, False)                  # from the centre: the far root
    assert one(rec, 2)[0] == T.NONE and np.isposinf(rec["t"][2]) and rec["index"][2] == T.NO_INDEX     # behind the ray
    assert np.array_equal(rec["normal"][0], [0, 0, -1])
    assert np.array_equal(rec["normal"][1], [0, 0, -1])              # the outward normal (0, 0, 1) turned to face the ray
    assert 0 < rec["t_bound"][0] < 1e-5


def test_ray_through_the_centroid_a_vertex_and_an_edge():
    o = [[1, 1, 5], [0, 0, 5], [1.5, 0, 5], [1, 1, -5]]
    d = [[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, 1]]
    rec = T.nearest_hit(o, d, 0.001, np.inf, None, TRI_F, TRI_V)
    assert one(rec, 0) == (T.FACE, 0, 5.0, False)
    assert np.array_equal(rec["normal"][0], [0, 0, 1]) and np.array_equal(rec["normal"][3], [0, 0, -1])      # either side faces its ray
    assert rec["ambiguous"][1] and rec["ambiguous"][2]               # a vertex and an edge: only the margin can say
    assert one(rec, 3) == (T.FACE, 0, 5.0, False)


def test_t_max_exactly_at_the_hit_is_a_miss_and_ambiguous():
    rec = T.nearest_hit([[1, 1, 5]] * 3, [[0, 0, -1]] * 3, 0.001, [5.0, 5.5, 4.5], None, TRI_F, TRI_V)
    assert one(rec, 0) == (T.NONE, T.NO_INDEX, np.inf, True)
    assert one(rec, 1) == (T.FACE, 0, 5.0, False)
    assert one(rec, 2) == (T.NONE, T.NO_INDEX, np.inf, False)
    rec = T.nearest_hit([[0, 0, -3]] * 2, [[0, 0, 1]] * 2, 0.001, [2.0, 2.5], UNIT_SPHERE)
    assert one(rec, 0) == (T.NONE, T.NO_INDEX, np.inf, True) and one(rec, 1) == (T.SPHERE, 0, 2.0, False)


def test_faces_win_ties_and_the_earlier_index_wins():
    sph = np.array([[0, 0, -1, 1], [0, 0, -1, 1]], np.float32)         # both spheres touch z = 0 from below at the origin ... a ray down x = y = 0.5
    v = np.concatenate([TRI_V, TRI_V])
    f = np.array([[0, 1, 2], [3, 4, 5]])
    rec = T.nearest_hit([[0.5, 0.5, 5]], [[0, 0, -1]], 0.001, np.inf, sph, f, v)
    assert one(rec)[:3] == (T.FACE, 0, 5.0) and rec["ambiguous"][0]  # the coincident second face is a runner-up at gap 0
    rec = T.nearest_hit([[0.0, 0.0, -5]], [[0, 0, 1]], 0.001, np.inf, sph)
    assert one(rec)[:3] == (T.SPHERE, 0, 3.0)


def test_a_ray_that_starts_on_a_surface_leaves_it():
    o = np.array([[0, 0, 1], [1, 1, 0]], np.float64)
    rec = T.nearest_hit(o[:1], [[0, 0, 1]], 0.001, np.inf, UNIT_SPHERE)
    assert one(rec) == (T.NONE, T.NO_INDEX, np.inf, False)           # the root at t = 0 is 0.001 below t_min, far above its bound
    rec = T.nearest_hit(o[:1], [[0, 0, -1]], 0.001, np.inf, UNIT_SPHERE)
    assert one(rec) == (T.SPHERE, 0, 2.0, False)                     # inwards: the far root
    rec = T.nearest_hit(o[1:], [[0, 0, 1]], 0.001, np.inf, None, TRI_F, TRI_V)
    assert one(rec) == (T.NONE, T.NO_INDEX, np.inf, False)
    rec = T.nearest_hit(o[1:], [[0, 0, 1]], 0.0, np.inf, None, TRI_F, TRI_V)
    assert rec["ambiguous"][0]                                       # t = t_min = 0 exactly


def test_snell_at_normal_incidence_at_30_degrees_and_at_the_critical_angle():
    n = np.array([0.0, 0.0, 1.0])
    out, total = T.refract(np.array([[0.0, 0.0, -1.0]]), n, 1.0 / 1.5)
    assert np.allclose(out, [[0, 0, -1]], atol=1e-15) and not total[0]
    a = np.radians(30.0)
    out, total = T.refract(np.array([[np.sin(a), 0.0, -np.cos(a)]]), n, 1.0 / 1.5)
    assert abs(out[0, 0] - np.sin(a) / 1.5) < 1e-15 and abs(np.linalg.norm(out[0]) - 1.0) < 1e-15 and out[0, 2] < 0
    crit = np.arcsin(1.0 / 1.5)
    d = lambda x: np.array([[np.sin(x), 0.0, -np.cos(x)]])           # noqa: E731
    out, total = T.refract(d(crit - 1e-9), n, 1.5)
    assert not total[0] and abs(out[0, 2]) < 1e-4 and out[0, 0] > 0.99999        # grazes the surface
    out, total = T.refract(d(crit + 1e-9), n, 1.5)
    assert total[0]
    assert np.allclose(T.reflect(d(a), n), [[np.sin(a), 0.0, np.cos(a)]], atol=1e-15)


def test_schlick_at_0_and_90_degrees():
    assert abs(T.schlick(1.0, 1.0 / 1.5) - 0.04) < 1e-15 and abs(T.schlick(1.0, 1.5) - 0.04) < 1e-15
    assert T.schlick(0.0, 1.5) == 1.0
    assert 0.04 < T.schlick(np.cos(np.radians(60.0)), 1.0 / 1.5) < 0.1


def test_form_factor_straight_below_and_by_quadrature():
    n = np.array([[0.0, 1.0, 0.0]])
    assert abs(T.form_factor_sphere([[0.0, 0.0, 0.0]], n, (0.0, 2.0, 0.0), 1.0)[0] - 0.25) < 1e-15
    with pytest.raises(AssertionError):
        T.form_factor_sphere([[3.0, 0.0, 0.0]], n, (0.0, 0.5, 0.0), 1.0)       # the sphere dips below the horizon
    # Nusselt's analogue by brute force: the share of the unit disc whose lifted direction meets the sphere (midpoint rule, 1200^2 cells)
    p, c, r = np.array([0.7, 0.0, -0.4]), np.array([0.0, 2.0, 0.0]), 1.0
    g = (np.arange(1200) + 0.5) / 600.0 - 1.0
    x, z = np.meshgrid(g, g)
    inside = x * x + z * z < 1.0
    d = np.stack([x, np.sqrt(np.maximum(1.0 - x * x - z * z, 0.0)), z], axis=-1)
    oc = c - p
    h = d @ oc
    hit = inside & (h > 0) & (h * h - (oc @ oc - r * r) > 0)
    assert abs(hit.sum() / inside.sum() - T.form_factor_sphere(p[None], n, c, r)[0]) < 1e-3


def test_camera_ray_pinhole_and_thin_lens():
    cam = K.Cam((0, 0, 0), (4, 0, 0), (0, 2, 0), (-2, -1, -1))
    p = K.Params(5, 3)
    o, d, ln = T.camera_ray(cam, p, [2, 0, 4], [1, 0, 2])
    assert np.array_equal(o, np.zeros((3, 3))) and np.array_equal(d[0], [0, 0, -1]) and ln[0] == 1.0
    assert np.allclose(d[1] * ln[1], [-2, 1, -1]) and np.allclose(d[2] * ln[2], [2, -1, -1])      # row 0 is the top row
    o, d, ln = T.camera_ray(cam, p, [2], [1], jitter=[[0.5, -0.25]])
    assert np.allclose(d[0] * ln[0], [0.5, -0.25, -1.0])             # pixel units: 1 pixel = hor / (W - 1)
    p = K.Params(5, 3, lens_radius=0.5)
    o, d, ln = T.camera_ray(cam, p, [2, 2], [1, 1], lens_sample=[[1.0, 0.0], [0.25, 0.25]])
    assert np.allclose(o, [[0.5, 0, 0], [0, 0.25, 0]])               # r = R sqrt(xi2) along hor, then along ver
    assert np.allclose(o + d * ln[:, None], [[0, 0, -1]] * 2)        # through the same image-plane point


def test_hash_known_answers_and_sample_layout():
    kat = json.load(open(os.path.join(GOLDEN, "reference_pins.json")))["hash_kat"]
    for k, v in kat.items():
        assert int(T.hash_u32(np.uint32(int(k)))) == int(v, 16)
    assert T.u01(np.uint32(0xFFFFFFFF)) == 1.0 - 2.0 ** -23 and T.u01(np.uint32(0x12800000)) == 0.0
    jit, lens, base = T.camera_samples(64, 9, 11, np.full(9, 5), np.full(9, 7), np.arange(9))
    assert ((jit[:, 0] + 0.5) * 3 // 1 == np.arange(9) % 3).all() and ((jit[:, 1] + 0.5) * 3 // 1 == np.arange(9) // 3).all()      # strata
    assert len(set(base.tolist())) == 9 and (lens >= 0).all() and (lens < 1).all()
    jit, _, _ = T.camera_samples(64, 1, 11, [5], [7], [0])
    assert (jit == 0).all()
    assert np.array_equal(T.owned_rows(K.Params(8, 36, tile_rows=4, tile_index=1, tile_count=3)), [4, 5, 6, 7, 16, 17, 18, 19, 28, 29, 30, 31])


# ====================================================================================================================== shared oracle answers
def make_triangle(oracle):
    return lambda a, b, c: oracle.prerender_triangle(a, b, c, (1.0, 1.0, 1.0))


def oracle_hits(oracle, o, d, t_min, t_max, sc):
    """oracle_nearest per ray with the t < t_max cut: (kind, index, t)."""
    kind, index, t = np.zeros(len(o), np.uint32), np.full(len(o), T.NO_INDEX, np.uint32), np.full(len(o), np.inf)
    for i in range(len(o)):
        k, tt, j = oracle.nearest(o[i], d[i], sc["spheres"], sc["faces"], sc["verts"], tmin=t_min)
        if k and np.float32(tt) < t_max[i]:
            kind[i], index[i], t[i] = k, j, tt
    return kind, index, t


def hit_case(oracle, scene, regime):
    return K.hit_case(make_triangle(oracle), oracle.merge, scene, regime)


@pytest.fixture(scope="module")
def mixed64(oracle):
    """The 64 + 64 scene at (scale 1, offset 300) with the oracle's answers: the mutants start from it."""
    sc, o, d, cls, t_min, ref = hit_case(oracle, "mixed64", 1)
    kind, index, t = oracle_hits(oracle, o, d, t_min, ref["t_max"].astype(np.float32), sc)
    return dict(sc=sc, o=o, d=d, cls=cls, t_min=t_min, ref=ref, kind=kind, index=index, t=t)


def render(oracle, sc, cam, p, want_sum=False, threads=8):
    mat = lambda m: None if m is None else np.ascontiguousarray(m).view(oracle.MATERIAL)      # noqa: E731
    return oracle.render_path(cam.struct(oracle.Camera), oracle.make_params(**p.kwargs()), spheres=sc["spheres"], smats=mat(sc["smats"]),
                              faces=sc["faces"], verts=sc["verts"], fmats=mat(sc["fmats"]), want_sum=want_sum, threads=threads)


# ====================================================================================================================== 2. mutants
def test_mutant_far_root_is_rejected(mixed64):
    m, ref = mixed64, mixed64["ref"]
    K.check_hits(ref, m["kind"], m["index"], m["t"])                 # the unmutated answers pass
    sel = (ref["kind"] == T.SPHERE) & (m["cls"] == 0)                # seen from outside: the near root is the answer
    c = m["sc"]["spheres"][ref["index"][sel]].astype(np.float64)
    h = ((c[:, :3] - m["o"][sel]) * m["d"][sel].astype(np.float64)).sum(axis=1)
    t = m["t"].copy()
    t[sel] = 2.0 * h - ref["t"][sel]                                 # the other root of t^2 - 2 h t + c
    assert sel.sum() > 100
    with pytest.raises(AssertionError, match="error_bound_t"):
        K.check_hits(ref, m["kind"], m["index"], t)


def test_mutant_plane_formula_with_the_wrong_sign_is_rejected(mixed64):
    m, ref = mixed64, mixed64["ref"]
    sel = ref["kind"] == T.FACE
    f = m["sc"]["faces"][ref["index"][sel]]
    p1 = m["sc"]["verts"][f["v1"], :3].astype(np.float64)
    n, o, d = ref["normal"][sel], m["o"][sel].astype(np.float64), m["d"][sel].astype(np.float64)
    t = m["t"].copy()
    t[sel] = ((n * o).sum(axis=1) + (n * p1).sum(axis=1)) / (n * d).sum(axis=1)      # (n.o + n.p1) / (n.d): right only for o = 0
    assert sel.sum() > 100
    with pytest.raises(AssertionError):
        K.check_hits(ref, m["kind"], m["index"], t)


def test_mutant_unflipped_normal_is_rejected(mixed64):
    m, ref = mixed64, mixed64["ref"]
    good = K.shading_normals(ref, m["o"], m["d"], m["t"], m["sc"]["spheres"], m["sc"]["faces"])
    fig = K.check_normals(ref, good, m["d"])
    print("oracle normals (documented float32 form):", fig)
    assert fig["compared"] > 1500
    outward = good.copy()
    s = ref["kind"] == T.SPHERE
    c = m["sc"]["spheres"][ref["index"][s]]
    p = m["o"][s] + m["t"][s, None] * m["d"][s]
    outward[s] = ((p - c[:, :3]) / c[:, 3:4]).astype(np.float32)      # (p - C) / r as it stands: inside a sphere it faces away
    with pytest.raises(AssertionError, match="face away"):
        K.check_normals(ref, outward, m["d"])
    stored = good.copy()
    f = ref["kind"] == T.FACE
    stored[f] = m["sc"]["faces"]["normal"][ref["index"][f]]           # the stored face normal as it stands
    with pytest.raises(AssertionError, match="face away"):
        K.check_normals(ref, stored, m["d"])


def test_mutant_wrong_primitive_and_wrong_miss_are_rejected(mixed64):
    m, ref = mixed64, mixed64["ref"]
    index = m["index"].copy()
    i = np.nonzero(~ref["ambiguous"] & (ref["kind"] == T.SPHERE))[0][0]
    index[i] ^= 1
    with pytest.raises(AssertionError, match="another primitive"):
        K.check_hits(ref, m["kind"], index, m["t"])
    occ = (m["kind"] != 0).astype(np.uint32)
    K.check_hits(ref, m["kind"], m["index"], m["t"], occ)
    occ[i] = 0
    with pytest.raises(AssertionError, match="occlusion"):
        K.check_hits(ref, m["kind"], m["index"], m["t"], occ)


@pytest.fixture(scope="module")
def cosine_sphere(oracle):
    sc = K.cosine_scene("sphere")
    cam, p = K.cosine_camera()
    o, d, _ = K.expected_camera_rays(cam, p)
    return sc, cam, p, o, d, K.cosine_expectation(sc, o, d, p.spp)


def test_mutant_uniform_hemisphere_is_rejected(cosine_sphere):
    sc, cam, p, o, d, F = cosine_sphere
    ac = K.COSINE["albedo"] * K.COSINE["c"]
    K.check_cosine(ac * F, F, ac, p.spp)
    uniform = K.uniform_hemisphere_fraction(sc, o, d, p.spp)
    with pytest.raises(AssertionError, match="sigma"):
        K.check_cosine(ac * uniform, F, ac, p.spp)                   # a noise-free frame of a uniformly sampled hemisphere
    sigma = ac * np.sqrt(F * (1 - F) / p.spp)
    z = np.abs(ac * uniform - ac * F) / sigma
    assert z.max() > 10.0 and z.min() > 4.0                          # 4 to 17 sigma away, pixel by pixel


def test_mutant_reflection_with_the_wrong_sign_is_rejected():
    sc, cam, p = K.mirror_scene()
    ex = K.specular_frame(sc, cam, p)
    K.check_frame(ex["allowed"][0], ex["allowed"], ex["skip"])
    wrong = K.specular_frame(sc, cam, p, mutate="reflect_sign")
    with pytest.raises(AssertionError, match="another colour"):
        K.check_frame(wrong["allowed"][0], ex["allowed"], ex["skip"])


@pytest.mark.parametrize("back", [False, True], ids=["front", "back"])
def test_mutant_inverted_refraction_ratio_is_rejected(oracle, back):
    sc, cam, p = K.glass_scene(make_triangle(oracle), oracle.merge, back)
    ex = K.specular_frame(sc, cam, p)
    wrong = K.specular_frame(sc, cam, p, mutate="ri_inverted")
    rng = np.random.default_rng(1)
    show_reflected = rng.random(len(ex["R"])) < wrong["R"]            # a frame that follows the wrong law faithfully
    frame = np.where(show_reflected, wrong["allowed"][0], wrong["allowed"][1])
    with pytest.raises(AssertionError):
        K.check_glass(frame, ex)
    good = np.where(rng.random(len(ex["R"])) < ex["R"], ex["allowed"][0], ex["allowed"][1])
    K.check_glass(good, ex, need_tir=back)


# ====================================================================================================================== 3. the oracle against truth
@pytest.mark.parametrize("regime", range(4), ids=["s1_o0", "s1_o300", "s1000_o0", "s0.01_o30"])
@pytest.mark.parametrize("scene", list(K.SCENES))
def test_oracle_nearest_hit_equals_truth(oracle, scene, regime):
    sc, o, d, cls, t_min, ref = hit_case(oracle, scene, regime)
    kind, index, t = oracle_hits(oracle, o, d, t_min, ref["t_max"].astype(np.float32), sc)
    fig = K.check_hits(ref, kind, index, t)
    print("oracle", scene, K.REGIMES[regime], fig)
    assert fig["hits"] > 1000 and (ref["kind"] == T.NONE).sum() > 500                         # not vacuous
    far = (cls == 2) & (ref["kind"] == T.SPHERE) & ~ref["ambiguous"]
    assert far.sum() > 300                                           # rays from inside a sphere


@pytest.mark.parametrize("ground", ["sphere", "triangles"])
def test_oracle_cosine_law(oracle, cosine_sphere, ground):
    if ground == "sphere":
        sc, cam, p, o, d, F = cosine_sphere
    else:
        sc = K.cosine_scene(ground, make_triangle(oracle), oracle.merge)
        cam, p = K.cosine_camera()
        o, d, _ = K.expected_camera_rays(cam, p)
        F = K.cosine_expectation(sc, o, d, p.spp)
    _, total, _ = render(oracle, sc, cam, p, want_sum=True)
    assert np.array_equal(total[..., 0], total[..., 1]) and np.array_equal(total[..., 0], total[..., 2])
    fig = K.check_cosine(total[..., 0].reshape(-1).astype(np.float64) / p.spp, F, K.COSINE["albedo"] * K.COSINE["c"], p.spp)
    print("oracle cosine law,", ground, fig, "F in [%.3f, %.3f]" % (F.min(), F.max()))


def test_oracle_mirror_law(oracle):
    """The reference's own share of skipped pixels: 9 of 2304 (0.4 %)."""
    sc, cam, p = K.mirror_scene()
    ex = K.specular_frame(sc, cam, p)
    px, _ = render(oracle, sc, cam, p)
    K.check_frame(px, ex["allowed"], ex["skip"])
    seen = ex["specular"] & ~ex["skip"]
    print("oracle mirror: %d pixels compared, %d skipped, %d through the mirror, %d of them on a target" % (
        (~ex["skip"]).sum(), ex["skip"].sum(), seen.sum(), (ex["allowed"][0][seen] != K.BLACK).sum()))
    assert seen.sum() > 1000 and (ex["allowed"][0][seen] != K.BLACK).sum() > 300 and len(np.unique(ex["allowed"][0][seen])) > 50


@pytest.mark.parametrize("back", [False, True], ids=["front", "back"])
def test_oracle_snell_and_schlick(oracle, back):
    """The reference's own share of skipped pixels: front 14 of 2304 (0.6 %), back 7 of 2304 (0.3 %)."""
    sc, cam, p = K.glass_scene(make_triangle(oracle), oracle.merge, back)
    ex = K.specular_frame(sc, cam, p)
    px, _ = render(oracle, sc, cam, p)
    fig = K.check_glass(px, ex, need_tir=back)
    print("oracle glass,", "back" if back else "front", fig)
    assert fig["counted"] > 500
    if not back:
        R = ex["R"][ex["specular"] & ~ex["skip"]]
        assert R.min() > 0.04 and R.max() < 0.5 and fig["total_reflection"] == 0


# ====================================================================================================================== 4. closed forms: known answers
def test_integrating_sphere_known_answers():
    law = T.integrating_sphere(1.0, 2.0, 0.8, 3.0, 2)
    assert law["F"] == 0.25 and abs(law["mean"] - 0.8 * 0.25 * 3.0) < 1e-15 and law["casts"] == 2.0          # D = 2: one bounce, a F E
    assert abs(law["second"] - (0.8 * 3.0) ** 2 * 0.25) < 1e-15
    law = T.integrating_sphere(1.0, 2.0, 0.8, 3.0, 3)
    assert abs(law["mean"] - 3.0 * 0.25 * (0.8 + 0.64 * 0.75)) < 1e-15 and law["casts"] == 2.75
    assert T.integrating_sphere(1.0, 2.0, 0.8, 3.0, 1)["mean"] == 0.0                                          # D = 1: the wall, and nothing else
    # D -> infinity: the geometric series a F E / (1 - a (1 - F)), and 1 + 1 / F casts
    law = T.integrating_sphere(1.0, 2.0, 0.8, 3.0, 400)
    assert abs(law["mean"] - 0.8 * 0.25 * 3.0 / (1.0 - 0.8 * 0.75)) < 1e-12 and abs(law["casts"] - 5.0) < 1e-12


def test_fuzz_absorption_known_answers_and_by_sampling():
    assert T.fuzz_absorption(0.0, 1.0) == 0.5 and T.fuzz_absorption(1.0, 1.0) == 0.0 and T.fuzz_absorption(0.25, 0.5) == 0.25
    assert T.fuzz_absorption(0.6, 0.5) == 0.0
    rng = np.random.default_rng(2)                                     # the construction itself, in float64: r + f u against n
    u = K.unit(rng, 400000)
    for cos, f in ((0.3, 1.0), (0.1, 0.2), (0.45, 0.5)):
        r = np.array([np.sqrt(1.0 - cos * cos), cos, 0.0])
        share = (((r[None] + f * u) @ np.array([0.0, 1.0, 0.0])) <= 0).mean()
        p = T.fuzz_absorption(cos, f)
        assert abs(share - p) < 6.0 * np.sqrt(p * (1 - p) / len(u))


def test_sky_and_pack_known_answers():
    assert np.allclose(T.sky([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3.0, 0.0]]),
                       [[0.5, 0.7, 1.0], [1.0, 1.0, 1.0], [0.75, 0.85, 1.0], [0.5, 0.7, 1.0]], atol=1e-15)
    w, b, tie = T.pack([[1.0, 0.5, 0.0], [2.0, 0.25, 0.001], [0.5, 0.5 / 255.0, 1.4999 / 255.0]], False)
    assert [hex(int(x)) for x in w] == ["0xff8000ff", "0xff4000ff", "0x800101ff"]      # 127.5 rounds away from zero, as roundf does
    assert tie.tolist() == [[False, True, False], [False, False, False], [True, True, False]]
    w, b, tie = T.pack([[0.25, 4.0, 1.0 / 255.0 ** 2]], True)
    assert b.tolist() == [[128, 255, 1]] and tie[0, 0] and not tie[0, 1]


# ====================================================================================================================== 5. mutants of the new helpers
def test_mutant_integrating_sphere_off_by_one_and_linear_form_factor_are_rejected():
    w, h, spp = K.INTEGRATING_SIZE
    for r, R, a, E, D in K.INTEGRATING:
        law = T.integrating_sphere(r, R, a, E, D)
        K.check_integrating(law, np.full(w * h, law["mean"]), spp, law["casts"], D)                    # the law's own noise-free frame passes
        one_more = T.integrating_sphere(r, R, a, E, D + 1)                                              # D terms for D - 1
        if D <= 8:                                                      # the extra term a^D (1 - F)^(D - 1) F E: 17 sigma of the frame mean at D = 8,
            with pytest.raises(AssertionError, match="sigma"):         # 0.3 at R = 4, D = 12, 1e-5 at D = 30: the shallow cases guard the cut-off
                K.check_integrating(law, np.full(w * h, one_more["mean"]), spp)
        if D <= 12:                                                     # one more cast with probability (1 - F)^(D - 1): 0.49 at R = 4, D = 12
            with pytest.raises(AssertionError, match="casts"):
                K.check_integrating(law, np.full(w * h, law["mean"]), spp, one_more["casts"], D)
        linear = T.integrating_sphere(np.sqrt(r * R), R, a, E, D)                                       # F = r / R
        assert linear["F"] == pytest.approx(r / R)
        with pytest.raises(AssertionError, match="sigma"):
            K.check_integrating(law, np.full(w * h, linear["mean"]), spp)


@pytest.fixture(scope="module")
def fuzz_cos(oracle):
    """Scene-independent of f: the cosines of incidence of every sample of the fuzz frame, per ground."""
    cam, p = K.fuzz_camera()
    o, d, _ = K.expected_camera_rays(cam, p)
    tri = K.fuzz_scene("triangles", 1.0, make_triangle(oracle), oracle.merge)
    return {"triangles": K.fuzz_cosines(tri, o, d, p.spp), "sphere": K.fuzz_cosines(K.fuzz_scene("sphere", 1.0), o, d, p.spp)}


@pytest.mark.parametrize("f", K.FUZZ["fs"])
def test_mutant_fuzz_in_the_ball_and_unscaled_fuzz_are_rejected(fuzz_cos, f):
    cos = fuzz_cos["triangles"]
    full = np.array(K.FUZZ["rgb"]) * K.FUZZ["c"]
    frame = lambda law: full[None] * (1.0 - law(cos, f).mean(axis=0))[:, None]      # noqa: E731
    fig = K.check_fuzz(frame(T.fuzz_absorption), cos, f)
    assert fig["statistical"] > 100 and (f == 1.0 or fig["exact"] > 100)
    assert cos.max() > 0.97 and cos.min() < 0.17
    with pytest.raises(AssertionError, match="sigma"):
        K.check_fuzz(frame(K.absorption_in_the_ball), cos, f)
    if f != 1.0:
        with pytest.raises(AssertionError):
            K.check_fuzz(frame(K.absorption_unscaled), cos, f)
    with pytest.raises(AssertionError):
        K.check_fuzz(frame(T.fuzz_absorption)[:, ::-1], cos, f)        # the attenuation's channels swapped


@pytest.fixture(scope="module")
def glass_sphere():
    """The glass-sphere scene with the float32 primary rays of DESIGN.md 4.1 (themselves within (b)'s bounds of camera_ray) and their tree."""
    sc, cam, p = K.glass_sphere_scene()
    o, d = K.pinhole_rays_f32(cam, p)
    K.check_camera_rays(cam, p, o, d, K.expected_camera_rays(cam, p))
    return sc, cam, p, o, d, K.glass_tree(sc, p, o, d)


def test_mutant_glass_sphere_with_ri_kept_or_the_normal_unflipped_is_rejected(glass_sphere):
    sc, cam, p, o, d, tree = glass_sphere
    rng = np.random.default_rng(4)
    fig = K.check_glass_tree(K.sample_glass_tree(tree, rng), tree)
    assert fig["through_glass"] >= 500 and fig["reflected"] >= 20
    for m in ("ri_kept", "normal_unflipped"):
        with pytest.raises(AssertionError):
            K.check_glass_tree(K.sample_glass_tree(K.glass_tree(sc, p, o, d, mutate=m), rng), tree)


def test_mutant_sky_of_y_is_rejected():
    sc, cam, p = K.sky_scene()
    xx, yy = K.pixel_grid(p)
    _, d, _ = T.camera_ray(cam, p, xx, yy)
    fig = K.check_sky(T.sky(d), cam, p)
    assert fig["t_range"][0] < 0.4 and fig["t_range"][1] > 0.8       # below and above the horizon
    with pytest.raises(AssertionError, match="bound"):
        K.check_sky(K.sky_of_y(d), cam, p)


@pytest.mark.parametrize("gamma2", [False, True], ids=["linear", "gamma2"])
def test_mutant_pack_truncated_reversed_or_gamma_after_the_bytes_is_rejected(gamma2):
    sc, cam, p = K.pack_scene(gamma2)
    rgb, amb, hit = K.pack_expectation(sc, cam, p)
    words, b, tie = T.pack(rgb, gamma2)
    fig = K.check_pack(words, rgb, gamma2)
    assert fig["ties"] == 0 and fig["bytes_seen"] == 256 and fig["clamped"] > 20 and fig["zeros"] > 1000

    def truncated(x, g):
        x = np.asarray(x, np.float32).astype(np.float64)
        t = np.floor(255.0 * np.clip(np.sqrt(x) if g else x, 0.0, 1.0)).astype(np.uint32)
        return (t[:, 0] << 24) | (t[:, 1] << 16) | (t[:, 2] << 8) | np.uint32(0xFF)

    def bytes_then_gamma(x, g):
        lin = T.pack(x, False)[1]
        t = np.floor(255.0 * np.sqrt(lin / 255.0) + 0.5).astype(np.uint32)
        return (t[:, 0] << 24) | (t[:, 1] << 16) | (t[:, 2] << 8) | np.uint32(0xFF)

    with pytest.raises(AssertionError, match="another byte"):
        K.check_pack(truncated(rgb, gamma2), rgb, gamma2)
    with pytest.raises(AssertionError):
        K.check_pack((b[:, 2] << 24) | (b[:, 1] << 16) | (b[:, 0] << 8) | np.uint32(0xFF), rgb, gamma2)      # a, b, g, r for r, g, b, a
    with pytest.raises(AssertionError):
        K.check_pack(np.uint32(0xFF000000) | (b[:, 2] << 16) | (b[:, 1] << 8) | b[:, 0], rgb, gamma2)         # the word's bytes reversed
    if gamma2:
        with pytest.raises(AssertionError, match="another byte"):
            K.check_pack(bytes_then_gamma(rgb, gamma2), rgb, gamma2)


# ====================================================================================================================== 6. the oracle against the closed forms
THREADS = 16


@pytest.mark.parametrize("case", range(len(K.INTEGRATING)), ids=K.INTEGRATING_IDS)
def test_oracle_integrating_sphere(oracle, case):
    r, R, a, E, D = K.INTEGRATING[case]
    sc = K.integrating_scene(r, R, a, E)
    cam, p = K.integrating_camera(r, R, D)
    o, d, _ = K.expected_camera_rays(cam, p)
    first = T.nearest_hit(o, d, p.t_min, np.inf, sc["spheres"], chunk=1 << 16)
    assert K.all_meet_the_wall(first["kind"], first["index"]) and not first["ambiguous"].any()
    _, total, casts = render(oracle, sc, cam, p, want_sum=True, threads=THREADS)
    assert np.array_equal(total[..., 0], total[..., 1]) and np.array_equal(total[..., 0], total[..., 2])
    n = p.width * p.height * p.spp
    fig = K.check_integrating(T.integrating_sphere(r, R, a, E, D), total[..., 0].astype(np.float64) / p.spp, p.spp, casts / n, D)
    print("oracle integrating sphere", K.INTEGRATING_IDS[case], fig)


@pytest.mark.parametrize("f", K.FUZZ["fs"])
@pytest.mark.parametrize("ground", ["triangles", "sphere"])
def test_oracle_metal_fuzz_obeys_the_absorption_law(oracle, fuzz_cos, ground, f):
    sc = K.fuzz_scene(ground, f, make_triangle(oracle), oracle.merge)
    cam, p = K.fuzz_camera(ground)
    _, total, _ = render(oracle, sc, cam, p, want_sum=True, threads=THREADS)
    fig = K.check_fuzz(total.reshape(-1, 3).astype(np.float64) / p.spp, fuzz_cos[ground], f)
    print("oracle fuzz", ground, f, fig)
    assert fig["statistical"] > 100 and (f == 1.0 or fig["exact"] > 100)


def test_oracle_glass_sphere_follows_the_path_tree(oracle, glass_sphere):
    """The reference's own share of skipped pixels: 34 of 2304 (1.5 %)."""
    sc, cam, p, o, d, tree = glass_sphere
    px, _ = render(oracle, sc, cam, p)
    fig = K.check_glass_tree(px, tree)
    print("oracle glass sphere", fig)
    assert fig["through_glass"] >= 500 and fig["reflected"] >= 20 and fig["counted"] >= 100


def test_oracle_sky(oracle):
    sc, cam, p = K.sky_scene()
    px, total, casts = render(oracle, sc, cam, p, want_sum=True)
    assert casts == p.width * p.height
    fig = K.check_sky(total, cam, p)
    print("oracle sky", fig)
    assert fig["t_range"][0] < 0.4 and fig["t_range"][1] > 0.8       # below and above the horizon


@pytest.mark.parametrize("gamma2", [False, True], ids=["linear", "gamma2"])
def test_oracle_pack(oracle, gamma2):
    sc, cam, p = K.pack_scene(gamma2)
    rgb, amb, hit = K.pack_expectation(sc, cam, p)
    assert not amb.any()
    px, total, _ = render(oracle, sc, cam, p, want_sum=True)
    assert np.array_equal(total.reshape(-1, 3), rgb), "the linear frame is the material's colour, bit for bit"
    fig = K.check_pack(px, total, gamma2)
    print("oracle pack", "gamma2" if gamma2 else "linear", fig)
    assert fig["ties"] == 0 and fig["bytes_seen"] == 256 and fig["clamped"] > 20 and fig["zeros"] > 1000
