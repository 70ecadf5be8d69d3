"""The emitters' sampling table and sampling law (RT3_FLAG_LIGHT_SAMPLING) without a GPU.

rt3_debug_light_sample builds the table serially in C and applies the functions the device's shade_lane calls (rt3_light_sample.hpp); it must equal
tests/light_sample_ref.py (numpy float32 + Python integers) bit for bit, on random soups of faces and spheres of all four material kinds and on the
degenerate cases.  Then the properties the estimator rests on: the chosen light's frequencies follow q / total (chi-square), and the points are
uniform on a triangle and on a sphere (first two moments)."""
import numpy as np
import pytest

import light_sample_ref as S

F = np.float32
PAIRS = 3000                                                          # (base, depth) pairs per scene


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pairs(seed, k=PAIRS):
    rng = np.random.default_rng(700 + seed)
    base = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    depth = rng.integers(0, 12, k).astype(np.uint32)
    depth[:4] = (0, 1, 63, 64)
    base[:2] = (0, 0xFFFFFFFF)
    return base, depth


def soup(rt3, seed, n_faces, n_sph, shared_vertices=False):
    """Random faces and spheres, every material kind among them, rgb in [-0.2, 3): some channels negative."""
    rng = np.random.default_rng(seed)
    if shared_vertices:                                               # an indexed mesh: faces share vertices, in any order
        verts = np.zeros((max(n_faces, 3), 4), F)
        verts[:, :3] = rng.normal(0.0, 1.5, (len(verts), 3))
        idx = np.stack([rng.permutation(len(verts))[:3] for _ in range(n_faces)]) if n_faces else np.zeros((0, 3), np.int64)
    else:
        verts = np.zeros((3 * n_faces, 4), F)
        verts[:, :3] = (rng.uniform(-2, 2, (n_faces, 1, 3)) + rng.normal(0.0, 0.4, (n_faces, 3, 3))).reshape(-1, 3)
        idx = np.arange(3 * n_faces).reshape(-1, 3)
    faces = np.zeros(n_faces, rt3.GFACE)
    if n_faces:
        faces["v1"], faces["v2"], faces["v3"] = idx[:, 0], idx[:, 1], idx[:, 2]
        faces["normal"] = rng.normal(0, 1, (n_faces, 3))              # the law never reads the stored normal
    fm = np.zeros(n_faces, rt3.MATERIAL)
    fm["kind"] = np.arange(n_faces) % 4
    fm["rgb"] = rng.uniform(-0.2, 3.0, (n_faces, 3))
    cr = np.zeros((n_sph, 4), F)
    cr[:, :3] = rng.uniform(-3, 3, (n_sph, 3))
    cr[:, 3] = rng.uniform(0.05, 0.8, n_sph)
    sm = np.zeros(n_sph, rt3.MATERIAL)
    sm["kind"] = (np.arange(n_sph) + 1) % 4
    sm["rgb"] = rng.uniform(-0.2, 3.0, (n_sph, 3))
    return faces, verts, fm, cr, sm


def compare(rt3, scene, seed, k=PAIRS):
    faces, verts, fm, cr, sm = scene
    T = S.Table(faces, verts, fm, cr, sm)
    base, depth = pairs(seed, k)
    got = rt3.light_sample(faces, verts, fm, cr, sm, base, depth)
    if T.total == 0:
        assert (got[0] == S.NO_LIGHT).all() and all((bits(g) == 0).all() for g in got[1:])
        return T, None
    light, point, normal, area, pl, a, b = S.sample(T, base, depth)
    assert np.array_equal(got[0], light), "%d lights differ" % (got[0] != light).sum()
    for name, g, w in (("point", got[1], point), ("normal", got[2], normal), ("area", got[3], area), ("pl", got[4], pl)):
        assert np.array_equal(bits(g), bits(w)), "%s: %d values differ" % (name, (bits(g) != bits(w)).sum())
    assert (T.q[light] > 0).all() and (pl > 0).all()                   # an entry with q = 0 is never drawn
    return T, (light, point, normal, area, pl)


@pytest.mark.parametrize("n_faces,n_sph,shared", [(40, 0, False), (0, 33, False), (57, 41, False), (64, 7, True), (1, 1, False)])
def test_the_host_law_equals_the_numpy_restatement(rt3, n_faces, n_sph, shared):
    scene = soup(rt3, 11 + n_faces + n_sph, n_faces, n_sph, shared)
    T, out = compare(rt3, scene, n_faces + n_sph)
    faces, verts, fm, cr, sm = scene
    assert T.total > 0 and T.total == int(T.cdf[-1]) and T.q.max() == 2 ** 24
    kinds = np.concatenate([fm["kind"], sm["kind"]])
    assert (T.q[kinds != 0] == 0).all() and len(T.q) == n_faces + n_sph      # only FLAT emits; faces first, then spheres
    light, point, normal, area, pl = out
    assert np.allclose(np.linalg.norm(normal.astype(np.float64), axis=1), 1.0, atol=1e-5)
    isf = light < n_faces
    if isf.any():                                                     # a face's point lies in the face's plane, inside the triangle
        G = T.faces
        rel = point[isf].astype(np.float64) - G.p1[light[isf]]
        assert np.abs((rel * normal[isf]).sum(axis=1)).max() < 1e-5
    if (~isf).any():                                                  # a sphere's point lies on the sphere
        s = cr[light[~isf] - n_faces].astype(np.float64)
        assert np.abs(np.linalg.norm(point[~isf] - s[:, :3], axis=1) - s[:, 3]).max() < 1e-5
    one = rt3.light_sample(faces, verts, fm, cr, sm, 123, 2)           # the scalar form
    assert isinstance(one[0], int) and one[1].shape == (3,) and one[2].shape == (3,) and one[4] > 0


def test_degenerate_entries_have_no_weight(rt3):
    """A zero-area face, NaN and negative colour channels, a NaN radius record, an infinite colour: weights stay finite numbers, the dead entries have
    q = 0 and are never drawn, and the C function agrees bit for bit."""
    faces, verts, fm, cr, sm = soup(rt3, 5, 12, 9)
    fm["kind"], sm["kind"] = 0, 0                                      # every primitive FLAT
    verts[3:6, :3] = verts[3, :3]                                     # face 1: a point
    verts[6:9, :3] = ((1.0, 2.0, 3.0), (2.0, 3.0, 4.0), (3.0, 4.0, 5.0))  # face 2: collinear, the edges exact
    fm["rgb"][3] = (np.nan, 2.0, -1.0)                               # brightness 2
    fm["rgb"][4] = (-1.0, -2.0, np.nan)                              # brightness 0
    fm["rgb"][5] = (np.inf, 1.0, 1.0)                                # brightness FLT_MAX, the largest weight
    verts[18:21, :3] = np.nan                                        # face 6: no area
    cr[2, 3] = np.nan                                                # a sphere record nothing can hit
    cr[3, 3] = np.inf
    cr[4, 0] = np.nan                                                # a NaN centre with a good radius: a weight, and points that are NaN
    sm["rgb"][5] = (0.0, 0.0, 0.0)
    T, out = compare(rt3, (faces, verts, fm, cr, sm), 99)
    assert np.isfinite(T.w).all() and T.total > 0
    for dead in (1, 2, 4, 6, 12 + 2, 12 + 3, 12 + 5):
        assert T.q[dead] == 0, dead
    assert T.q[5] == 2 ** 24 and T.q[3] >= 1 and T.q[12 + 4] >= 1
    assert S.brightness(fm)[3] == 2.0 and S.brightness(fm)[5] == S.FLT_MAX


def test_a_scene_without_an_emitter_is_reported_not_sampled(rt3):
    faces, verts, fm, cr, sm = soup(rt3, 6, 9, 9)
    fm["kind"] = np.where(fm["kind"] == 0, 1, fm["kind"])
    sm["kind"] = np.where(sm["kind"] == 0, 2, sm["kind"])
    T, out = compare(rt3, (faces, verts, fm, cr, sm), 3, 16)
    assert T.total == 0 and out is None and not T.q.any()
    fm["kind"][0], fm["rgb"][0] = 0, (0.0, -1.0, np.nan)               # a FLAT face of brightness 0 is no emitter either
    T, out = compare(rt3, (faces, verts, fm, cr, sm), 3, 16)
    assert T.total == 0


def test_chosen_lights_follow_the_table(rt3):
    """Pearson's chi-square of the drawn light against q / total over N = 60 000 draws at a fixed seed, the entries with an expected count below 5 pooled
    into one class.  Significance level 1e-4 (a fixed seed: the test is deterministic; the level says how surprising a failure of a correct law would
    have been): chi2 <= the 1 - 1e-4 quantile of chi-square with k - 1 degrees of freedom, taken from the Wilson-Hilferty approximation with
    z = 3.719."""
    faces, verts, fm, cr, sm = soup(rt3, 8, 24, 24)
    T = S.Table(faces, verts, fm, cr, sm)
    n = 60000
    rng = np.random.default_rng(9)
    base = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    depth = rng.integers(0, 8, n).astype(np.uint32)
    light = S.sample(T, base, depth)[0]
    some = slice(0, 2000)
    assert np.array_equal(rt3.light_sample(faces, verts, fm, cr, sm, base[some], depth[some])[0], light[some])
    expect = T.q.astype(np.float64) / T.total * n
    count = np.bincount(light, minlength=len(T.q)).astype(np.float64)
    assert (count[T.q == 0] == 0).all()
    big = expect >= 5
    obs = np.append(count[big], count[~big].sum())
    exp = np.append(expect[big], expect[~big].sum())
    if exp[-1] == 0:
        obs, exp = obs[:-1], exp[:-1]
    k = len(exp)
    assert k >= 8
    chi2 = ((obs - exp) ** 2 / exp).sum()
    dof = k - 1
    limit = dof * (1 - 2 / (9 * dof) + 3.719 * np.sqrt(2 / (9 * dof))) ** 3
    print("chi-square %.2f with %d degrees of freedom, limit %.2f" % (chi2, dof, limit))
    assert chi2 <= limit


def test_points_are_uniform_on_a_triangle_and_on_a_sphere(rt3):
    """One emissive triangle, then one emissive sphere, N = 40 000 points each.  A uniform point on a triangle has barycentric coordinates with mean 1/3,
    variance 1/18 and covariance -1/36; a uniform point on the unit sphere has components with mean 0, variance 1/3 and covariance 0.  Every statistic is
    a mean of N independent bounded terms (|term| <= 1), so its standard error is at most sqrt(Var / N) <= 1 / sqrt(N); the bound is 6 of those standard
    errors with the terms' exact variance bounded by their range: 6 / sqrt(N) x (range / 2)."""
    n = 40000
    rng = np.random.default_rng(10)
    base = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    depth = rng.integers(0, 8, n).astype(np.uint32)
    tol = 6.0 / np.sqrt(n) * 0.5                                       # terms in [0, 1] or [-1/2, 1/2]: half the range
    fm = np.zeros(1, rt3.MATERIAL)
    fm["rgb"] = 1.0
    faces = np.zeros(1, rt3.GFACE)
    faces["v2"], faces["v3"] = 1, 2
    verts = np.array([[0.5, -1.0, 2.0, 0], [2.5, 0.0, 2.5, 0], [0.0, 1.5, 1.0, 0]], F)
    light, point, normal, area, pl = rt3.light_sample(faces, verts, fm, None, None, base, depth)
    assert (light == 0).all() and (pl == 1.0).all()
    e1, e2 = (verts[1, :3] - verts[0, :3]).astype(np.float64), (verts[2, :3] - verts[0, :3]).astype(np.float64)
    ab = np.linalg.lstsq(np.stack([e1, e2], axis=1), (point.astype(np.float64) - verts[0, :3]).T, rcond=None)[0].T
    a, b = ab[:, 0], ab[:, 1]
    assert a.min() > -1e-6 and b.min() > -1e-6 and (a + b).max() < 1 + 1e-6
    assert abs(area[0] - 0.5 * np.linalg.norm(np.cross(e1, e2))) < 1e-5
    for name, got, want in (("E a", a.mean(), 1 / 3), ("E b", b.mean(), 1 / 3), ("E a^2", (a * a).mean(), 1 / 6), ("E b^2", (b * b).mean(), 1 / 6),
                            ("E ab", (a * b).mean(), 1 / 12)):
        print("triangle %s: %.5f, uniform %.5f, bound %.5f" % (name, got, want, tol))
        assert abs(got - want) <= tol, name
    sm = np.zeros(1, rt3.MATERIAL)
    sm["rgb"] = 2.0
    cr = np.array([[1.0, -2.0, 0.5, 0.75]], F)
    light, point, normal, area, pl = rt3.light_sample(None, None, None, cr, sm, base, depth)
    assert (light == 0).all() and abs(area[0] - 4 * np.pi * 0.75 ** 2) < 1e-5
    v = (point.astype(np.float64) - cr[0, :3]) / 0.75
    assert np.abs(v - normal).max() < 1e-5
    tol = 6.0 / np.sqrt(n) * 1.0                                       # terms in [-1, 1]
    for i in range(3):
        assert abs(v[:, i].mean()) <= tol and abs((v[:, i] ** 2).mean() - 1 / 3) <= tol, i
        j = (i + 1) % 3
        assert abs((v[:, i] * v[:, j]).mean()) <= tol, (i, j)
