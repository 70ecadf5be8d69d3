"""Lens sequences without a device (include/rt3.h "Lens sequences"): rt3_debug_turns and rt3_debug_optic_pixel — the statements
the lens forms of k_temporal_reproject evaluate — against the numpy restatement (tests/optic_ref.py) bit for bit, turns against float64 arctan2,
the inverse law against the forward law over whole frames, and the reprojection against float64 geometry of a scene of spheres."""
import numpy as np
import pytest

import lens_ref as L
import optic_ref as O

F = np.float32
MODELS = ("equirect", "fisheye", "ortho", "cube")
FRAMES = {"equirect": ((2, 2), (33, 17), (64, 32)), "fisheye": ((2, 2), (33, 17), (64, 32)), "ortho": ((2, 2), (33, 17), (64, 32)),
          "cube": ((2, 12), (5, 30))}
U24 = 2.0 ** -24            # the unit roundoff of f32
EPS_SINCOS = 5e-7           # sincos2pi's absolute error
EPS_TURNS = 2.0 ** -23      # turns' error in turns


@pytest.fixture(scope="module")
def turns_inputs():
    """More than 10^6 (c, s): random directions with lengths e^+-20, dense slopes in [0, 1] in all eight octants, and the special values."""
    rng = np.random.default_rng(2024)
    n = 700000
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    length = np.exp(rng.uniform(-20.0, 20.0, n))
    c, s = (np.cos(ang) * length).astype(F), (np.sin(ang) * length).astype(F)
    t = np.concatenate([np.linspace(0.0, 1.0, 50001), rng.uniform(0.0, 1.0, 30000)]).astype(F)
    one = np.ones_like(t)
    oct_c = np.concatenate([one, t, -t, -one, -one, -t, t, one])
    oct_s = np.concatenate([t, one, one, t, -t, -one, -one, -t])
    sp = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30, 1e30, np.inf, -np.inf, np.nan, 3e-45, 3.4e38], F)
    sc, ss = (a.reshape(-1) for a in np.meshgrid(sp, sp))
    c, s = np.concatenate([c, oct_c, sc]), np.concatenate([s, oct_s, ss])
    assert c.size >= 10 ** 6
    return c, s


def test_turns_equals_the_restatement_bit_for_bit(rt3, turns_inputs):
    c, s = turns_inputs
    fn = rt3.lib().rt3_debug_turns
    got = np.array([fn(a, b) for a, b in zip(c.tolist(), s.tolist())], F)
    want = O.turns(c, s)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (c[~same][:4], s[~same][:4], got[~same][:4], want[~same][:4])
    assert float(rt3.turns(1.0, 1.0)) == float(O.turns(1.0, 1.0))


def test_turns_exact_values():
    t = lambda c, s: float(O.turns(c, s))       # noqa: E731
    assert (t(1, 0), t(0, 1), t(-1, 0), t(0, -1)) == (0.0, 0.25, 0.5, 0.75)
    assert (t(3e-45, 0), t(0, 3.4e38), t(-1e30, 0.0), t(-0.0, -1e-30)) == (0.0, 0.25, 0.5, 0.75)
    for k, (c, s) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1))):
        want = F((2 * k + 1) / 8.0)
        assert abs(float(O.turns(c, s)) - float(want)) <= float(np.spacing(want)), (c, s)
    assert t(1.0, -1e-30) == 0.0                                          # 1 - tiny rounds to 1, which wraps to 0: the result stays in [0, 1)
    for c, s in ((0.0, 0.0), (-0.0, 0.0), (np.inf, 1.0), (1.0, -np.inf), (np.inf, np.inf), (np.nan, 1.0), (1.0, np.nan)):
        assert np.isnan(O.turns(c, s)), (c, s)


def test_turns_is_within_2_to_the_minus_23_turns_of_float64_atan2(turns_inputs):
    c, s = turns_inputs
    got = O.turns(c, s).astype(np.float64)
    ok = np.isfinite(c) & np.isfinite(s) & ((c != 0) | (s != 0))
    assert not np.isnan(got[ok]).any() and np.isnan(got[~ok]).all()
    assert (got[ok] >= 0.0).all() and (got[ok] < 1.0).all()
    err = np.abs(got[ok] - O.turns64(c[ok], s[ok]))
    err = np.minimum(err, 1.0 - err)                                          # the angle is cyclic
    print("turns: %d inputs, max error %.3g turns (2^-23 = %.3g)" % (ok.sum(), err.max(), EPS_TURNS))
    assert err.max() <= EPS_TURNS


# ------------------------------------------------------------------------------------------------ rt3_debug_optic_pixel
def random_lens(rt3, model, rng):
    origin = rng.uniform(-3.0, 3.0, 3)
    at = origin + rng.normal(size=3)
    vup = rng.normal(size=3)
    return rt3.make_lens(model, origin, at, vup, fov_deg=float(rng.uniform(60.0, 360.0)), extent=tuple(rng.uniform(0.5, 6.0, 2)))


def host_pixels(rt3, lens, w, h, r, is_hit):
    out = [rt3.lens_pixel(lens, w, h, v, is_hit) for v in r]
    return (np.array([o[0] for o in out], F), np.array([o[1] for o in out], F), np.array([o[2] for o in out], F),
            np.array([o[3] for o in out]), np.array([o[4] for o in out]))


def same_bits(a, b):
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("model", MODELS)
def test_host_inverse_law_equals_the_restatement(rt3, model):
    """Bit for bit: random lenses with random vup, every frame, hits (points) and misses (unit directions), all six cube faces, r = 0."""
    rng = np.random.default_rng(MODELS.index(model))
    faces = set()
    frames = FRAMES[model] if model != "cube" else ((2, 12), (5, 30), (16, 96))
    for (w, h) in frames:
        for _ in range(3):
            lens = random_lens(rt3, model, rng)
            axes = np.array([list(lens.right), list(lens.up), list(lens.forward)], F)
            pts = rng.normal(size=(150, 3)) * np.exp(rng.uniform(-3.0, 4.0, (150, 1)))
            dirs = rng.normal(size=(150, 3))
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            special = np.concatenate([axes, -axes, axes * F(7.5), [[0.0, 0.0, 0.0]], axes[0:1] + axes[1:2], axes[1:2] - axes[2:3]])
            for r, is_hit in ((np.concatenate([pts, special]).astype(F), True), (np.concatenate([dirs, special]).astype(F), False)):
                gx, gy, gz, gf, gv = host_pixels(rt3, lens, w, h, r, is_hit)
                wx, wy, wz, wf, wv = O.project(lens, w, h, r)
                if model == "ortho" and not is_hit:                       # not projected: (NaN, NaN, zhat), valid
                    assert np.isnan(gx).all() and np.isnan(gy).all() and gv.all() and same_bits(gz, wz) and not gf.any()
                    continue
                assert same_bits(gx, wx) and same_bits(gy, wy) and same_bits(gz, wz), (model, w, h)
                assert np.array_equal(gf, wf) and np.array_equal(gv, wv)
                assert gv[len(r) - 3] == (model == "ortho")               # r = 0: no history (the orthographic window's centre is a position)
                faces.update(gf[gv].tolist())
    assert faces == (set(range(6)) if model == "cube" else {0})


def test_fisheye_poles_and_an_orthographic_miss(rt3):
    for fov in (90.0, 180.0, 360.0):
        lens = rt3.make_lens("fisheye", (1.0, 2.0, 3.0), (0.0, 2.5, -1.0), (0.2, 1.0, 0.1), fov_deg=fov)
        fwd = np.array(list(lens.forward), F)
        for (w, h) in ((33, 17), (64, 32), (2, 2)):
            x, y, z, face, valid = rt3.lens_pixel(lens, w, h, fwd * F(3.0))
            assert valid and (x, y) == (0.5 * w - 0.5, 0.5 * h - 0.5) and face == 0          # the image centre, exactly
            assert abs(z - 3.0) <= 4 * float(np.spacing(F(3.0)))
    for at in ((0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)):                              # axis-aligned: the local x and y of -forward are exactly 0
        lens = rt3.make_lens("fisheye", (0.0, 0.0, 0.0), at, fov_deg=360.0)
        back = -np.array(list(lens.forward), F)
        for (w, h) in ((33, 17), (2, 2)):
            x, y, z, face, valid = rt3.lens_pixel(lens, w, h, back * F(2.0))
            assert not valid and np.isnan(x) and np.isnan(y) and z == 2.0                     # the pole behind the lens: no history
            ox, oy, oz, of, ov = O.project(lens, w, h, back * F(2.0))
            assert not ov and np.isnan(ox) and np.isnan(oy) and oz == 2.0
    lens = rt3.make_lens("ortho", (0.0, 0.0, 5.0), (0.0, 0.0, 0.0), extent=(4.0, 2.0))
    x, y, z, face, valid = rt3.lens_pixel(lens, 8, 4, (0.0, 0.0, -1.0), is_hit=False)
    assert valid and np.isnan(x) and np.isnan(y) and z == 1.0
    x, y, z, face, valid = rt3.lens_pixel(lens, 8, 4, (1.0, -0.5, -3.0), is_hit=True)
    assert valid and (x, y, z) == (5.5, 2.5, 3.0)                                             # nx = 0.5 -> px = 6; ny = -0.5 -> py = 3
    with pytest.raises(rt3.Fatal):
        rt3.lens_pixel(rt3.make_lens("cube", (0, 0, 0), (0, 0, -1)), 4, 20, (0.0, 0.0, -1.0))  # H != 6 W
    with pytest.raises(rt3.Fatal):
        rt3.lens_pixel(lens, 1, 4, (0.0, 0.0, -1.0))


# ------------------------------------------------------------------------------------------------ the round trip
def angular_error(model, origin_norm, depth):
    """The bound of DESIGN.md 4.24 on the angle (radians) between the float32 r the inverse law is handed and the exact direction of the pixel
    centre: the forward law's direction, the point o + z d and P - o', and the three local dot products."""
    e_d = {"equirect": np.sqrt(3.0) * (2.0 * EPS_SINCOS + 2.0 * U24), "fisheye": np.sqrt(2.0) * (EPS_SINCOS + 2.0 * U24)}.get(model, 0.0)
    return e_d + 2.0 * np.sqrt(3.0) * U24 * (origin_norm / depth + 1.0) + 16.0 * U24


def pixel_bounds(model, lens, w, h, depth):
    """(bound on |x' - x|, bound on |y' - y|) per pixel, (H, W) each."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    on = float(np.linalg.norm(np.array(list(lens.origin), np.float64)))
    th = angular_error(model, on, depth)
    ulp = 4.0 * U24 * max(w, h)                                    # px, py and the subtraction of 0.5: a few roundings at the frame's scale
    if model == "equirect":
        polar = np.pi * (yy + 0.5) / h
        return w * (th / (2.0 * np.pi * np.sin(polar)) + EPS_TURNS) + ulp, h * (th / np.pi + 2.0 * EPS_TURNS) + ulp + 0 * xx
    if model == "fisheye":
        m, hf = 0.5 * min(w, h), float(F(lens.half_fov_turns))
        rho = np.hypot(xx + 0.5 - 0.5 * w, 0.5 * h - (yy + 0.5))    # the pixel's distance from the image centre, in pixels
        tau = np.minimum(rho / m * hf, 0.5)
        radial = m / hf * (th / (2.0 * np.pi) + EPS_TURNS)
        with np.errstate(divide="ignore", invalid="ignore"):
            azimuthal = np.where(tau > 0, rho * th / np.sin(2.0 * np.pi * tau), 0.0)
        b = radial + azimuthal + ulp
        return b, b
    if model == "ortho":
        he = np.array(list(lens.half_extent), np.float64)
        pos = 8.0 * U24 * (on + np.hypot(he[0], he[1]) + depth)      # the position error of P - o' and of its dot products
        return 0.5 * w * pos / he[0] + ulp + 0 * xx, 0.5 * h * pos / he[1] + ulp + 0 * xx
    b = w * th + ulp + 0 * xx                                         # cube: d(sc / m) <= (1 + (sc / m)^2) th <= 2 th, times N / 2
    return b, b


@pytest.mark.parametrize("model", MODELS)
def test_round_trip_through_the_forward_law(rt3, model):
    """Every pixel of small frames: the centre ray's point at depths 0.5, 3 and 100, projected back into the same lens, lands on the pixel
    within the bound of DESIGN.md 4.24 (sincos2pi's 5e-7, turns' 2^-23 and the conditioning)."""
    lens = rt3.make_lens(model, (0.3, 1.1, 2.0), (-0.2, 0.4, -1.0), (0.1, 1.0, 0.05), fov_deg=200.0, extent=(3.0, 1.75))
    worst = 0.0
    for (w, h) in FRAMES[model]:
        o, d = O.centre_rays(lens, w, h)
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        for depth in (0.5, 3.0, 100.0):
            P = (o + F(depth) * d).astype(F)
            r = (P - L._vec(lens, "origin")).astype(F)
            xp, yp, zhat, face, valid = O.project(lens, w, h, r)
            bx, by = pixel_bounds(model, lens, w, h, depth)
            ex, ey = np.abs(xp.astype(np.float64) - xx), np.abs(yp.astype(np.float64) - yy)
            if model == "equirect":
                ex = np.minimum(ex, w - ex)                           # columns are cyclic
            if model == "fisheye":                                    # near the pole behind the lens the azimuth is ill-conditioned: out of the claim
                near = np.hypot(xx + 0.5 - 0.5 * w, 0.5 * h - (yy + 0.5)) / (0.5 * min(w, h)) * float(F(lens.half_fov_turns)) <= 0.45
            else:
                near = np.ones((h, w), bool)
            assert valid[near].all()
            if model == "cube":
                assert np.array_equal(face, (yy // w).astype(np.int64))
            ratio = max(float((ex / bx)[near].max()), float((ey / by)[near].max()))
            worst = max(worst, ratio)
            print("%s %dx%d depth %g: max |x' - x| %.3g, max |y' - y| %.3g px, largest deviation / bound %.3f"
                  % (model, w, h, depth, ex[near].max(), ey[near].max(), ratio))
            assert (ex[near] <= bx[near]).all() and (ey[near] <= by[near]).all()
            zt = depth if model != "ortho" else depth
            assert np.abs(zhat[near].astype(np.float64) - zt).max() <= 16.0 * U24 * (zt + 4.0)
    assert worst > 0.0


# ------------------------------------------------------------------------------------------------ geometry truth
def trace64(spheres, o, d):
    """Nearest hit of rays (o, d) (K, 3) float64 against spheres (n, 4): (t, index), t = inf and index = -1 for a miss."""
    t_best = np.full(len(o), np.inf)
    i_best = np.full(len(o), -1)
    for i, (cx, cy, cz, rad) in enumerate(np.asarray(spheres, np.float64)):
        oc = o - np.array([cx, cy, cz])
        b = (oc * d).sum(-1)
        disc = b * b - ((oc * oc).sum(-1) - rad * rad)
        with np.errstate(invalid="ignore"):
            sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
        for t in (-b - sq, -b + sq):
            better = (disc >= 0) & (t > 1e-3) & (t < t_best)
            t_best, i_best = np.where(better, t, t_best), np.where(better, i, i_best)
    return t_best, i_best


@pytest.mark.parametrize("model,size", [("equirect", (96, 48)), ("fisheye", (64, 64))])
def test_reprojection_lands_on_the_same_sphere(rt3, model, size):
    """scene_three_spheres from two poses, traced in float64 against the analytic spheres: a hit pixel of pose B, carried by the f32 inverse law
    into pose A's frame, lands on a pixel that shows the same sphere wherever A's 3 x 3 neighbourhood there is of one sphere."""
    w, h = size
    cr, _ = rt3.scene_three_spheres()
    at = (0.0, 0.0, -1.0)
    lens_a = rt3.make_lens(model, (0.0, 0.3, 1.0), at, fov_deg=160.0)
    lens_b = rt3.make_lens(model, (0.25, 0.35, 0.9), at, (0.05, 1.0, 0.0), fov_deg=160.0)
    index, depth = {}, {}
    for name, lens in (("a", lens_a), ("b", lens_b)):
        o, d = O.centre_rays(lens, w, h)
        t, i = trace64(cr.reshape(-1, 4), o.reshape(-1, 3).astype(np.float64), d.reshape(-1, 3).astype(np.float64))
        index[name], depth[name] = i.reshape(h, w), t.reshape(h, w)
    z = depth["b"].astype(F)
    view, ok, xp, yp = O.reproject(lens_b, lens_a, w, h, z)
    hit = index["b"] >= 0
    qx, qy = np.floor(xp + F(0.5)).astype(np.int64), np.floor(yp + F(0.5)).astype(np.int64)
    if model == "equirect":
        qx = np.mod(qx, w)
    inside = hit & ok & (qx >= 1) & (qx < w - 1) & (qy >= 1) & (qy < h - 1)
    ia = index["a"]
    uniform = np.ones((h, w), bool)
    cx, cy = np.clip(qx, 1, w - 2), np.clip(qy, 1, h - 2)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            uniform &= ia[cy + dy, cx + dx] == ia[cy, cx]
    checked = inside & uniform
    share = checked.sum() / hit.sum()
    print("%s %dx%d: %d hit pixels of pose B, %.3f of them checked" % (model, w, h, hit.sum(), share))
    assert share >= 0.5
    assert np.array_equal(ia[cy, cx][checked], index["b"][checked])
    za = depth["a"][cy, cx][checked]
    assert (np.abs(za - view.zhat[checked]) <= 0.05 * za + 0.05).mean() > 0.9       # and mostly at the depth the history would hold
