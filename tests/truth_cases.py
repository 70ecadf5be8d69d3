"""Scenes, rays and comparison helpers shared by the two sources that are held against tests/truth_ref.py: the CPU oracle
(tests/test_truth_ref.py) and the kernels (tests/test_gpu_truth.py).  Nothing here knows which of the two produced an answer.

A source is described by callables: make_triangle(p1, p2, p3) -> (GFACE[1], verts (3, 4)) and merge([(faces, verts), ...]) for the product's
or the oracle's own pre-render (the stored normals are theirs), and per check a function that returns the answers to compare."""
import numpy as np

import truth_ref as T

MAT_FLAT, MAT_LAMBERT, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2, 3
MATERIAL = np.dtype([("rgb", "<f4", 3), ("param", "<f4"), ("kind", "<u4")])
FLAG_BLACK = 2
BLACK = 0x000000FF                                                     # pack_pixel(0, 0, 0)

REGIMES = [(1.0, 0.0), (1.0, 300.0), (1000.0, 0.0), (0.01, 30.0)]    # (scale, offset) of the coordinates
SCENES = {"spheres300": (300, 0), "mixed64": (64, 64), "mixed700": (700, 700)}
AXIS = np.array([0.6, 0.3, -0.74]) / np.linalg.norm([0.6, 0.3, -0.74])
N_RAYS = 4096
AMBIGUOUS_CAP = 0.01
SPECULAR_CAP = 0.05
# t_min of the specular scenes: a scattered ray starts on the surface it left, uncertain by the first ray's propagated error (about 1e-4 of
# the scene's size near grazing incidence); its second meeting with that surface must stay clear of t_min.  Every target is more than 1 away.
SPECULAR_T_MIN = 0.01


def t_min_of(scale, offset):
    """0.001 scale, but at least 2^-15 of the offset: a ray that starts on a surface meets that surface again at |t| of the order of its
    error_bound_t, about 14u M / cos = 2^-18 M for M = the offset and cos >= 0.43; t_min stays eight times above that."""
    return np.float32(max(1e-3 * scale, 2.0 ** -15 * offset))


# ====================================================================================================================== cameras
class Cam:
    """The four camera vectors as float32 tuples (the fields of rt3_camera)."""

    def __init__(self, origin, horizontal, vertical, lower_left_corner):
        f = lambda v: tuple(float(np.float32(x)) for x in v)             # noqa: E731
        self.origin, self.horizontal, self.vertical, self.lower_left_corner = f(origin), f(horizontal), f(vertical), f(lower_left_corner)

    def struct(self, cls):
        c = cls()
        for name in ("origin", "horizontal", "vertical", "lower_left_corner"):
            setattr(c, name, getattr(self, name))
        return c


def look_at(width, height, look_from, at, vfov_deg, vup=(0.0, 1.0, 0.0), focus=1.0):
    """A look-from / look-at camera as four vectors; any four vectors define a camera, so this need not repeat the product's arithmetic."""
    look_from, at, vup = (np.asarray(v, np.float64) for v in (look_from, at, vup))
    vh = 2.0 * np.tan(np.radians(vfov_deg) / 2.0) * focus
    vw = vh * width / height
    w = (look_from - at) / np.linalg.norm(look_from - at)
    u = np.cross(vup, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    hor, ver = vw * u, vh * v
    return Cam(look_from, hor, ver, look_from - hor / 2 - ver / 2 - focus * w)


class Params:
    """The fields of rt3_params the reference reads."""

    def __init__(self, width, height, spp=1, max_depth=1, seed=1, flags=0, lens_radius=0.0, t_min=0.001, tile_rows=8, tile_index=0, tile_count=1):
        self.width, self.height, self.spp, self.max_depth, self.seed, self.flags = width, height, spp, max_depth, seed, flags
        self.lens_radius, self.t_min = float(np.float32(lens_radius)), float(np.float32(t_min))
        self.tile_rows, self.tile_index, self.tile_count = tile_rows, tile_index, tile_count

    def kwargs(self):
        return dict(self.__dict__)


def material(kind, rgb, param=0.0):
    m = np.zeros(1, MATERIAL)
    m["rgb"][0], m["param"][0], m["kind"][0] = rgb, param, kind
    return m


# ====================================================================================================================== (a) scenes and rays
def unit(rng, n):
    v = rng.normal(0.0, 1.0, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def soup(rng, n_spheres, n_faces, scale, offset, make_triangle, merge):
    """Random spheres and triangles in a box around offset * AXIS; the box grows with the count so the density stays that of 128 primitives
    in a box of 10 scale."""
    half = 5.0 * scale * max(1.0, ((n_spheres + n_faces) / 128.0) ** (1.0 / 3.0))
    c0 = offset * AXIS
    sph = np.concatenate([c0 + rng.uniform(-half, half, (n_spheres, 3)), rng.uniform(0.2, 0.8, (n_spheres, 1)) * scale], axis=1).astype(np.float32)
    faces = verts = None
    if n_faces:
        parts = []
        for _ in range(n_faces):
            c = c0 + rng.uniform(-half, half, 3)
            while True:
                p = rng.uniform(-1.0, 1.0, (3, 3)) * scale
                e1, e2 = p[1] - p[0], p[2] - p[0]
                if np.linalg.norm(np.cross(e1, e2)) > 0.3 * np.linalg.norm(e1) * np.linalg.norm(e2):      # no slivers: they only inflate the bounds
                    break
            parts.append(make_triangle(*(c + p)))
        faces, verts = merge(parts)
    return dict(spheres=sph if n_spheres else None, faces=faces, verts=verts, half=half, c0=c0, scale=scale, offset=offset)


def _f32_unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def soup_rays(rng, sc, n=N_RAYS):
    """Three classes: n/2 camera-like rays from outside the box aimed into it; n/4 that start on a primitive's surface and leave it at
    cos >= 0.43 (t_min must reject the surface itself); n/4 that start inside a sphere (the far root)."""
    half, c0, sph = sc["half"], sc["c0"], sc["spheres"]
    k = n // 4
    oA = c0 + unit(rng, 2 * k) * half * 2.5
    dA = c0 + rng.uniform(-half, half, (2 * k, 3)) - oA
    nB = k
    use_face = (rng.random(nB) < 0.5) if (sc["faces"] is not None and sph is not None) else np.full(nB, sc["faces"] is not None)
    oB, dB = np.zeros((nB, 3)), np.zeros((nB, 3))
    if use_face.any():
        m = int(use_face.sum())
        f = sc["faces"][rng.integers(0, len(sc["faces"]), m)]
        v = np.asarray(sc["verts"], np.float64)
        p1, p2, p3 = v[f["v1"], :3], v[f["v2"], :3], v[f["v3"], :3]
        w = rng.dirichlet([1.0, 1.0, 1.0], m) * 0.7 + 0.1              # barycentric weights >= 0.1
        oB[use_face] = w[:, :1] * p1 + w[:, 1:2] * p2 + w[:, 2:] * p3
        nn = np.cross(p2 - p1, p3 - p1)
        nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        dB[use_face] = nn * rng.choice([-1.0, 1.0], (m, 1)) + 0.9 * unit(rng, m)
    if (~use_face).any():
        m = int((~use_face).sum())
        s = sph[rng.integers(0, len(sph), m)].astype(np.float64)
        nn = unit(rng, m)
        oB[~use_face] = s[:, :3] + s[:, 3:4] * nn
        dB[~use_face] = nn + 0.9 * unit(rng, m)
    nC = n - 2 * k - nB
    s = sph[rng.integers(0, len(sph), nC)].astype(np.float64)
    oC = s[:, :3] + s[:, 3:4] * rng.uniform(0.0, 0.8, (nC, 1)) * unit(rng, nC)
    dC = unit(rng, nC)
    o = np.concatenate([oA, oB, oC]).astype(np.float32)
    d = _f32_unit(np.concatenate([dA, dB, dC]))
    cls = np.concatenate([np.zeros(2 * k, int), np.ones(nB, int), np.full(nC, 2)])
    return o, d, cls


def draw_t_max(seed, t_min):
    """nearest_hit's t_max function: half of the rays get a finite t_max around the true t (0.5 to 1.5 times it; between 0 and twice the
    median hit where nothing is hit), rounded to float32 and kept above 4 t_min (a ray with t_max <= t_min is invalid)."""
    def draw(sl, t_open):
        rng = np.random.default_rng([seed, sl.start])
        n = len(t_open)
        fin = np.isfinite(t_open)
        t = np.where(fin, t_open, 2.0 * np.median(t_open[fin]) if fin.any() else 1.0)
        tm = np.maximum(t * rng.uniform(0.5, 1.5, n), 4.0 * float(t_min)).astype(np.float32)
        return np.where(rng.random(n) < 0.5, tm, np.float32(np.inf)).astype(np.float32)
    return draw


def hit_case(make_triangle, merge, scene, regime):
    """Scene, rays and truth of one case of check (a): (scene, origins, directions, ray class, t_min, nearest_hit's record with t_max)."""
    ns, nf = SCENES[scene]
    scale, offset = REGIMES[regime]
    rng = np.random.default_rng([ns, nf, regime])
    sc = soup(rng, ns, nf, scale, offset, make_triangle, merge)
    o, d, cls = soup_rays(rng, sc)
    t_min = t_min_of(scale, offset)
    ref = T.nearest_hit(o, d, t_min, draw_t_max(regime, t_min), sc["spheres"], sc["faces"], sc["verts"])
    return sc, o, d, cls, t_min, ref


AOV_SIZE = (64, 48)


def aov_case(make_triangle, merge, regime):
    """Check (c): the 64 + 64 scene of a regime seen by a camera outside its box, spp 1."""
    scale, offset = REGIMES[regime]
    rng = np.random.default_rng([64, 64, regime])
    sc = soup(rng, 64, 64, scale, offset, make_triangle, merge)
    w, h = AOV_SIZE
    eye = sc["c0"] + 2.5 * sc["half"] * np.array([0.48, 0.6, 0.64])
    return sc, look_at(w, h, eye, sc["c0"], 40.0, focus=2.5 * sc["half"]), Params(w, h, t_min=t_min_of(scale, offset))


def aov_truth(sc, p, origins, directions):
    """Truth for the AOVs of the exported primary rays (float32, promoted exactly): a camera far from the origin loses direction bits to the
    cancellation llc - org, which check (b)'s bound counts once, on the rays; the hit is then judged on the rays the kernel really traced."""
    return T.nearest_hit(origins, directions, p.t_min, np.inf, sc["spheres"], sc["faces"], sc["verts"])


# ====================================================================================================================== comparison helpers
def check_hits(ref, kind, index, t, occluded=None, cap=AMBIGUOUS_CAP):
    """kind, index and t of a source against nearest_hit's record on every non-ambiguous ray.  Returns the figures."""
    kind, index = np.asarray(kind, np.uint32), np.asarray(index, np.uint32)
    t = np.asarray(t, np.float64)
    amb = ref["ambiguous"]
    ok = ~amb
    assert amb.mean() <= cap, "%d of %d rays ambiguous: the inputs are wrong" % (int(amb.sum()), len(amb))
    bad = ok & ((kind != ref["kind"]) | (index != ref["index"]))
    assert not bad.any(), "%d rays name another primitive, first %s" % (int(bad.sum()), [
        (int(i), int(kind[i]), int(index[i]), float(t[i]), int(ref["kind"][i]), int(ref["index"][i]), float(ref["t"][i]))
        for i in np.nonzero(bad)[0][:3]])
    hit = ok & (ref["kind"] != T.NONE)
    miss = ok & (ref["kind"] == T.NONE)
    assert np.isposinf(t[miss]).all() and (index[miss] == T.NO_INDEX).all(), "a miss is {+inf, NONE, 0xFFFFFFFF}"
    with np.errstate(invalid="ignore"):
        ratio = np.abs(t[hit] - ref["t"][hit]) / ref["t_bound"][hit]
    assert np.isfinite(t[hit]).all()
    worst = float(ratio.max()) if hit.any() else 0.0
    rel = float((np.abs(t[hit] - ref["t"][hit]) / ref["t"][hit]).max() / T.U) if hit.any() else 0.0
    assert worst <= 1.0, "|t - t64| reaches %.2f of error_bound_t" % worst
    if occluded is not None:
        assert np.array_equal(np.asarray(occluded)[ok] != 0, ref["kind"][ok] != T.NONE), "occlusion differs from kind != NONE"
    return dict(compared=int(ok.sum()), ambiguous=int(amb.sum()), hits=int(hit.sum()), max_ratio=worst, max_rel_u=rel)


def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = np.linalg.norm(np.cross(a, b), axis=-1)
    return np.arctan2(c, (a * b).sum(axis=-1))


def check_normals(ref, normals, directions, select=None):
    """Shading normals against the float64 geometric normal: within normal_bound of it, facing the ray."""
    ok = ~ref["ambiguous"] & (ref["kind"] != T.NONE)
    if select is not None:
        ok &= select
    n = np.asarray(normals, np.float64)
    d = np.asarray(directions, np.float64)
    facing = (n[ok] * d[ok]).sum(axis=1) < 0
    assert facing.all(), "%d normals face away from their ray" % int((~facing).sum())
    ratio = angle(n[ok], ref["normal"][ok]) / ref["normal_bound"][ok]
    worst = float(ratio.max()) if ok.any() else 0.0
    assert worst <= 1.0, "a normal is %.2f of its bound from the float64 normal" % worst
    return dict(compared=int(ok.sum()), max_ratio=worst)


def check_cosine(mean, F, albedo_c, spp, sigmas=6.0):
    """Per-pixel linear mean against albedo * c * F with sigma^2 = (albedo c)^2 F (1 - F) / spp."""
    mean, F = np.asarray(mean, np.float64), np.asarray(F, np.float64)
    sigma = albedo_c * np.sqrt(F * (1.0 - F) / spp)
    z = (mean - albedo_c * F) / sigma
    worst = float(np.abs(z).max())
    assert worst <= sigmas, "a pixel is %.1f sigma from the cosine law" % worst
    return dict(compared=int(z.size), max_z=worst)


def check_frame(pixels, allowed, skip, cap=SPECULAR_CAP):
    """Every pixel outside skip shows one of its allowed packed colours (allowed: (k, n) uint32).  Returns which alternative each pixel shows."""
    pixels = np.asarray(pixels, np.uint32).reshape(-1)
    assert skip.mean() <= cap, "%d of %d pixels skipped" % (int(skip.sum()), len(skip))
    match = allowed == pixels[None]
    bad = ~skip & ~match.any(axis=0)
    assert not bad.any(), "%d pixels show another colour, first %s" % (int(bad.sum()), [
        (int(i), hex(int(pixels[i])), [hex(int(a)) for a in allowed[:, i]]) for i in np.nonzero(bad)[0][:3]])
    return np.argmax(match, axis=0)


def check_count(count, probabilities, sigmas=6.0):
    """A count of independent events against the sum of their probabilities, variance sum p (1 - p)."""
    p = np.asarray(probabilities, np.float64)
    sigma = np.sqrt((p * (1.0 - p)).sum())
    z = (count - p.sum()) / sigma
    assert abs(z) <= sigmas, "%d events where %.1f +- %.1f are expected" % (count, p.sum(), sigma)
    return float(z)


def check_glass(pixels, ex, need_tir=False, cap=SPECULAR_CAP):
    """A frame through the dielectric against specular_frame's record: every pixel its reflected or its refracted target; the number of
    reflected pixels within 6 sigma of the sum of the reflectances; beyond the critical angle the reflected target only."""
    pixels = np.asarray(pixels, np.uint32).reshape(-1)
    glass = ex["specular"]
    same = ex["allowed"][0] == ex["allowed"][1]
    skip = ex["skip"] | (glass & same & ~ex["tir"])                    # the two colours coincide: the pixel cannot tell
    which = check_frame(pixels, ex["allowed"], skip, cap)
    counted = glass & ~skip & ~ex["tir"]
    reflected = int((which[counted] == 0).sum())
    z = check_count(reflected, ex["R"][counted])
    total = glass & ex["tir"] & ~skip
    if need_tir:
        assert total.sum() > 0, "no pixel beyond the critical angle"
    assert (pixels[total] == ex["allowed"][0][total]).all(), "a pixel beyond the critical angle does not show the reflected target"
    return dict(compared=int((~skip).sum()), skipped=int(skip.sum()), counted=int(counted.sum()), reflected=reflected,
                expected=float(ex["R"][counted].sum()), z=z, total_reflection=int(total.sum()))


def shading_normals(ref, origins, directions, t, spheres, faces):
    """The normals of DESIGN.md 4.10 from a source's own t and stored face normals, in float32: the stored face normal, or
    (fma(t, d, o) - C) * (1 / r), flipped unless d.n < 0."""
    o, d = np.asarray(origins, np.float32), np.asarray(directions, np.float32)
    n = np.zeros((len(o), 3), np.float32)
    f = ref["kind"] == T.FACE
    if f.any():
        n[f] = faces["normal"][ref["index"][f]]
    s = ref["kind"] == T.SPHERE
    if s.any():
        c = spheres[ref["index"][s]]
        p = (np.asarray(t, np.float32)[s, None].astype(np.float64) * d[s] + o[s]).astype(np.float32)
        n[s] = (p - c[:, :3]) * (np.float32(1.0) / c[:, 3:4])
    away = (n.astype(np.float64) * d).sum(axis=1) >= 0
    n[away] = -n[away]
    return n


# ====================================================================================================================== (b) camera rays
CAMERA_CASES = [(33, 17, 1, 0.0, None), (33, 17, 9, 0.05, None), (64, 36, 9, 0.0, None), (64, 36, 1, 0.05, None), (64, 36, 9, 0.05, (4, 1, 3)),
                (33, 17, 1, 0.05, None), (33, 17, 9, 0.0, None), (64, 36, 1, 0.0, None)]


def camera_case(w, h, spp, lens, tile):
    cam = look_at(w, h, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, focus=10.0)
    kw = dict(tile_rows=tile[0], tile_index=tile[1], tile_count=tile[2]) if tile else {}
    return cam, Params(w, h, spp=spp, seed=11, lens_radius=lens, **kw)


def expected_camera_rays(cam, p, hash_words=None):
    """camera_ray for every owned pixel and sample, in rt3_camera_rays' order (sample-major); hash_words(words) -> the exported hash of
    those words, checked against truth_ref's on the keys in use."""
    ys = T.owned_rows(p)
    xx, yy = np.meshgrid(np.arange(p.width), ys)
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    O, D, L = [], [], []
    for s in range(p.spp):
        jit, lens, base = T.camera_samples(p.width, p.spp, p.seed, xx, yy, np.full(len(xx), s))
        if hash_words is not None and s == 0:
            words = np.concatenate([base[:64], (yy * p.width + xx).astype(np.uint32)[:64], np.arange(5, dtype=np.uint32)])
            assert np.array_equal(hash_words(words), T.hash_u32(words)), "the exported hash is not the documented one"
        o, d, ln = T.camera_ray(cam, p, xx, yy, jit, lens)
        O.append(o); D.append(d); L.append(ln)
    return np.concatenate(O), np.concatenate(D), np.concatenate(L)


def check_camera_rays(cam, p, origins, directions, exp):
    eo, ed, ln = exp
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    assert o.shape == eo.shape
    if p.lens_radius > 0:
        r_o = np.linalg.norm(o - eo, axis=1) / T.error_bound_origin(cam, p.lens_radius)
    else:
        r_o = np.where((o == eo).all(axis=1), 0.0, np.inf)           # a pinhole's origin is the camera's, exactly
    r_d = angle(d, ed) / T.error_bound_dir(cam, p.width, p.height, ln, p.lens_radius)
    assert r_o.max() <= 1.0, "an origin is %.2f of its bound from the lens point" % r_o.max()
    assert r_d.max() <= 1.0, "a direction is %.2f of error_bound_dir off" % r_d.max()
    assert (np.abs((d * d).sum(axis=1) - 1.0) <= 2.0 ** -20).all()
    return dict(compared=len(o), max_origin_ratio=float(r_o.max()), max_dir_ratio=float(r_d.max()))


# ====================================================================================================================== (d) cosine law
COSINE = dict(albedo=0.8, c=2.0, R=1.0, centre=(0.0, 2.0, 0.0), size=12, spp=4096)


def cosine_scene(ground, make_triangle=None, merge=None):
    """A Lambert ground (a sphere of r = 1000 below y = 0, or two triangles in y = 0) under one FLAT sphere, R = 1, centre 2 above it."""
    a, c = COSINE["albedo"], COSINE["c"]
    if ground == "sphere":
        sph = np.array([[0.0, -1000.0, 0.0, 1000.0], list(COSINE["centre"]) + [COSINE["R"]]], np.float32)
        sm = np.concatenate([material(MAT_LAMBERT, (a, a, a)), material(MAT_FLAT, (c, c, c))])
        return dict(spheres=sph, smats=sm, faces=None, verts=None, fmats=None)
    q = [(-60.0, 0.0, -60.0), (60.0, 0.0, -60.0), (60.0, 0.0, 60.0), (-60.0, 0.0, 60.0)]
    faces, verts = merge([make_triangle(q[0], q[2], q[1]), make_triangle(q[0], q[3], q[2])])
    sph = np.array([list(COSINE["centre"]) + [COSINE["R"]]], np.float32)
    return dict(spheres=sph, smats=material(MAT_FLAT, (c, c, c)), faces=faces, verts=verts, fmats=np.repeat(material(MAT_LAMBERT, (a, a, a)), 2))


def cosine_camera():
    n = COSINE["size"]
    return look_at(n, n, (4.0, 2.0, 4.0), (0.3, 0.0, 0.2), 12.0), Params(n, n, spp=COSINE["spp"], max_depth=2, seed=5, flags=FLAG_BLACK)


def cosine_expectation(sc, origins, directions, spp):
    """Per pixel, the mean over its samples' primary rays (sample-major) of the emitter's form factor at each ray's hit point.  Asserts in
    float64 that no primary ray meets the emitter and (form_factor_sphere) that the emitter lies above every hit point's horizon."""
    rec = T.nearest_hit(origins, directions, 0.001, np.inf, sc["spheres"], sc["faces"], sc["verts"], chunk=1 << 16)
    emitter = len(sc["spheres"]) - 1
    assert (rec["kind"] != T.NONE).all() and not ((rec["kind"] == T.SPHERE) & (rec["index"] == emitter)).any()
    p = np.asarray(origins, np.float64) + rec["t"][:, None] * np.asarray(directions, np.float64)
    F = T.form_factor_sphere(p, rec["normal"], COSINE["centre"], COSINE["R"])
    return F.reshape(spp, -1).mean(axis=0)


def uniform_hemisphere_fraction(sc, origins, directions, spp):
    """The mutant's expectation: the emitter's share of a uniformly sampled hemisphere, solid angle / 2 pi = 1 - sqrt(1 - (R / D)^2)."""
    rec = T.nearest_hit(origins, directions, 0.001, np.inf, sc["spheres"], sc["faces"], sc["verts"], chunk=1 << 16)
    p = np.asarray(origins, np.float64) + rec["t"][:, None] * np.asarray(directions, np.float64)
    D = np.linalg.norm(np.asarray(COSINE["centre"])[None] - p, axis=1)
    return (1.0 - np.sqrt(1.0 - (COSINE["R"] / D) ** 2)).reshape(spp, -1).mean(axis=0)


# ====================================================================================================================== (e), (f) specular frames
def colour_code(k):
    """Target k's colour as three byte values, all non-zero and distinct per k < 1000 (decimal digits + 1, times 25), and as the rgb the
    scene stores."""
    b = np.array([(k % 10 + 1) * 25, ((k // 10) % 10 + 1) * 25, ((k // 100) % 10 + 1) * 25], np.uint32)
    return b, (b / 255.0).astype(np.float32)


def packed(b):
    return np.uint32(0xFF | (int(b[2]) << 8) | (int(b[1]) << 16) | (int(b[0]) << 24))


def mirror_scene(seed=3, n_targets=200):
    """One METAL sphere (fuzz 0, albedo 1) of radius 1 at the origin inside a shell (radius 4) of colour-coded FLAT spheres of radius 0.3."""
    rng = np.random.default_rng(seed)
    k = np.arange(n_targets) + 0.5
    phi, th = np.arccos(1.0 - 2.0 * k / n_targets), np.pi * (1.0 + 5.0 ** 0.5) * k               # a Fibonacci lattice: even gaps
    c = 4.0 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1) + rng.uniform(-0.05, 0.05, (n_targets, 3))
    sph = np.concatenate([[[0.0, 0.0, 0.0, 1.0]], np.concatenate([c, np.full((n_targets, 1), 0.3)], axis=1)]).astype(np.float32)
    sm = np.concatenate([material(MAT_METAL, (1.0, 1.0, 1.0), 0.0)] + [material(MAT_FLAT, colour_code(i)[1]) for i in range(n_targets)])
    codes = np.array([BLACK] + [packed(colour_code(i)[0]) for i in range(n_targets)], np.uint32)
    cam = look_at(48, 48, (1.6, 0.9, 2.0), (0.0, 0.0, 0.0), 50.0)
    return (dict(spheres=sph, smats=sm, faces=None, verts=None, fmats=None, sphere_codes=codes), cam,
            Params(48, 48, max_depth=2, seed=2, flags=FLAG_BLACK, t_min=SPECULAR_T_MIN))


def glass_scene(make_triangle, merge, back):
    """One large DIELECTRIC triangle (ior 1.5) in z = 0 between two walls of colour-coded FLAT spheres; the camera looks at it at 50 to 70
    degrees of incidence from the front (z > 0), or at 30 to 60 degrees from behind, where part of the frame is beyond the critical angle."""
    faces, verts = merge([make_triangle((-40.0, -30.0, 0.0), (0.0, 50.0, 0.0), (40.0, -30.0, 0.0))])      # stored normal +z: z > 0 is the front
    cs = []
    for z in (3.0, -3.0):
        for ix in range(-10, 11):
            for iy in range(-5, 6):
                cs.append([1.2 * ix + 0.3 * (iy % 2), 1.2 * iy, z + np.sign(z) * 0.3 * ((ix + iy) % 3), 0.85])
    sph = np.array(cs, np.float32)
    sm = np.concatenate([material(MAT_FLAT, colour_code(i)[1]) for i in range(len(sph))])
    codes = np.array([packed(colour_code(i)[0]) for i in range(len(sph))], np.uint32)
    if back:
        cam = look_at(48, 48, (1.9, 0.3, -2.0), (0.0, 0.0, 0.0), 28.0)
    else:
        cam = look_at(48, 48, (3.4, 0.5, 2.0), (0.0, 0.0, 0.0), 20.0)
    return (dict(spheres=sph, smats=sm, faces=faces, verts=verts, fmats=material(MAT_DIELECTRIC, (1.0, 1.0, 1.0), 1.5), sphere_codes=codes), cam,
            Params(48, 48, max_depth=2, seed=9 if back else 4, flags=FLAG_BLACK, t_min=SPECULAR_T_MIN))


def specular_frame(sc, cam, p, mutate=None):
    """What a spp-1, max_depth-2 frame of a scene of FLAT targets and one specular primitive must show, traced in float64: per pixel the
    allowed packed colours ((2, n): the reflected and the refracted alternative; equal where there is only one), the pixels to skip
    (ambiguous at either ray, by the margins with the first ray's error propagated into the second), and for a dielectric the reflectance
    R and the total-internal-reflection mask.  mutate: 'reflect_sign' / 'ri_inverted' build a deliberately wrong frame."""
    ys = T.owned_rows(p)
    xx, yy = np.meshgrid(np.arange(p.width), ys)
    o, d, ln = T.camera_ray(cam, p, xx.reshape(-1), yy.reshape(-1))
    n = len(o)
    e_o = T.error_bound_origin(cam) if p.lens_radius > 0 else 0.0
    e_d = T.error_bound_dir(cam, p.width, p.height, ln)
    args = (sc["spheres"], sc["faces"], sc["verts"])
    h0 = T.nearest_hit(o, d, p.t_min, np.inf, *args, origin_err=e_o, dir_err=e_d)
    codes = sc["sphere_codes"]
    skinds = sc["smats"]["kind"]
    skip = h0["ambiguous"].copy()
    allowed = np.full((2, n), BLACK, np.uint32)
    R = np.zeros(n)
    tir = np.zeros(n, bool)
    specular = np.zeros(n, bool)
    issph = h0["kind"] == T.SPHERE
    si = np.where(issph, h0["index"], 0).astype(np.int64)
    flat = issph & (skinds[si] == MAT_FLAT)
    allowed[:, flat] = codes[si[flat]]
    mirror = issph & (skinds[si] == MAT_METAL)
    glass = h0["kind"] == T.FACE

    debug = []

    def second(sel, direction, dir_err, normal_err):
        """Colours and ambiguity of the rays that leave the pixels `sel` in `direction`."""
        t = h0["t"][sel]
        M = np.abs(o[sel] + t[:, None] * d[sel]).max(axis=1)
        p_err = e_o + t * e_d[sel] + h0["t_bound"][sel] + T.SQRT3 * T.U * M
        h1 = T.nearest_hit(o[sel] + t[:, None] * d[sel], direction, p.t_min, np.inf, *args, origin_err=p_err, dir_err=dir_err)
        i1 = np.where(h1["kind"] == T.SPHERE, h1["index"], 0).astype(np.int64)
        col = np.where((h1["kind"] == T.SPHERE) & (skinds[i1] == MAT_FLAT), codes[i1], BLACK)     # depth exhausted on anything else: black
        debug.append(h1)
        return col.astype(np.uint32), h1["ambiguous"]

    if mirror.any():
        nrm = h0["normal"][mirror]
        n_err = h0["normal_bound"][mirror] + (e_o + h0["t"][mirror] * e_d[mirror]) / sc["spheres"][si[mirror], 3]
        rd = T.reflect(d[mirror], nrm) if mutate != "reflect_sign" else d[mirror] + 2.0 * (d[mirror] * nrm).sum(axis=1, keepdims=True) * nrm
        col, amb = second(mirror, rd, T.reflect_error(e_d[mirror], n_err), n_err)
        allowed[:, mirror] = col
        skip[mirror] |= amb
        specular |= mirror
    if glass.any():
        nrm = h0["normal"][glass]
        n_err = h0["normal_bound"][glass]
        ior = float(sc["fmats"]["param"][0])
        g = np.asarray(sc["verts"], np.float64)
        gn = np.cross(g[1, :3] - g[0, :3], g[2, :3] - g[0, :3])
        stored_outward = -gn / np.linalg.norm(gn)                     # the pre-render stores MINUS the normalised (p2 - p1) x (p3 - p1)
        front = (d[glass] * stored_outward).sum(axis=1) < 0
        ri = np.where(front, 1.0 / ior, ior)
        if mutate == "ri_inverted":
            ri = 1.0 / ri
        cos_in = -(d[glass] * nrm).sum(axis=1)
        fd, total = T.refract(d[glass], nrm, ri)
        cos_out = np.where(total, 1.0, np.sqrt(np.maximum(1.0 - ri * ri * (1.0 - cos_in ** 2), 0.0)))
        col_r, amb_r = second(glass, T.reflect(d[glass], nrm), T.reflect_error(e_d[glass], n_err), n_err)
        fd = np.where(total[:, None], T.reflect(d[glass], nrm), fd)
        f_err = np.where(total, T.reflect_error(e_d[glass], n_err), T.refract_error(e_d[glass], n_err, ri, cos_in, np.maximum(cos_out, 1e-12)))
        col_f, amb_f = second(glass, fd, f_err, n_err)
        col_f = np.where(total, col_r, col_f)
        allowed[0, glass], allowed[1, glass] = col_r, col_f
        skip[glass] |= amb_r | (amb_f & ~total)
        near_critical = np.abs(ri * np.sqrt(np.maximum(1.0 - cos_in ** 2, 0.0)) - 1.0) < 64.0 * T.U + 2.0 * ri * (e_d[glass] + n_err)
        skip[glass] |= near_critical
        R[glass] = np.where(total, 1.0, T.schlick(cos_in, ri))
        tir[glass] = total
        specular |= glass
    return dict(allowed=allowed, skip=skip, R=R, tir=tir, specular=specular, primary=h0, secondary=debug)


def pixel_grid(p):
    xx, yy = np.meshgrid(np.arange(p.width), T.owned_rows(p))
    return xx.reshape(-1), yy.reshape(-1)


# ====================================================================================================================== (g) the integrating sphere
# (r, R, albedo, E, max_depth): the first geometry at four depths, a second one at depth 12
INTEGRATING = [(1.0, 2.0, 0.8, 3.0, 2), (1.0, 2.0, 0.8, 3.0, 3), (1.0, 2.0, 0.8, 3.0, 8), (1.0, 2.0, 0.8, 3.0, 30), (1.0, 4.0, 0.6, 5.0, 12)]
INTEGRATING_IDS = ["R2_D2", "R2_D3", "R2_D8", "R2_D30", "R4_D12"]
INTEGRATING_SIZE = (48, 32, 256)
EMITTER, WALL, SHELL = 0, 1, 2


def integrating_scene(r, R, albedo, E):
    """A FLAT sphere (r, radiance E) at the centre of a Lambert sphere (R, albedo a), and a second Lambert sphere of the same albedo
    2^-10 R outside it.  The outer shell is for float32, not for the law: a scattered ray that leaves the wall at a grazing angle meets the
    wall again at a t of the order of t_min and can lose that root to rounding (tests/test_gpu_env_sampling.py counts 3 such rays in
    10 000); without the shell it would escape into the black background, with it it scatters on from a point 2^-10 R further out, where
    F differs by 0.2 %.  At R = 2 the shell changed no bit of the oracle's frame; it stays so that the law holds for the next scene too."""
    sph = np.array([[0.0, 0.0, 0.0, r], [0.0, 0.0, 0.0, R], [0.0, 0.0, 0.0, R * (1.0 + 2.0 ** -10)]], np.float32)
    sm = np.concatenate([material(MAT_FLAT, (E, E, E)), material(MAT_LAMBERT, (albedo,) * 3), material(MAT_LAMBERT, (albedo,) * 3)])
    return dict(spheres=sph, smats=sm, faces=None, verts=None, fmats=None)


def integrating_camera(r, R, max_depth, size=INTEGRATING_SIZE, seed=7, flags=FLAG_BLACK, inward=False):
    """Between the emitter and the wall, looking outward (every sample meets the wall first); inward: at the emitter, for the pixels on it."""
    w, h, spp = size
    eye = np.array([0.3, 0.2, 0.5])
    eye = eye / np.linalg.norm(eye) * 0.5 * (r + R)
    return (look_at(w, h, eye, (0.0, 0.0, 0.0) if inward else 2.0 * eye, 40.0),
            Params(w, h, spp=spp, max_depth=max_depth, seed=seed, flags=flags))


def all_meet_the_wall(kind, index):
    return bool(((np.asarray(kind) == T.SPHERE) & (np.asarray(index) == WALL)).all())


def check_integrating(law, mean, n_pixel, casts_per_sample=None, max_depth=None, each=True, sigmas=6.0):
    """Values (linear means over n_pixel samples each, any shape) against integrating_sphere's law: the mean of all within 6 sigma /
    sqrt(all samples), each (a frame's pixels) within 6 sigma / sqrt(n_pixel); casts per sample within 6 ((D - 1) / 2) / sqrt(all samples)
    of the closed form — a path casts between 1 and D rays, and half that range bounds the standard deviation of any variable."""
    mean = np.asarray(mean, np.float64).reshape(-1)
    n = mean.size * n_pixel
    z = (mean.mean() - law["mean"]) / (law["sigma"] / np.sqrt(n))
    worst = float((np.abs(mean - law["mean"]) / (law["sigma"] / np.sqrt(n_pixel))).max())
    fig = dict(samples=int(n), mean=float(mean.mean()), expected=float(law["mean"]), z=float(z), worst_pixel=worst)
    assert abs(z) <= sigmas, "the mean %.6f is %.1f sigma from %.6f" % (mean.mean(), z, law["mean"])
    assert not each or worst <= sigmas, "a pixel is %.1f sigma from the closed form" % worst
    if casts_per_sample is not None:
        bound = sigmas * 0.5 * (max_depth - 1.0) / np.sqrt(n)
        fig.update(casts=float(casts_per_sample), casts_expected=law["casts"])
        assert abs(casts_per_sample - law["casts"]) <= bound, "%.5f casts per sample where %.5f +- %.5f are expected" % (
            casts_per_sample, law["casts"], bound)
    return fig


def integrating_rays(r, R, n, seed=21):
    """n rays that start between the emitter and the wall and move away from the centre (o.d >= 0.1 |o|): none can meet the emitter."""
    rng = np.random.default_rng(seed)
    radial = unit(rng, n)
    o = radial * rng.uniform(r + 0.1 * (R - r), R - 0.1 * (R - r), (n, 1))
    d = radial + 0.9 * unit(rng, n)
    return o.astype(np.float32), _f32_unit(d)


def light_sample_range(r, R, albedo, E, max_depth):
    """The largest value of a sample with a shadow ray to the emitter at every wall hit: sum over the wall hits j = 1 .. D - 1 of a^j E k,
    k = c c_l A / (pi d^2 p_l) with both cosines at most 1, A = 4 pi r^2, p_l = 1 (one light) and d >= R - r: k <= 4 r^2 / (R - r)^2."""
    j = np.arange(1, max_depth, dtype=np.float64)
    return E * 4.0 * r * r / (R - r) ** 2 * (albedo ** j).sum()


def check_range_mean(mean, expected, low, high, n, sigmas=6.0):
    """The mean of n independent samples that lie in [low, high] against its expectation: a variable confined to an interval has a
    standard deviation of at most half the interval's length."""
    bound = sigmas * 0.5 * (high - low) / np.sqrt(n)
    z = (mean - expected) / (0.5 * (high - low) / np.sqrt(n))
    assert abs(mean - expected) <= bound, "the mean %.6f is off %.6f by more than %.6f" % (mean, expected, bound)
    return dict(mean=float(mean), expected=float(expected), bound=float(bound), z_of_half_ranges=float(z))


# ====================================================================================================================== (h) metal fuzz
# rgb and c have few mantissa bits: the sum of 1024 equal samples is then exact in float32 (k rgb c needs 7 + 10 bits), and a pixel without
# absorption equals rgb c; with arbitrary values the running sum alone would round up to spp / 2 times
FUZZ = dict(rgb=(0.8125, 0.5625, 0.3125), c=2.5, size=(48, 32, 1024), fs=(1.0, 0.5, 0.2))


def fuzz_scene(ground, f, make_triangle=None, merge=None):
    """A METAL ground (two triangles in y = 0 whose stored normal points down, away from the camera; or a sphere of r = 1000 below y = 0)
    inside one FLAT sphere of radiance c and radius 60: every scattered ray that is not absorbed meets the emitter."""
    c = FUZZ["c"]
    metal = material(MAT_METAL, FUZZ["rgb"], f)
    if ground == "sphere":
        sph = np.array([[0.0, 0.0, 0.0, 60.0], [0.0, -1000.0, 0.0, 1000.0]], np.float32)
        return dict(spheres=sph, smats=np.concatenate([material(MAT_FLAT, (c, c, c)), metal]), faces=None, verts=None, fmats=None)
    q = [(-60.0, 0.0, -60.0), (60.0, 0.0, -60.0), (60.0, 0.0, 60.0), (-60.0, 0.0, 60.0)]
    faces, verts = merge([make_triangle(q[0], q[2], q[1]), make_triangle(q[0], q[3], q[2])])
    assert (faces["normal"][:, 1] < 0).all(), "the stored normals must point away from the camera"
    return dict(spheres=np.array([[0.0, 0.0, 0.0, 60.0]], np.float32), smats=material(MAT_FLAT, (c, c, c)), faces=faces, verts=verts,
                fmats=np.repeat(metal, 2))


def fuzz_camera(ground="triangles"):
    """One above the ground, looking along it: the cosine of incidence falls from 0.98 to 0.16 down the frame.

    t_min is 0.001 over the triangles and 0.5 over the sphere.  No surface of this scene is nearer than 1 to a ray's start (the camera's
    height; the emitter is 53 from the part of the ground in view), so any t_min below 1 leaves the truth as it is.  In float32 a ray that
    leaves the r = 1000 sphere meets it again at t = |dc| / (2 r cos), cos the cosine it leaves at and dc the error of c = |oc|^2 - r^2,
    up to 13.5u r^2 = 0.8 (5u (|oc|^2 + r^2) of its roundings, error_bound_disc, and 2 r times the hit point's sqrt(3) u r): 4e-4 / cos.
    With t_min = 0.001 that swallows the rays that leave within some degrees of the surface: measured on the oracle, 3.2 % of a pixel at
    f = 0.2 and the whole frame 13 sigma low at f = 1.  That is the reference's t_min at the radius of its own ground sphere, not a fault
    of the scatter law, which this scene is about; at 0.5 the frame is 0.7 sigma off."""
    w, h, spp = FUZZ["size"]
    return (Cam((0.0, 1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 0.0, -6.0), (-1.0, 0.0, -0.2)),
            Params(w, h, spp=spp, max_depth=2, seed=3, flags=FLAG_BLACK, t_min=0.5 if ground == "sphere" else 0.001))


def fuzz_cosines(sc, origins, directions, spp):
    """The cosine of incidence of every sample's primary ray on the ground, (spp, pixels); asserts that every ray meets the ground."""
    rec = T.nearest_hit(origins, directions, 0.001, np.inf, sc["spheres"], sc["faces"], sc["verts"], chunk=1 << 16)
    ground = (rec["kind"] == T.FACE) if sc["faces"] is not None else ((rec["kind"] == T.SPHERE) & (rec["index"] == 1))
    assert ground.all(), "a primary ray misses the ground"
    return (-(rec["normal"] * np.asarray(directions, np.float64)).sum(axis=1)).reshape(spp, -1)


def check_fuzz(mean, cos, f, absorption=T.fuzz_absorption, sigmas=6.0):
    """The linear frame (pixels, 3) against rgb c (1 - mean P(absorbed)) per pixel: within 6 sigma, sigma^2 = (rgb c)^2 q (1 - q) / spp with
    q the pixel's mean survival (the variance of a mean of Bernoulli draws of differing q_i is at most that); a pixel no sample of which
    can be absorbed equals rgb c to 4u relative.  exact counts the pixels whose every sample has cos > f (1 + 1e-4)."""
    mean = np.asarray(mean, np.float64).reshape(-1, 3)
    spp = cos.shape[0]
    q = 1.0 - absorption(cos, f).mean(axis=0)
    full = np.array(FUZZ["rgb"], np.float64) * FUZZ["c"]
    exact = (cos > f * (1.0 + 1e-4)).all(axis=0)
    sure = q == 1.0
    assert (sure | ~exact).all()
    stat = ~sure
    fig = dict(statistical=int(stat.sum()), exact=int(exact.sum()), max_z=0.0, frame_z=0.0)
    if sure.any():
        rel = np.abs(mean[sure] / full[None] - 1.0).max()
        assert rel <= 4.0 * T.U, "a pixel without absorption is %.3g off rgb c" % rel
    if stat.any():
        sigma = np.sqrt(q[stat] * (1.0 - q[stat]) / spp)
        z = (mean[stat] / full[None] - q[stat][:, None]) / sigma[:, None]
        fig["max_z"] = float(np.abs(z).max())
        fig["frame_z"] = float((mean[stat, 0] / full[0] - q[stat]).sum() / np.sqrt((sigma ** 2).sum()))
        assert fig["max_z"] <= sigmas, "a pixel is %.1f sigma from the absorption law" % fig["max_z"]
    return fig


def absorption_in_the_ball(cos, f):
    """Mutant: u uniform IN the unit ball; its component along n has the density 3 (1 - s^2) / 4, so P = 1/2 - 3x/4 + x^3/4, x = cos / f."""
    x = np.minimum(np.asarray(cos, np.float64) / f, 1.0)
    return 0.5 - 0.75 * x + 0.25 * x ** 3


def absorption_unscaled(cos, f):
    """Mutant: the fuzz vector not scaled by f."""
    return T.fuzz_absorption(cos, 1.0)


# ====================================================================================================================== (i) a glass sphere
GLASS_SPHERE_DEPTH = 6
GLASS_MIN_WEIGHT = 1e-3


def glass_sphere_scene():
    """mirror_scene's sphere and shell with the sphere DIELECTRIC (ior 1.5), 1 spp, max_depth 6.  A unit sphere is a strong lens: an error
    of a ray's direction moves its next hit on the sphere, the normal there turns with it, and a reflection doubles that, so a
    direction's bound grows about sixfold per interface (interface_gains).  With ior 1.5 the leaf 'enter, reflect, reflect, leave' weighs
    (1 - R)^2 R^2 >= 0.96^2 0.04^2 = 1.5e-3 in every pixel through the glass, above the 1e-3 from which a leaf counts, and meets its
    target after four interfaces.  So the tree starts from the primary rays the source itself traced (float32, promoted exactly; the
    primary ray has its own check, (b)) and not from a direction known to error_bound_dir only; the camera stands 1.8 from the centre
    (|oc| enters a sphere's error_bound_t, and it is the lever arm of the first hit); and t_min is 0.1: a ray that starts on the glass has
    a root at 0 that is uncertain by its origin's error (0.001 after four interfaces, times 1 + tan of the incidence in the bound), while
    the chords through the sphere are longer than 1.49 and the targets more than 2 away."""
    sc, _, _ = mirror_scene()
    sc["smats"] = sc["smats"].copy()
    sc["smats"]["kind"][0], sc["smats"]["param"][0] = MAT_DIELECTRIC, 1.5
    cam = look_at(48, 48, (1.0, 0.6, 1.37), (0.0, 0.0, 0.0), 70.0)
    return sc, cam, Params(48, 48, max_depth=GLASS_SPHERE_DEPTH, seed=6, flags=FLAG_BLACK, t_min=0.1)


def pinhole_rays_f32(cam, p):
    """The float32 primary rays of a spp-1 pinhole frame as DESIGN.md 4.1 forms them, every operation rounded to float32: u = x / (W - 1),
    v = (H - 1 - y) / (H - 1), dir = ((llc + u hor) + v ver) - org, d = dir * (1 / sqrt((x x + y y) + z z)).  For a source that does not
    export its rays; held against camera_ray by check_camera_rays where it is used."""
    f = np.float32
    xx, yy = pixel_grid(p)
    u = (xx.astype(f) / (f(p.width) - f(1.0)))[:, None]
    v = ((p.height - 1 - yy).astype(f) / (f(p.height) - f(1.0)))[:, None]
    org, hor, ver, llc = (np.array(getattr(cam, name), f)[None] for name in ("origin", "horizontal", "vertical", "lower_left_corner"))
    d = ((llc + u * hor) + v * ver) - org
    inv = f(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d * inv[:, None]
    assert d.dtype == f
    return np.broadcast_to(org, d.shape).copy(), d


def sphere_interface(o, d, c, r, inside, ri):
    """A ray's meeting with a sphere it is known to meet, in float64: the point (the far root from inside, the near one from outside),
    and the reflected and the refracted unit direction there (the refracted one NaN beyond the critical angle)."""
    oc = c - o
    a, h = (d * d).sum(axis=1), (oc * d).sum(axis=1)
    s = np.sqrt(np.maximum(h * h - a * ((oc * oc).sum(axis=1) - r * r), 0.0))
    t = np.where(inside, h + s, h - s) / a
    P = o + t[:, None] * d
    n = (P - c) / r[:, None] * np.where(inside, -1.0, 1.0)[:, None]
    du = d / np.sqrt(a)[:, None]
    return P, T.reflect(du, n), T.refract(du, n, ri)[0]


def interface_gains(o, d, c, r, inside, ri, step=2.0 ** -20):
    """How far the hit point and the two outgoing directions of sphere_interface move per unit of a small displacement of the ray's origin
    (across the ray: along it nothing moves) and per radian of its direction: central differences of the float64 interface along two
    axes across the ray, combined as a root of the sum of squares, which is at least the gain along any axis between them.  A ray
    uncertain by (origin_err, dir_err) leaves the interface uncertain by gain_o origin_err + gain_d dir_err, to first order: the point's
    displacement along the ray and across it, the normal's turn with the point and the direction's own error are one linear map, and
    adding their separate bounds (as the single bounce of specular_frame may) would triple the growth per interface."""
    du = d / np.linalg.norm(d, axis=1, keepdims=True)
    e1 = np.cross(du, np.where((np.abs(du[:, :1]) < 0.6), [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(du, e1)
    sq = {name: 0.0 for name in ("point_o", "point_d", "reflect_o", "reflect_d", "refract_o", "refract_d")}
    for e in (e1, e2):
        for what, plus, minus in (("o", sphere_interface(o + step * e, du, c, r, inside, ri), sphere_interface(o - step * e, du, c, r, inside, ri)),
                                  ("d", sphere_interface(o, du + step * e, c, r, inside, ri), sphere_interface(o, du - step * e, c, r, inside, ri))):
            for name, x, y in zip(("point_", "reflect_", "refract_"), plus, minus):
                sq[name + what] = sq[name + what] + (((x - y) / (2.0 * step)) ** 2).sum(axis=1)
    return {name: np.sqrt(v) for name, v in sq.items()}


def glass_tree(sc, p, origins, directions, mutate=None):
    """The float64 path tree behind every primary ray (origins, directions: one per pixel, float32 promoted exactly) of a spp-1 frame of
    FLAT targets around DIELECTRIC spheres.  At an interface a path goes on
    reflected with weight R (Schlick) or refracted with 1 - R (reflected only beyond the critical angle), ri = 1 / ior where the ray meets
    the outward normal from outside and ior from inside, where the normal is turned to face it.  A branch ends on a target (its colour), in
    the background or at the depth cut-off (black).  A leaf's slot is its string of decisions (0 reflected, 1 refracted), padded with
    zeros to max_depth - 1 bits: leaves are prefix-free, so slots are unique.  Per slot and pixel: colour, weight (0: no such leaf),
    ambiguous (any hit along the branch, with the errors of origin and direction carried from interface to interface by interface_gains
    plus each interface's own float32 bounds; or an interface within its error of the critical angle), reflected (the branch contains a
    reflection).
    mutate: 'ri_kept' (ri = 1 / ior on the way out too), 'normal_unflipped' (the outward normal inside as well)."""
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    n = len(o)
    bits = p.max_depth - 1
    L = 1 << bits
    out = dict(colour=np.full((L, n), BLACK, np.uint32), weight=np.zeros((L, n)), ambiguous=np.zeros((L, n), bool),
               reflected=np.zeros((L, n), bool), glass=np.zeros(n, bool))
    sph = np.asarray(sc["spheres"], np.float64)
    kinds, params_, codes = sc["smats"]["kind"], sc["smats"]["param"].astype(np.float64), sc["sphere_codes"]
    a = dict(pix=np.arange(n), code=np.zeros(n, np.int64), nb=np.zeros(n, np.int64), o=o, d=d, eo=np.zeros(n), ed=np.zeros(n), w=np.ones(n),
             amb=np.zeros(n, bool), refl=np.zeros(n, bool))
    for k in range(p.max_depth):
        if not len(a["pix"]):
            break
        h = T.nearest_hit(a["o"], a["d"], p.t_min, np.inf, sc["spheres"], origin_err=a["eo"], dir_err=a["ed"])
        amb = a["amb"] | h["ambiguous"]
        si = np.where(h["kind"] == T.SPHERE, h["index"], 0).astype(np.int64)
        issph = h["kind"] == T.SPHERE
        glass = issph & (kinds[si] == MAT_DIELECTRIC)
        if k == 0:
            out["glass"][a["pix"]] = glass
        last = k + 1 == p.max_depth
        leaf = ~glass | last
        slot = a["code"][leaf] << (bits - a["nb"][leaf])
        px = a["pix"][leaf]
        out["colour"][slot, px] = np.where(issph & (kinds[si] == MAT_FLAT), codes[si], BLACK)[leaf]
        out["weight"][slot, px] = a["w"][leaf]
        out["ambiguous"][slot, px] = amb[leaf]
        out["reflected"][slot, px] = a["refl"][leaf]
        g = glass & (not last)
        if not g.any():
            break
        oo, dd, t, eo, ed = a["o"][g], a["d"][g], h["t"][g], a["eo"][g], a["ed"][g]
        c, r, ior = sph[si[g], :3], sph[si[g], 3], params_[si[g]]
        P = oo + t[:, None] * dd
        nout = (P - c) / r[:, None]
        front = (dd * nout).sum(axis=1) < 0
        nrm = nout if mutate == "normal_unflipped" else h["normal"][g]
        ri = 1.0 / ior if mutate == "ri_kept" else np.where(front, 1.0 / ior, ior)
        du = dd / np.linalg.norm(dd, axis=1, keepdims=True)
        cos_in = -(du * nrm).sum(axis=1)
        sin_in = np.sqrt(np.maximum(1.0 - cos_in ** 2, 0.0))
        fd, total = T.refract(du, nrm, ri)
        total = total | np.isnan(fd).any(axis=1)
        R = np.where(total, 1.0, np.clip(T.schlick(cos_in, ri), 0.0, 1.0))
        cos_out = np.sqrt(np.maximum(1.0 - (ri * sin_in) ** 2, 1e-24))
        # what this interface adds by its own float32 arithmetic: the hit's error_bound_t without a ray uncertainty, the normal's bound with it
        oc = c - oo
        oc2, a2 = (oc * oc).sum(axis=1), (dd * dd).sum(axis=1)
        disc = (oc * dd).sum(axis=1) ** 2 - a2 * (oc2 - r * r)
        t_own = T.error_bound_t_sphere(np.sqrt(oc2), oc2 + r * r, np.sqrt(np.maximum(disc, 0.0)), t, np.abs(oc2 - r * r), np.maximum(np.abs(a2 - 1.0), 8.0 * T.U))
        M = np.maximum(np.abs(oo).max(axis=1), np.abs(c).max(axis=1) + r)
        n_own = T.error_bound_normal_sphere(t_own, M, r)
        # what it does to the uncertainty the ray arrives with: the gains of the float64 interface itself
        G = interface_gains(oo, dd, c, r, ~front, np.where(front, 1.0 / ior, ior))
        p_err = G["point_o"] * eo + G["point_d"] * ed + t_own + T.SQRT3 * T.U * M
        n_err = n_own + (G["point_o"] * eo + G["point_d"] * ed) / r
        r_err = G["reflect_o"] * eo + G["reflect_d"] * ed + T.reflect_error(0.0, n_own)
        f_err = G["refract_o"] * eo + G["refract_d"] * ed + T.refract_error(0.0, n_own, ri, np.abs(cos_in), cos_out)
        amb_g = amb[g] | (np.abs(ri * sin_in - 1.0) < 64.0 * T.U + 2.0 * ri * (ed + n_err))
        keep = ~total
        child = lambda sel, bit, direction, err, w, refl: dict(                      # noqa: E731
            pix=a["pix"][g][sel], code=(a["code"][g][sel] << 1) | bit, nb=a["nb"][g][sel] + 1, o=P[sel], d=direction[sel], eo=p_err[sel], ed=err[sel],
            w=w[sel], amb=amb_g[sel], refl=refl[sel])
        every = np.ones(len(t), bool)
        kids = [child(every, 0, T.reflect(du, nrm), r_err, a["w"][g] * R, every),
                child(keep, 1, fd, np.where(np.isfinite(f_err), f_err, 1.0), a["w"][g] * (1.0 - R), a["refl"][g])]
        a = {key: np.concatenate([kid[key] for kid in kids]) for key in kids[0]}
        alive = a["w"] > 0.0
        a = {key: v[alive] for key, v in a.items()}
    return out


def sample_glass_tree(tree, rng):
    """A frame that follows a tree faithfully: per pixel one leaf, drawn by weight."""
    cdf = np.cumsum(tree["weight"], axis=0)
    pick = (rng.random(cdf.shape[1])[None] * cdf[-1][None] >= cdf).sum(axis=0)
    return tree["colour"][np.minimum(pick, len(cdf) - 1), np.arange(cdf.shape[1])]


def check_glass_tree(pixels, tree, cap=SPECULAR_CAP):
    """(a) every pixel shows the colour of one of its leaves; a pixel is skipped when a leaf of weight > 1e-3 is ambiguous.  (b) the number
    of pixels that show their all-refract leaf (enter, leave: slot 11 0..0) within 6 sigma of the sum of that leaf's weights, over the
    pixels where no other leaf has its colour.  (c) counts: through the glass, showing a leaf with a reflection in it (no leaf without one
    has that colour)."""
    pixels = np.asarray(pixels, np.uint32).reshape(-1)
    w, col = tree["weight"], tree["colour"]
    L = len(w)
    present = w > 0.0
    skip = (tree["ambiguous"] & (w > GLASS_MIN_WEIGHT)).any(axis=0)
    heaviest = np.argmax(w, axis=0)
    allowed = np.where(present, col, col[heaviest, np.arange(w.shape[1])][None])
    check_frame(pixels, allowed, skip, cap)
    glass = tree["glass"] & ~skip
    rr = (L >> 1) | (L >> 2)                                              # refracted twice, then a leaf
    others = present.copy()
    others[rr] = False
    unique = present[rr] & ~((col == col[rr][None]) & others).any(axis=0)
    counted = glass & unique
    shown = int((pixels[counted] == col[rr][counted]).sum())
    z = check_count(shown, w[rr][counted])
    match = present & (col == pixels[None])
    reflected = glass & (match & tree["reflected"]).any(axis=0) & ~(match & ~tree["reflected"]).any(axis=0)
    return dict(compared=int((~skip).sum()), skipped=int(skip.sum()), through_glass=int(glass.sum()), counted=int(counted.sum()),
                all_refract=shown, expected=float(w[rr][counted].sum()), z=z, reflected=int(reflected.sum()))


# ====================================================================================================================== (j) sky and pack
SKY_SIZE = (64, 36)


def sky_scene():
    """One sphere behind the camera: every primary ray escapes."""
    sc = dict(spheres=np.array([[0.0, 0.0, 50.0, 1.0]], np.float32), smats=material(MAT_FLAT, (1.0, 1.0, 1.0)), faces=None, verts=None, fmats=None)
    w, h = SKY_SIZE
    return sc, look_at(w, h, (0.5, 1.0, 2.0), (0.2, 1.4, -1.0), 70.0), Params(w, h)


def check_sky(linear, cam, p, law=T.sky):
    """The linear frame (pixels, 3) against the float64 sky of the float64 primary ray, within error_bound_sky of the primary direction's bound."""
    xx, yy = pixel_grid(p)
    _, d, ln = T.camera_ray(cam, p, xx, yy)
    bound = T.error_bound_sky(T.error_bound_dir(cam, p.width, p.height, ln))
    ratio = np.abs(np.asarray(linear, np.float64).reshape(-1, 3) - law(d)) / bound[:, None]
    assert ratio.max() <= 1.0, "a sky channel is %.2f of its bound off" % ratio.max()
    return dict(compared=int(ratio.size), max_ratio=float(ratio.max()), t_range=(float(0.5 * (d[:, 1].min() + 1)), float(0.5 * (d[:, 1].max() + 1))))


def sky_of_y(d):
    """Mutant: t = y."""
    t = np.asarray(d, np.float64)[..., 1]
    return (1.0 - t)[..., None] * np.ones(3) + t[..., None] * np.array([0.5, 0.7, 1.0])


PACK_GRID = (20, 15, 3)                                                # 300 blocks of 3 x 3 pixels
PACK_CAP = 0.01


def pack_values():
    """900 channel values, three per sphere: for every byte b a value that packs to it without gamma ((b + e) / 255) and one that does
    with gamma 2 (((b + e) / 255)^2), |e| <= 0.4; exact zeros; values above 1 (just above, and far); the rest uniform in [0, 1.2].  A
    value is redrawn until 255 x and 255 sqrt(x) are both 0.02 from a half-integer, so the reference leaves no channel out; shuffled, so
    the three channels of a sphere are unrelated numbers."""
    rng = np.random.default_rng(17)
    gx, gy, _ = PACK_GRID

    def clear(x):
        x = float(np.float32(x))
        return all(abs(v - np.floor(v) - 0.5) > 0.02 for v in (255.0 * x, 255.0 * np.sqrt(x)))

    def draw(make):
        while True:
            x = make()
            if clear(x):
                return x

    vals = [draw(lambda: max((b + rng.uniform(-0.4, 0.4)) / 255.0, 1e-4)) for b in range(256)]
    vals += [draw(lambda: max((b + rng.uniform(-0.4, 0.4)) / 255.0, 1e-3) ** 2) for b in range(256)]
    vals += [0.0] * 12 + [1.0, 1.0 + 2.0 ** -23, 1.001, 1.5, 2.0, 7.25, 100.0, 255.0, 1000.0]
    vals += [draw(lambda: rng.uniform(0.0, 1.2)) for _ in range(3 * gx * gy - len(vals))]
    vals = np.array(vals, np.float32)
    while True:
        rgb = rng.permutation(vals).reshape(-1, 3)
        if ((rgb[:, 0] != rgb[:, 1]) & (rgb[:, 1] != rgb[:, 2]) & (rgb[:, 0] != rgb[:, 2])).all():
            return rgb


def pack_scene(gamma2):
    """A grid of FLAT spheres on the image plane, one per 3 x 3 pixel block, radius 1.2 pixels, centred on the block's middle pixel."""
    gx, gy, b = PACK_GRID
    w, h = gx * b, gy * b
    cam = Cam((0.0, 0.0, 0.0), (float(w - 1), 0.0, 0.0), (0.0, float(h - 1), 0.0), (-0.5 * (w - 1), -0.5 * (h - 1), -64.0))      # one unit per pixel
    rgb = pack_values()
    ix, iy = np.meshgrid(np.arange(gx), np.arange(gy))
    cx = -0.5 * (w - 1) + b * ix.reshape(-1) + 1.0
    cy = -0.5 * (h - 1) + (h - 1.0 - (b * iy.reshape(-1) + 1.0))
    sph = np.stack([cx, cy, np.full(len(cx), -64.0), np.full(len(cx), 1.2)], axis=1).astype(np.float32)
    sm = np.concatenate([material(MAT_FLAT, c) for c in rgb])
    return (dict(spheres=sph, smats=sm, faces=None, verts=None, fmats=None), cam,
            Params(w, h, flags=FLAG_BLACK | (1 if gamma2 else 0)))


def pack_expectation(sc, cam, p):
    """Per pixel the float32 linear colour the float64 nearest hit asks for (black where the ray escapes), and the pixels it cannot decide."""
    xx, yy = pixel_grid(p)
    o, d, ln = T.camera_ray(cam, p, xx, yy)
    rec = T.nearest_hit(o, d, p.t_min, np.inf, sc["spheres"], dir_err=T.error_bound_dir(cam, p.width, p.height, ln))
    hit = rec["kind"] == T.SPHERE
    rgb = np.where(hit[:, None], sc["smats"]["rgb"][np.where(hit, rec["index"], 0)], np.float32(0.0)).astype(np.float32)
    assert len(np.unique(rec["index"][hit])) == len(sc["spheres"]), "a sphere of the grid is not seen"
    return rgb, rec["ambiguous"], hit


def check_pack(pixels, linear, gamma2, pack=T.pack, cap=PACK_CAP):
    """Packed pixels against T.pack of the same source's float32 linear frame, channel by channel; the channels within the tie margin are
    left out and counted.  Returns the figures and the set of bytes seen."""
    pixels = np.asarray(pixels, np.uint32).reshape(-1)
    linear = np.asarray(linear, np.float32).reshape(-1, 3)
    _, want, tie = pack(linear, gamma2)
    assert tie.mean() <= cap, "%d of %d channels at a tie" % (int(tie.sum()), tie.size)
    got = np.stack([(pixels >> 24) & 0xFF, (pixels >> 16) & 0xFF, (pixels >> 8) & 0xFF], axis=1)
    assert ((pixels & 0xFF) == 0xFF).all(), "the low byte is 0xFF"
    bad = ~tie & (got != want)
    assert not bad.any(), "%d channels pack to another byte, first %s" % (int(bad.sum()), [
        (float(linear[i, c]), int(got[i, c]), int(want[i, c])) for i, c in zip(*np.nonzero(bad))][:3])
    return dict(compared=int((~tie).sum()), ties=int(tie.sum()), bytes_seen=len(np.unique(want[~tie])), clamped=int((linear > 1.0).sum()),
                zeros=int((linear == 0.0).sum()))
