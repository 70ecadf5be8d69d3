"""The image texture law (rt3.h "Image textures") without a GPU: rt3_debug_texture_lookup, rt3_debug_texture_sphere_uv and
rt3_debug_texture_face_uv — the law in C, the statement the device compiles too (rt3_texture_law.hpp) — against tests/texture_ref.py bit for bit, and
the law's own properties: a one-colour texture, the book's sphere coordinates, a face's vertices."""
import numpy as np
import pytest

import texture_ref as T

F = np.float32
SIZES = [(8, 8), (5, 3), (1, 1), (1, 4), (7, 1), (2, 2)]


def same(a, b):
    """Bit equality, a NaN equal to any NaN (a NaN's sign and payload are the compiler's choice, not the law's)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("wrap", ["repeat", "clamp"])
@pytest.mark.parametrize("w,h", SIZES)
def test_lookup_is_the_law_bit_for_bit(rt3, w, h, wrap):
    """Random (u, v), every texel corner and centre with their float neighbours (the REPEAT seam, both CLAMP edges), negative, huge, NaN and +-inf."""
    image = T.random_image(w, h, seed=1)
    uv = T.lookup_points(w, h)
    got = rt3.texture_lookup(image, uv, wrap)
    want = T.lookup(image, uv, T.CLAMP if wrap == "clamp" else T.REPEAT)
    assert same(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    finite = np.isfinite(uv).all(axis=1) & (np.abs(uv).max(axis=1) < 1e30)      # (u * W stays finite: the weight is one)
    assert np.isfinite(got[finite]).all()                               # a (u, v) with finite weights blends texels and nothing else


def test_lookup_reads_the_texels_it_should(rt3):
    """Texel centres return their texel; the REPEAT seam blends the last column with the first, CLAMP holds the edge; row 0 is on top (v = 0)."""
    w, h = 5, 3
    image = T.random_image(w, h, seed=2, channels=3)
    centres = np.array([[(i + 0.5) / w, (j + 0.5) / h] for j in range(h) for i in range(w)], F)
    for wrap in ("repeat", "clamp"):
        got = rt3.texture_lookup(image, centres, wrap).reshape(h, w, 3)
        # the centre's u is rounded to f32 and so is u * W: fx is i up to W * 2^-23 < 2^-20, a weight that far from 0 or 1, times texel
        # differences below 2: 2^-19, and the three roundings of the combination on values below 2 (2^-23 each) stay far below the 2^-18 asked
        assert np.abs(got - image).max() <= 2.0 ** -18
    seam = np.array([[0.0, 0.5 / h], [1.0, 0.5 / h]], F)
    rep = rt3.texture_lookup(image, seam, "repeat")
    mid = (image[0, w - 1] + F(0.5) * (image[0, 0] - image[0, w - 1])).astype(F)
    assert same(rep[0], mid) and same(rep[1], mid)
    cl = rt3.texture_lookup(image, seam, "clamp")
    assert same(cl[0], image[0, 0]) and same(cl[1], image[0, w - 1])
    far = rt3.texture_lookup(image, np.array([[-7.0, -7.0], [9.0, 9.0]], F), "clamp")
    assert same(far[0], image[0, 0]) and same(far[1], image[h - 1, w - 1])


@pytest.mark.parametrize("wrap", ["repeat", "clamp"])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (8, 8)])
def test_a_one_colour_texture_returns_that_colour_exactly(rt3, w, h, wrap):
    colour = np.array([0.3, 1.7, 0.0123], F)
    image = np.broadcast_to(colour, (h, w, 3))
    uv = T.lookup_points(w, h)
    uv = uv[np.isfinite(uv).all(axis=1) & (np.abs(uv).max(axis=1) < 1e30)]     # (a finite weight: c + w * 0 = c)
    got = rt3.texture_lookup(image, uv, wrap)
    assert same(got, np.broadcast_to(colour, got.shape))


def test_sphere_uv_is_the_law_bit_for_bit(rt3):
    n = T.sphere_normals()
    assert same(rt3.texture_sphere_uv(n), T.sphere_uv(n))


def test_sphere_uv_poles_and_seam(rt3):
    got = rt3.texture_sphere_uv(np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [1, 0, -0.0], [0, 0, -1], [-1, 0, 0], [0, 0, 1]], F))
    assert got.tolist() == [[0, 0], [0, 1], [0.5, 0.5], [0.5, 0.5], [0.75, 0.5], [0.0, 0.5], [0.25, 0.5]]       # the book's table: u of +x is 0.5, of -z 0.75
    eps = F(1e-6)
    near = rt3.texture_sphere_uv(np.array([[-1, 0, eps], [-1, 0, -eps]], F))        # either side of the seam at -x
    assert near[0, 0] < 0.01 and near[1, 0] > 0.99 and (near[:, 0] >= 0).all() and (near[:, 0] < 1).all()


def test_sphere_uv_is_the_books_formula_within_the_error_of_turns(rt3):
    """|u - u64| <= 2^-23 turns and |v - v64| <= 2 * 2^-23 (v = 2 turns(ny, hxz): the doubling is exact), plus what the float32 inputs' own sqrt adds:
    hxz is sqrt(nx^2 + nz^2) rounded three times, a relative 1.5 * 2^-24, which moves the polar angle by at most that times |ny| hxz / (2 pi) turns —
    below 2^-26 — so v's bound is 2 * (2^-23 + 2^-26).  u wraps at the seam: the distance is taken on the circle."""
    n = T.sphere_normals()
    n = n[np.isfinite(n).all(axis=1) & (np.hypot(n[:, 0], n[:, 2]) > 1e-3)]          # away from the poles, where u is defined
    got = rt3.texture_sphere_uv(n).astype(np.float64)
    want = T.sphere_uv64(n)
    du = np.abs(got[:, 0] - want[:, 0])
    du = np.minimum(du, 1.0 - du)
    assert du.max() <= 2.0 ** -23, du.max()
    assert np.abs(got[:, 1] - want[:, 1]).max() <= 2.0 * (2.0 ** -23 + 2.0 ** -26)


def random_faces(k, seed):
    rng = np.random.default_rng(seed)
    p1 = rng.uniform(-2, 2, (k, 3)).astype(F)
    p2 = (p1 + rng.uniform(-1, 1, (k, 3))).astype(F)
    p3 = (p1 + rng.uniform(-1, 1, (k, 3))).astype(F)
    uv6 = rng.uniform(-2, 3, (k, 6)).astype(F)
    return p1, p2, p3, uv6


def test_face_uv_is_the_law_bit_for_bit(rt3):
    p1, p2, p3, uv6 = random_faces(256, 11)
    rng = np.random.default_rng(12)
    b = rng.dirichlet((1, 1, 1), 256)
    inside = (b[:, :1] * p1 + b[:, 1:2] * p2 + b[:, 2:] * p3).astype(F)
    for pts in (inside, p1, p2, p3, (inside + F(0.25)).astype(F)):                   # inside, the vertices, off the plane
        got = np.stack([rt3.texture_face_uv(p1[i], p2[i], p3[i], uv6[i], pts[i]) for i in range(len(pts))])
        assert same(got, T.face_uv(p1, p2, p3, uv6, pts))


def test_face_uv_of_a_degenerate_face(rt3):
    """den == 0: b2 = b3 = 0, the first vertex's (u, v) — for a point, for a segment (p3 = p1 + 2 (p2 - p1), exactly) and with NaN nowhere."""
    uv6 = np.array([0.25, 0.75, 3, 4, 5, 6], F)
    a = np.array([1, 2, 3], F)
    e = np.array([0.5, -0.25, 1], F)
    for p2, p3 in ((a, a), (a + e, a + 2 * e), (a, a + e)):
        got = rt3.texture_face_uv(a, p2, p3, uv6, a + F(0.125))
        assert same(got, T.face_uv(a, p2, p3, uv6, a + F(0.125))[0]) and got.tolist() == [0.25, 0.75]


def test_face_uv_returns_a_vertex_its_own_uv(rt3):
    """At p = p2 the law has q = e1 exactly, so q1 = d11 and q2 = d12 bit for bit and
        b2 = (d22 d11 - d12 d12) / den,  b3 = (d11 d12 - d12 d11) / den = 0 exactly (the two products are the same float).
    b2's numerator IS den's expression with the factors of the first product swapped — the same float — so b2 = 1 exactly, b1 = 0, and u = u2, v = v2
    bit for bit.  At p = p3 the same with the roles swapped.  At p = p1, q = 0: b2 = b3 = 0 and u = u1 exactly.  The bound is therefore 0 ulps; the test
    allows the 4 ulps of the uv magnitudes that the issue's "a few ulps" names, and asserts the exact result separately."""
    p1, p2, p3, uv6 = random_faces(512, 21)
    for k, pts in enumerate((p1, p2, p3)):
        got = np.stack([rt3.texture_face_uv(p1[i], p2[i], p3[i], uv6[i], pts[i]) for i in range(len(pts))])
        want = uv6[:, 2 * k:2 * k + 2]
        ulp = np.spacing(np.abs(uv6).max(axis=1)).astype(np.float64)[:, None]
        assert (np.abs(got.astype(np.float64) - want) <= 4 * ulp).all()
        assert same(got, want)
