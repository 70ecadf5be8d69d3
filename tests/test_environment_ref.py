"""The environment map's lookup law without a GPU: the C restatement on the host (rt3_debug_environment_lookup) against the numpy
one (tests/environment_ref.py) by bit pattern, the properties the law promises, its orientation against float64 geometry written independently,
and cube_from_equirect."""
import numpy as np
import pytest

import environment_ref as E

SIZES = [1, 2, 5, 16]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_the_host_lookup_equals_the_numpy_law_bit_for_bit(rt3, n):
    cube = E.random_cube(n, seed=1)
    d = E.directions(n)
    assert len(d) > 4096 + 6 + 8 + 12
    got = rt3.environment_lookup(cube, d)
    want = E.lookup(cube, d)
    assert got.shape == want.shape == (len(d), 3)
    bad = (bits(got) != bits(want)).any(axis=1)
    assert not bad.any(), "%d of %d directions differ, first %s: %s vs %s" % (bad.sum(), len(d), d[bad][:3], got[bad][:3], want[bad][:3])
    assert rt3.HipRenderer.environment_lookup(cube[..., :3], d[7]).tolist() == want[7].tolist()       # the method, three channels, one direction


@pytest.mark.parametrize("n", SIZES)
def test_directions_that_are_not_finite_or_not_unit_read_inside_the_map(rt3, n):
    cube = E.random_cube(n, seed=2)
    inf, nan = np.inf, np.nan
    d = np.array([[0, 0, 0], [-0.0, -0.0, -0.0], [nan, 0, 0], [0, nan, 1], [nan, nan, nan], [inf, 0, 0], [-inf, 1, 2], [inf, inf, 1], [inf, -inf, inf],
                  [1e-45, 0, 0], [3e38, 3e38, -3e38], [1, 1e30, nan], [5, -7, 3]], np.float32)
    got, want = rt3.environment_lookup(cube, d), E.lookup(cube, d)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (got, want)


@pytest.mark.parametrize("n", SIZES)
def test_a_face_of_one_colour_returns_that_colour_exactly(rt3, n):
    rng = np.random.default_rng(3 + n)
    colours = rng.uniform(0.0, 9.0, (6, 3)).astype(np.float32)
    cube = np.broadcast_to(colours[:, None, None, :], (6, n, n, 3)).copy()
    for f in range(6):
        s, t = rng.uniform(-0.999, 0.999, (2, 10000))
        d = E.unit(E.face_direction(f, s, t))
        assert (E.face_coords(d)[0] == f).all()
        for got in (rt3.environment_lookup(cube, d), E.lookup(cube, d)):
            assert (bits(got) == bits(colours[f])).all(), f


# ---- orientation, against float64 geometry that does not use the law's formulas: per face the outward axis, the world direction in which its columns
# grow and the one in which its rows grow.  Rows grow downwards (-Y) on the four side faces; the faces are laid out as the usual cube-map convention
# has them, mirrored for a viewer inside: columns x up = axis.
AXIS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
RIGHT = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
DOWN = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.float64)
SIDE = [0, 1, 4, 5]                                                  # +X, -X, +Z, -Z


def test_the_six_axes_land_in_faces_0_to_5(rt3):
    cube = np.zeros((6, 2, 2, 3), np.float32)
    cube[..., 0] = np.arange(6, dtype=np.float32)[:, None, None] + 1
    for f in range(6):
        assert rt3.environment_lookup(cube, AXIS[f].astype(np.float32))[0] == f + 1
        assert E.lookup(cube, AXIS[f:f + 1].astype(np.float32))[0, 0] == f + 1
    for f in SIDE:                                                 # the side faces: +Y up, columns x up = axis
        assert np.array_equal(-DOWN[f], [0, 1, 0]) and np.allclose(np.cross(RIGHT[f], -DOWN[f]), AXIS[f])


@pytest.mark.parametrize("f", range(6))
@pytest.mark.parametrize("row,col", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_a_lit_texel_is_seen_from_its_own_quadrant(rt3, f, row, col):
    cube = np.zeros((6, 2, 2, 3), np.float32)
    cube[f, row, col] = 1.0
    seen = {}
    for r in (0, 1):
        for c in (0, 1):                                               # 0.3 rad from the axis towards the quadrant of texel (r, c)
            toward = (RIGHT[f] * (1 if c else -1) + DOWN[f] * (1 if r else -1)) / np.sqrt(2.0)
            d = (np.cos(0.3) * AXIS[f] + np.sin(0.3) * toward).astype(np.float32)
            got = rt3.environment_lookup(cube, d)
            assert np.array_equal(bits(got), bits(E.lookup(cube, d[None])[0]))
            seen[(r, c)] = float(got[0])
    assert all(seen[(row, col)] > v for k, v in seen.items() if k != (row, col)), seen


@pytest.mark.parametrize("f", SIDE)
@pytest.mark.parametrize("n", [2, 5])
def test_row_0_of_a_side_face_is_up(rt3, f, n):
    """0.9 of the way from the face's centre to its upper edge and 0.1 to the side — (0.1, 0.9, .) in the face's (right, +Y, axis) frame, normalised —
    lies above the centre of row 0 for n <= 5: the clamp makes row 0 the only row read."""
    cube = np.zeros((6, n, n, 3), np.float32)
    cube[:, 0] = 1.0
    d = E.unit(0.1 * RIGHT[f] + 0.9 * np.array([0.0, 1.0, 0.0]) + AXIS[f])
    assert E.face_coords(d)[0][0] == f
    assert rt3.environment_lookup(cube, d)[0] == 1.0 and E.lookup(cube, d[None])[0, 0] == 1.0
    assert rt3.environment_lookup(cube, d * np.float32([1, -1, 1]))[0] == 0.0      # mirrored downwards: the last row


# ---- cube_from_equirect
def test_equirect_of_a_constant_is_that_constant(rt3):
    img = np.full((7, 13, 3), 0.37, np.float32)
    cube = rt3.cube_from_equirect(img, 5)
    assert cube.shape == (6, 5, 5, 4) and cube.dtype == np.float32
    assert (cube[..., :3] == np.float32(0.37)).all() and (cube[..., 3] == 0).all()


def test_equirect_of_the_direction_reproduces_the_direction(rt3):
    h, w, n = 128, 256, 16
    lat = np.pi * (0.5 - (np.arange(h) + 0.5) / h)                     # row 0 is +Y
    lon = 2.0 * np.pi * ((np.arange(w) + 0.5) / w - 0.5)               # the centre column is -Z; +X a quarter turn to its right
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    d = np.stack([np.cos(la) * np.sin(lo), np.sin(la), -np.cos(la) * np.cos(lo)], axis=-1)
    cube = rt3.cube_from_equirect(0.5 + 0.5 * d, n)
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    s, t = np.meshgrid(c, c)
    for f in range(6):
        centre = E.face_direction(f, s, t)
        centre = centre / np.linalg.norm(centre, axis=-1, keepdims=True)
        assert (E.face_coords(centre.reshape(-1, 3).astype(np.float32))[0] == f).all()
        # bilinear interpolation of a function with second derivative <= 0.5 on a 0.0245-rad grid errs by less than 1e-4; the rest is margin
        assert np.abs(cube[f, :, :, :3] - (0.5 + 0.5 * centre)).max() < 1e-3, f
    # what set_environment would see: the lookup of a texel centre's direction is that texel
    got = rt3.environment_lookup(cube, E.unit(E.face_direction(2, s.ravel(), t.ravel())))
    assert np.abs(got - cube[2, :, :, :3].reshape(-1, 3)).max() < 1e-5


def test_equirect_refuses_what_is_no_image(rt3):
    for bad in (np.zeros((4, 4)), np.zeros((4, 4, 2)), np.zeros((0, 4, 3))):
        with pytest.raises(rt3.Fatal):
            rt3.cube_from_equirect(bad, 4)
    with pytest.raises(rt3.Fatal):
        rt3.cube_from_equirect(np.zeros((4, 4, 3)), 0)
