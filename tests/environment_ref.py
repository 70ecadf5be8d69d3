"""The environment map's lookup law (include/rt3.h) restated in numpy float32, and the directions the tests look up.

Every operation of the law is an IEEE f32 add, subtract, multiply, divide, compare or floor rounded on its own, so float32 arrays reproduce the
device's env_lookup and the host's rt3_debug_environment_lookup bit for bit: the tests compare bit patterns, not values."""
import numpy as np

F = np.float32


def _axis(c, m, n):
    """One in-face coordinate -> (i0, i1, w): the law's q, u, fx, floor, weight and the clamp in float before the conversion."""
    with np.errstate(all="ignore"):
        q = c / m
        u = q * F(0.5) + F(0.5)
        fx = u * F(n) - F(0.5)
        x0 = np.floor(fx)
        w = fx - x0
        k = np.fmin(np.fmax(x0, F(-1.0)), F(n) - F(1.0)).astype(np.int64)       # fmax / fmin drop a NaN: it gives -1
    return np.maximum(k, 0), np.minimum(k + 1, n - 1), w


def face_coords(d):
    """(face, m, sc, tc) of float32 directions (K, 3), by the law's three cases."""
    d = np.asarray(d, F).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(invalid="ignore"):
        cx = (ax >= ay) & (ax >= az)
        cy = ~cx & (ay >= az)
        xn, yn, zn = x < 0, y < 0, z < 0
    f = np.where(cx, np.where(xn, 1, 0), np.where(cy, np.where(yn, 3, 2), np.where(zn, 5, 4)))
    m = np.where(cx, ax, np.where(cy, ay, az))
    sc = np.where(cx, np.where(xn, z, -z), np.where(cy, x, np.where(zn, -x, x)))
    tc = np.where(cx, -y, np.where(cy, np.where(yn, -z, z), -y))
    return f, m.astype(F), sc.astype(F), tc.astype(F)


def lookup(cube, d):
    """env(d): cube (6, N, N, 3 | 4) float32, d (K, 3) float32 -> (K, 3) float32."""
    cube = np.asarray(cube, F)
    n = cube.shape[1]
    assert cube.shape[0] == 6 and cube.shape[2] == n and cube.shape[3] in (3, 4)
    f, m, sc, tc = face_coords(d)
    i0, i1, wx = _axis(sc, m, n)
    j0, j1, wy = _axis(tc, m, n)
    rgb = cube[..., :3]
    c00, c10, c01, c11 = rgb[f, j0, i0], rgb[f, j0, i1], rgb[f, j1, i0], rgb[f, j1, i1]    # cAB: column iA, row jB
    wx, wy = wx[:, None], wy[:, None]
    with np.errstate(all="ignore"):
        top = c00 + wx * (c10 - c00)
        bot = c01 + wx * (c11 - c01)
        return (top + wy * (bot - top)).astype(F)


def face_direction(f, s, t):
    """The direction whose in-face coordinates on face f are sc / m = s and tc / m = t, float64, not normalised: the law's cases inverted by hand."""
    one = np.ones_like(s)
    return np.stack([(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)][f], axis=-1)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def directions(n, seed=5):
    """The unit directions of the lookup-law tests for a map of face size n: 4096 random ones, the six axes, the eight (+-a, +-a, +-a) and the
    twelve (+-a, +-a, 0)-type ties between faces, axes with components of -0.0, and directions through every texel corner and centre."""
    rng = np.random.default_rng(seed + n)
    out = [unit(rng.normal(0.0, 1.0, (4096, 3)))]
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    out.append(axes.astype(F))
    a3, a2 = F(1.0) / np.sqrt(F(3.0)), np.sqrt(F(0.5))
    out.append(np.array([[sx * a3, sy * a3, sz * a3] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], F))
    ties = []
    for zero in range(3):
        for s1 in (1, -1):
            for s2 in (1, -1):
                v = [s1 * a2, s2 * a2]
                v.insert(zero, 0.0)
                ties.append(v)
    out.append(np.array(ties, F))
    neg = np.array([[1, -0.0, -0.0], [-1, -0.0, 0.0], [-0.0, 1, -0.0], [0.0, -1, -0.0], [-0.0, -0.0, 1], [-0.0, 0.0, -1],
                    [-0.0, a2, a2], [a2, -0.0, -a2], [-a2, a2, -0.0]], F)
    out.append(neg)
    corners = np.arange(n + 1, dtype=np.float64) / n * 2.0 - 1.0
    centres = (np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0
    for grid in (corners, centres):
        s, t = np.meshgrid(grid, grid)
        for f in range(6):
            out.append(unit(face_direction(f, s.ravel(), t.ravel())))
    return np.ascontiguousarray(np.concatenate(out), F)


def random_cube(n, seed=0, channels=4):
    """A random map with texels in [0, 4): float32 (6, n, n, channels)."""
    return np.random.default_rng(1000 * seed + n).uniform(0.0, 4.0, (6, n, n, channels)).astype(F)
