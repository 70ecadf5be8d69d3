"""The environment map's sampling table and sampling law (include/rt3.h "Environment map: sampling") restated in numpy float32 and
Python integers.

The table is integers wherever something is added up and every float operation of the law is an IEEE f32 one rounded on its own, so this file
reproduces rt3_debug_environment_sample (host) and the device's table and shadow rays bit for bit: the tests compare bit patterns.  The one fused
multiply-add of the law, under the normalisation of the direction, is fma32 below: exact product, round-to-odd sum in float64, one rounding to f32."""
import numpy as np

F = np.float32
U = np.uint32
MAX_CELLS = 256
QUANTUM = F(16777216.0)
FLT_MAX = np.finfo(np.float32).max
PI32 = F(3.14159274)


def hash_u32(x):
    x = np.asarray(x, U).copy()
    with np.errstate(over="ignore"):
        x += x << U(10); x ^= x >> U(6); x += x << U(3); x ^= x >> U(11); x += x << U(15)
    return x


def u01(m):
    return ((np.asarray(m, U) & U(0x007FFFFF)) | U(0x3F800000)).view(F) - F(1.0)


def fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays: the product is exact in float64; the sum is rounded to odd there (two-sum gives the error), so the
    final rounding to float32 sees a correct sticky bit."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    need = (e != 0) & ((bits & 1) == 0)
    step = np.where((e > 0) == (s > 0), 1, -1)
    bits = np.where(need, bits + step, bits)
    return bits.view(np.float64).astype(F)


def cells_per_edge(n):
    return min(int(n), MAX_CELLS)


def cell_lo(c, n, m):
    """The first and (cell_hi) the last texel the bilinear lookup reads inside cell c of an axis: floor(c N / M - 0.5), floor((c + 1) N / M - 0.5) + 1."""
    return 0 if c == 0 else (2 * c * n - m) // (2 * m)


def cell_hi(c, n, m):
    return min((2 * (c + 1) * n - m) // (2 * m) + 1, n - 1)


def cell_coord(idx, a, m):
    return ((np.asarray(idx).astype(F) + F(a)) / F(m)) * F(2.0) - F(1.0)


def solid_factor(s, t):
    g = (s * s + t * t) + F(1.0)
    return g * np.sqrt(g)


def brightness(cube):
    """(6, N, N) float32: (max(r, 0) + max(g, 0)) + max(b, 0) with the NaN-dropping max, +inf clamped to FLT_MAX."""
    c = np.asarray(cube, F)
    with np.errstate(all="ignore"):
        l = (np.fmax(c[..., 0], F(0)) + np.fmax(c[..., 1], F(0))) + np.fmax(c[..., 2], F(0))
        return np.fmin(l, F(FLT_MAX)).astype(F)


def weights(cube):
    """(6, M, M) float32 cell weights: the largest brightness over the texels the lookup reads inside the cell, times 1 / (g sqrt(g)) at the centre."""
    l = brightness(cube)
    n = l.shape[1]
    m = cells_per_edge(n)
    lo = [cell_lo(c, n, m) for c in range(m)]
    hi = [cell_hi(c, n, m) for c in range(m)]                                 # inclusive
    cols = np.stack([l[:, :, lo[c]:hi[c] + 1].max(axis=2) for c in range(m)], axis=2)            # (6, N, M)
    lmax = np.stack([cols[:, lo[r]:hi[r] + 1, :].max(axis=1) for r in range(m)], axis=1)         # (6, M, M)
    centre = cell_coord(np.arange(m), 0.5, m)
    sa = F(1.0) / solid_factor(centre[None, :], centre[:, None])               # [row, col]: s from the column, t from the row
    return (lmax * sa[None]).astype(F)


class Table:
    def __init__(self, cube):
        w = weights(cube)
        self.n = int(np.asarray(cube).shape[1])
        self.m = w.shape[1]
        self.w = w
        wmax = w.max()
        with np.errstate(all="ignore"):
            scaled = np.floor(w / wmax * QUANTUM)
        q = np.where(w == 0, 0, np.maximum(np.nan_to_num(scaled), 1)).astype(np.uint32)
        self.q = q                                                             # (6, M, M)
        flat = [int(v) for v in q.ravel()]
        run, sums = 0, []
        for v in flat:                                                         # Python integers: no width, no order
            run += v
            sums.append(run)
        self.cdf_ints = sums
        self.total = run
        self.cdf = np.array(sums, np.uint64).reshape(q.shape)


def sample(table, base, depth):
    """The law for arrays of (base, depth): (cell uint32, a, b float32, direction (K, 3) float32, pdf float32).  table.total must not be 0."""
    T = table
    m = T.m
    base = np.asarray(base, U).reshape(-1)
    depth = np.broadcast_to(np.asarray(depth, U).reshape(-1), base.shape)
    with np.errstate(over="ignore"):
        ctr = U(1) + U(8) * (depth + U(1))
        w3, w4, w5, w6 = (hash_u32(base ^ hash_u32(ctr + U(k))) for k in (3, 4, 5, 6))
    targets = [(((int(h) << 32) | int(l)) * T.total) >> 64 for h, l in zip(w3, w4)]
    cdf = np.array(T.cdf_ints, np.uint64)
    cell = np.searchsorted(cdf, np.array(targets, np.uint64), side="right").astype(np.int64)     # the first index with cdf > target
    face, inn = cell // (m * m), cell % (m * m)
    row, col = inn // m, inn % m
    a, b = u01(w5), u01(w6)
    s = ((col.astype(F) + a) / F(m)) * F(2.0) - F(1.0)
    t = ((row.astype(F) + b) / F(m)) * F(2.0) - F(1.0)
    one = np.ones_like(s)
    table_v = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]
    v = np.zeros((len(s), 3), F)
    for f in range(6):
        sel = face == f
        for k in range(3):
            v[sel, k] = table_v[f][k][sel]
    inv = F(1.0) / np.sqrt(fma32(v[:, 2], v[:, 2], fma32(v[:, 1], v[:, 1], v[:, 0] * v[:, 0])))
    d = (v * inv[:, None]).astype(F)
    qf = T.q.ravel()[cell].astype(F)
    pdf = ((qf / F(np.float64(T.total))) * (F(m * m) * F(0.25))) * solid_factor(s, t)
    return cell.astype(U), a, b, d, pdf.astype(F)


def pdf_at(table, face, s, t):
    """The density per solid angle, float64, at in-face coordinates (s, t) in [-1, 1) of face `face` (arrays): q / total of the cell that holds the point
    times (M^2 / 4) (1 + s^2 + t^2)^(3/2)."""
    m = table.m
    col = np.clip(np.floor((np.asarray(s, np.float64) + 1.0) * 0.5 * m).astype(np.int64), 0, m - 1)
    row = np.clip(np.floor((np.asarray(t, np.float64) + 1.0) * 0.5 * m).astype(np.int64), 0, m - 1)
    q = table.q[face, row, col].astype(np.float64)
    return q / float(table.total) * (m * m / 4.0) * (1.0 + s * s + t * t) ** 1.5
