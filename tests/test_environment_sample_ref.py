"""The environment map's sampling table and sampling law (RT3_FLAG_ENV_SAMPLING) without a GPU.

rt3_debug_environment_sample builds the table serially in C and applies rt3env::sample, the function the device's shade_lane calls; it must equal
tests/environment_sample_ref.py (numpy float32 + Python integers) bit for bit.  Then the properties the estimator rests on: support (the table is
positive wherever the bilinear lookup can be), normalisation (the density integrates to 1), the density of a constant map (the furnace test's bound),
and the header / binding / stub coverage of the new symbols.

Pairs: 4096 (base, depth) pairs per map for every N.  At N = 300 — the size with N > M and cells of unequal texel counts — the map with zeros next to
bright texels takes the 4096 and the two other maps 512 each: the one-sample host function keeps the last map's table but compares the whole map
(8.6 MB) on every call, about 1 ms, so 4096 pairs on each of the three maps would take 12 s."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import environment_ref as E
import environment_sample_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 5, 64, 300]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pairs(n, k):
    rng = np.random.default_rng(77 + n)
    base = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    depth = rng.integers(0, 12, k).astype(np.uint32)
    depth[:4] = (0, 1, 63, 64)
    base[:2] = (0, 0xFFFFFFFF)
    return base, depth


def one_bright(n):
    cube = np.zeros((6, n, n, 4), np.float32)
    cube[3, n // 2, n - 1, :3] = (5.0, 0.25, 100.0)
    return cube


def maps(n):
    spiky = E.random_cube(n, seed=12)
    spiky[..., :3] *= (np.random.default_rng(n).uniform(0, 1, (6, n, n, 1)) < 0.3)        # zeros next to bright texels
    return {"random": E.random_cube(n, seed=11), "spiky": spiky, "one bright texel": one_bright(n)}


@pytest.mark.parametrize("n", SIZES)
def test_the_host_law_equals_the_numpy_restatement(rt3, n):
    all_base, all_depth = pairs(n, 4096)
    for name, cube in maps(n).items():
        k = 4096 if n <= 64 or name == "spiky" else 512
        base, depth = all_base[:k], all_depth[:k]
        T = S.Table(cube)
        assert T.m == min(n, 256) and T.total > 0 and T.total == int(T.cdf.ravel()[-1])
        cell, a, b, d, pdf = S.sample(T, base, depth)
        gc, gd, gp = rt3.environment_sample(cube, base, depth)
        assert np.array_equal(gc, cell), "%s N=%d: %d cells differ" % (name, n, (gc != cell).sum())
        assert np.array_equal(bits(gd), bits(d)), "%s N=%d: %d directions differ" % (name, n, (bits(gd) != bits(d)).any(axis=1).sum())
        assert np.array_equal(bits(gp), bits(pdf)), "%s N=%d: %d densities differ" % (name, n, (bits(gp) != bits(pdf)).sum())
        assert (T.q.ravel()[cell] > 0).all() and (pdf > 0).all()                       # a cell with q = 0 is never drawn
        assert np.allclose(np.linalg.norm(gd.astype(np.float64), axis=1), 1.0, atol=1e-6)
        if name == "one bright texel":                                                # only the texel's cell and its ring can be drawn
            face, inn = cell // (T.m * T.m), cell % (T.m * T.m)
            assert (face == 3).all() and len(np.unique(cell)) <= 9 and 1 <= (T.q > 0).sum() <= 9 and (T.q[:3] == 0).all()
        f, m, sc, tc = E.face_coords(gd)                                               # the direction lies on the face of its cell, inside the cell
        assert np.array_equal(f, cell // (T.m * T.m))
    c, d3, p = rt3.environment_sample(maps(n)["random"], 123, 2)                       # the scalar form
    assert isinstance(c, int) and d3.shape == (3,) and p > 0


@pytest.mark.parametrize("n", [1, 5, 300])
def test_an_all_zero_map_is_reported_not_sampled(rt3, n):
    zero = np.zeros((6, n, n, 4), np.float32)
    zero[..., 3] = 7.0                                                                 # the fourth channel is ignored
    zero[0, 0, 0, 0] = np.nan                                                          # a NaN counts as 0
    zero[1, 0, 0, 1] = -3.0                                                            # and so does a negative channel
    T = S.Table(zero)
    assert T.total == 0 and (T.q == 0).all()
    cell, d, pdf = rt3.environment_sample(zero, np.arange(8, dtype=np.uint32), 1)
    assert (cell == 0xFFFFFFFF).all() and (bits(d) == 0).all() and (bits(pdf) == 0).all()


def test_brightness_edge_cases():
    cube = np.zeros((6, 2, 2, 4), np.float32)
    cube[0, 0, 0, :3] = (np.inf, 1.0, 1.0)
    cube[1, 0, 0, :3] = (3e38, 3e38, 3e38)
    cube[2, 0, 0, :3] = (np.nan, 2.0, -1.0)
    l = S.brightness(cube)
    assert l[0, 0, 0] == S.FLT_MAX and l[1, 0, 0] == S.FLT_MAX and l[2, 0, 0] == 2.0
    T = S.Table(cube)
    assert T.q.max() == 2 ** 24 and T.total > 0 and np.isfinite(T.w).all()


@pytest.mark.parametrize("n", [5, 64, 300])
def test_support_the_table_is_positive_wherever_the_lookup_can_be(rt3, n):
    """Isolated bright texels next to zeros: every cell in which the lookup is non-zero at one of a grid of probe points (5 x 5 per cell, strictly inside
    it, the outer ones 1 % from its edges) has q > 0 — the condition the estimator's unbiasedness rests on.  For N > 256 a cell's own texels and a ring
    of one do NOT provide it (a cell of N = 300 starts 0.17 texels into a texel whose left neighbour the lookup still reads): the table takes the texels
    the lookup reads inside the cell.  The lookup is tests/environment_ref.py's, which test_environment_ref.py pins to rt3_debug_environment_lookup bit
    for bit; a sample of the probes is looked up through the C function as well."""
    rng = np.random.default_rng(5 + n)
    cube = np.zeros((6, n, n, 4), np.float32)
    k = max(3, n * n // 40)
    cube[rng.integers(0, 6, k), rng.integers(0, n, k), rng.integers(0, n, k), :3] = rng.uniform(0.5, 2.0, (k, 3))
    T = S.Table(cube)
    m = T.m
    faces = range(6) if n <= 64 else (0, 3)                                            # deliberate: the table's cell rule is the same on every face, only the
                                                                                       # probe directions' mapping differs, and N <= 64 covers all six
    frac = np.array([0.01, 0.25, 0.5, 0.75, 0.99])
    grid = ((np.arange(m)[:, None] + frac[None, :]) / m * 2.0 - 1.0).ravel()           # (m * 5,)
    checked = lit_cells = 0
    for f in faces:
        s, t = np.meshgrid(grid, grid)                                                 # [row point, column point]
        d = E.unit(E.face_direction(f, s.ravel(), t.ravel()))
        ff, mm, sc, tc = E.face_coords(d)
        assert (ff == f).all()
        looked = E.lookup(cube, d)
        some = np.random.default_rng(f).integers(0, len(d), 256)
        assert np.array_equal(bits(rt3.environment_lookup(cube, d[some])), bits(looked[some]))
        lit = (looked != 0).any(axis=1).reshape(m, 5, m, 5).any(axis=(1, 3))           # [row, col]
        assert not (lit & (T.q[f] == 0)).any(), "face %d: %d cells are lit but cannot be drawn" % (f, (lit & (T.q[f] == 0)).sum())
        checked += lit.size
        lit_cells += int(lit.sum())
    assert lit_cells >= 9 and lit_cells < checked                                      # some cells are dark, some are lit


@pytest.mark.parametrize("n", [2, 5, 64])
def test_the_density_integrates_to_one(n):
    """Sum over cells of the integral of pdf over the cell's solid angle = 1.  Analytically: the integral is q / total (the cell's share) times the
    integral of (M^2 / 4) (1 + s^2 + t^2)^(3/2) against d omega = ds dt / (1 + s^2 + t^2)^(3/2), which is (M^2 / 4) (2 / M)^2 = 1.  The first factor is
    checked in integers, the second numerically in float64 (midpoint rule, 64 x 64 points per cell: the integrand of ds dt is the constant M^2 / 4)."""
    T = S.Table(E.random_cube(n, seed=13))
    assert sum(int(v) for v in T.q.ravel()) == T.total
    m = T.m
    k = 64
    for col, row in ((0, 0), (m - 1, 0), (m // 2, m // 2), (m - 1, m - 1)):
        s = ((col + (np.arange(k) + 0.5) / k) / m) * 2.0 - 1.0
        t = ((row + (np.arange(k) + 0.5) / k) / m) * 2.0 - 1.0
        ss, tt = np.meshgrid(s, t)
        g = 1.0 + ss * ss + tt * tt
        domega = (2.0 / m / k) ** 2 / g ** 1.5                                         # the cube's solid-angle measure
        density = (m * m / 4.0) * g ** 1.5                                             # pdf / (q / total)
        assert abs((density * domega).sum() - 1.0) < 1e-12
        sphere_part = domega.sum()                                                     # and the measure itself: six faces tile the sphere
        assert 0 < sphere_part < 4 * np.pi / 6
    # the six faces' solid angles add up to 4 pi (midpoint rule over a whole face, 1024^2 points: error ~1e-6)
    u = (np.arange(1024) + 0.5) / 1024 * 2.0 - 1.0
    ss, tt = np.meshgrid(u, u)
    assert abs(6.0 * ((2.0 / 1024) ** 2 / (1.0 + ss * ss + tt * tt) ** 1.5).sum() - 4 * np.pi) < 1e-5


def test_constant_map_density_is_uniform_within_ten_percent(rt3):
    """A constant map at N = 64: pdf within 10 % of 1 / (4 pi) at every probed point (the table's solid-angle factor is taken at the cell centre, the
    density's at the point: they differ by the variation of (1 + s^2 + t^2)^(3/2) across one cell, at most ~ 3 * 2 / 64 at a corner, plus the
    quantisation's 2^-24).  The furnace test of tests/test_gpu_env_sampling.py takes its bound from this."""
    n = 64
    cube = np.full((6, n, n, 4), 0.75, np.float32)
    T = S.Table(cube)
    frac = np.array([0.0, 0.25, 0.5, 0.75, 0.999])
    grid = ((np.arange(n)[:, None] + frac[None, :]) / n * 2.0 - 1.0).ravel()
    s, t = np.meshgrid(grid, grid)
    worst = 0.0
    for f in range(6):
        p = S.pdf_at(T, f, s, t) * 4 * np.pi
        worst = max(worst, np.abs(p - 1.0).max())
    assert worst < 0.10, worst
    base, depth = pairs(n, 4096)
    _, _, pdf = rt3.environment_sample(cube, base, depth)
    assert (np.abs(pdf.astype(np.float64) * 4 * np.pi - 1.0) < 0.10).all()


# ------------------------------------------------------------------------------------------------ ABI and header
def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    header = open(os.path.join(ROOT, "include", "rt3.h")).read()
    for s, args in (("rt3_debug_environment_sample", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
                    ("rt3_debug_environment_table", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])):
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
    assert "#define RT3_FLAG_ENV_SAMPLING      16u" in header and rt3.FLAG_ENV_SAMPLING == 16
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3 and "RT3_ABI_VERSION 3u" in header     # a flag bit and functions: nothing else
    assert C.sizeof(rt3.rt3_params) == 44
    assert "Out of scope: importance sampling" not in header


def test_python_surface(rt3):
    assert list(inspect.signature(rt3.environment_sample).parameters) == ["cube", "base", "depth"]
    assert list(inspect.signature(rt3.HipRenderer.environment_table).parameters) == ["self"]
    with pytest.raises(rt3.Fatal):
        rt3.environment_sample(np.zeros((6, 2, 3, 4)), 1, 0)


def test_refusals_that_need_no_device(rt3, tmp_path):
    L = rt3.lib()
    rgba = np.ones((6, 2, 2, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                         # noqa: E731
    cell, d, pdf = np.full(1, 9, np.uint32), np.full(3, 9.0, np.float32), np.full(1, 9.0, np.float32)
    assert L.rt3_debug_environment_sample(p(rgba), 2, 1, 0, p(cell), p(d), p(pdf)) == 0 and cell[0] < 24 and pdf[0] > 0
    cell[:], d[:], pdf[:] = 9, 9.0, 9.0
    for args in ((None, 2, 1, 0, p(cell), p(d), p(pdf)), (p(rgba), 0, 1, 0, p(cell), p(d), p(pdf)), (p(rgba), 2049, 1, 0, p(cell), p(d), p(pdf)),
                 (p(rgba), 2, 1, 0, None, p(d), p(pdf)), (p(rgba), 2, 1, 0, p(cell), None, p(pdf)), (p(rgba), 2, 1, 0, p(cell), p(d), None)):
        assert L.rt3_debug_environment_sample(*args) == -1, args
    assert cell[0] == 9 and d.tolist() == [9, 9, 9] and pdf[0] == 9                    # a refused call writes nothing
    m = C.c_uint32(0)
    q, cdf = np.zeros(24, np.uint32), np.zeros(24, np.uint64)
    assert L.rt3_debug_environment_table(None, p(q), p(cdf), 24, C.byref(m)) == -1     # RT3_E_ARG, as every entry point refuses a NULL context
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    stub = C.CDLL(str(so)).rt3_debug_environment_table
    stub.restype = C.c_int
    assert stub(C.c_void_p(0x10), p(q), p(cdf), C.c_uint64(24), C.byref(m)) == -2       # RT3_E_DEVICE: "no device"


def test_cli_usage_errors():
    from test_cli import run
    rc, out, err = run("--scene", "three", "--spp", "4", "--env-sampling", "o.png")
    assert rc == -1 and "--env-sampling needs --env." in err, err
    rc, out, err = run("-h")
    assert rc == 0 and "--env-sampling" in out
