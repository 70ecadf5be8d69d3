"""The lens models' ray law without a device (include/rt3.h "Lens models"): rt3_debug_lens_ray — the statement k_lens_rays evaluates —
against the numpy restatement (tests/lens_ref.py) bit for bit, the unit-length and float64 bounds, the cube frame against the environment map's
lookup law, the fisheye's centre, the orthographic window, rt3_lens_look_at, and every refusal of a lens."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import environment_ref as E
import lens_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MODELS = ("equirect", "fisheye", "ortho", "cube")
FRAMES = {"equirect": ((37, 29), (8, 5)), "fisheye": ((37, 29), (8, 5)), "ortho": ((37, 29), (8, 5)), "cube": ((1, 6), (5, 30), (8, 48))}


def a_lens(rt3, model, fov_deg=220.0):
    return rt3.make_lens(model, (0.3, 1.1, 2.0), (-0.2, 0.4, -1.0), (0.1, 1.0, 0.05), fov_deg=fov_deg, extent=(3.0, 1.75))


def identity_lens(rt3, model):
    return rt3.make_lens(model, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))


def host_rays(rt3, lens, p):
    """rt3_debug_lens_ray over every (sample, pixel) of the frame, in rt3_lens_rays' order."""
    out = np.zeros((p.spp, p.height, p.width), L.RAY)
    for s in range(p.spp):
        for y in range(p.height):
            for x in range(p.width):
                out[s, y, x] = rt3.lens_ray(lens, p, x, y, s)
    return out.reshape(-1)


def angle(a, b):
    """The angle between unit vectors (K, 3), float64, accurate near 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 2.0 * np.arcsin(np.minimum(0.5 * np.linalg.norm(a - b, axis=-1), 1.0))


@pytest.mark.parametrize("spp", (1, 3, 4))
@pytest.mark.parametrize("model", MODELS)
def test_host_law_equals_the_restatement(rt3, model, spp):
    """Bit for bit, all four models, odd and small frames, no jitter / unstratified / stratified, every sample; with it the two bounds of the law."""
    lens = a_lens(rt3, model)
    for (w, h) in FRAMES[model]:
        p = rt3.make_params(w, h, spp=spp, seed=11)
        got = host_rays(rt3, lens, p)
        want = L.frame_rays(lens, p)
        assert got.tobytes() == want.tobytes(), (model, w, h, spp)
        d = got["direction"].astype(np.float64)
        dd = np.abs((d * d).sum(axis=1) - 1.0)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        truth = np.concatenate([L.directions64(lens, w, h, spp, 11, xx.reshape(-1), yy.reshape(-1), np.full(w * h, s)) for s in range(spp)])
        ang = angle(got["direction"], truth)
        print("%s %dx%d spp %d: max |d.d - 1| = %.3g, max angle to float64 = %.3g rad" % (model, w, h, spp, dd.max(), ang.max()))
        assert dd.max() <= 2.0 ** -20
        assert ang.max() <= 2.0 ** -19
        assert np.isinf(got["t_max"]).all() and (got["_pad"] == 0).all()


@pytest.mark.parametrize("n", (1, 5, 8))
def test_cube_frame_is_the_lookup_laws_layout(rt3, n):
    """spp 1, the identity frame: texel (f, j, i)'s direction is looked up in face f at row j, column i."""
    lens = identity_lens(rt3, "cube")
    p = rt3.make_params(n, 6 * n, spp=1)
    d = host_rays(rt3, lens, p)["direction"]
    f, m, sc, tc = E.face_coords(d)
    col = np.floor(((sc / m) * F(0.5) + F(0.5)) * F(n)).astype(np.int64)
    row = np.floor(((tc / m) * F(0.5) + F(0.5)) * F(n)).astype(np.int64)
    ff, jj, ii = np.meshgrid(np.arange(6), np.arange(n), np.arange(n), indexing="ij")
    assert np.array_equal(f, ff.reshape(-1)) and np.array_equal(row, jj.reshape(-1)) and np.array_equal(col, ii.reshape(-1))


def test_fisheye_centre_is_forward(rt3):
    lens = a_lens(rt3, "fisheye")
    for n in (1, 5, 37):
        p = rt3.make_params(n, n, spp=1)
        d = rt3.lens_ray(lens, p, n // 2, n // 2, 0)["direction"]
        fwd = np.array(list(lens.forward), F)
        inv = F(1.0) / np.sqrt((fwd[0] * fwd[0] + fwd[1] * fwd[1]) + fwd[2] * fwd[2])
        assert d.tobytes() == (fwd * inv).astype(F).tobytes()
    ident = identity_lens(rt3, "fisheye")
    assert rt3.lens_ray(ident, rt3.make_params(9, 9), 4, 4, 0)["direction"].tolist() == [0.0, 0.0, -1.0]


def test_ortho_is_parallel_and_spans_the_window(rt3):
    lens = a_lens(rt3, "ortho")
    p = rt3.make_params(37, 29, spp=4, seed=3)
    r = host_rays(rt3, lens, p)
    fwd = np.array(list(lens.forward), F)
    inv = F(1.0) / np.sqrt((fwd[0] * fwd[0] + fwd[1] * fwd[1]) + fwd[2] * fwd[2])
    assert all(d.tobytes() == (fwd * inv).astype(F).tobytes() for d in r["direction"])
    rel = r["origin"].astype(np.float64) - np.array(list(lens.origin), np.float64)
    e1, e2 = rel @ np.array(list(lens.right), np.float64), rel @ np.array(list(lens.up), np.float64)
    hx, hy = float(lens.half_extent[0]), float(lens.half_extent[1])
    assert np.abs(rel @ fwd.astype(np.float64)).max() < 1e-5                    # the window lies in the plane through the origin
    assert np.abs(e1).max() <= hx * (1 + 1e-6) and np.abs(e2).max() <= hy * (1 + 1e-6)
    assert e1.min() < -hx * (1 - 2.0 / 37) and e1.max() > hx * (1 - 2.0 / 37) and e2.min() < -hy * (1 - 2.0 / 29) and e2.max() > hy * (1 - 2.0 / 29)
    one = rt3.make_params(37, 29)
    left_top = rt3.lens_ray(lens, one, 0, 0, 0)["origin"].astype(np.float64) - np.array(list(lens.origin), np.float64)
    assert left_top @ np.array(list(lens.right), np.float64) < 0 < left_top @ np.array(list(lens.up), np.float64)      # row 0 on top, column 0 on the left


def test_look_at_gives_an_accepted_right_handed_frame(rt3):
    rng = np.random.default_rng(4)
    p = rt3.make_params(8, 5)
    for _ in range(50):
        o, at, vup = rng.uniform(-50, 50, 3), rng.uniform(-50, 50, 3), rng.normal(size=3)
        lens = rt3.make_lens("equirect", o, at, vup)
        rt3.lens_ray(lens, p, 0, 0, 0)                                          # raises if the validation refuses it
        r, u, f = (np.array(list(v), np.float64) for v in (lens.right, lens.up, lens.forward))
        assert np.abs(np.cross(r, u) + f).max() < 1e-6
        want = (at - o) / np.linalg.norm(at - o)
        assert np.abs(f - want).max() < 1e-6 and u @ vup > 0
        assert np.array(list(lens.origin), F).tobytes() == o.astype(F).tobytes()
    lens = rt3.make_lens(rt3.LENS_FISHEYE, (0, 0, 0), (0, 0, -1), fov_deg=90.0, extent=(4.0, 2.0))
    assert lens.model == 2 and lens.half_fov_turns == F(0.125) and list(lens.half_extent) == [2.0, 1.0]
    assert list(lens.right) == [1.0, 0.0, 0.0] and list(lens.up) == [0.0, 1.0, 0.0] and list(lens.forward) == [0.0, 0.0, -1.0]


def refused(rt3, lens, w=8, h=5):
    out = np.zeros(1, L.RAY)
    p = rt3.make_params(w, h)
    return rt3.lib().rt3_debug_lens_ray(C.byref(lens), C.byref(p), 0, 0, 0, out.ctypes.data_as(C.c_void_p))


def test_every_refusal_of_a_lens(rt3, tmp_path):
    """Without a device: the validation every entry point shares, through the host law; the stub library's entry points answer "no device"."""
    def lens_of(model="equirect", **kw):
        lens = identity_lens(rt3, model)
        for k, v in kw.items():
            if isinstance(v, tuple):
                for c, x in enumerate(v):
                    getattr(lens, k)[c] = x
            else:
                setattr(lens, k, v)
        return lens
    assert refused(rt3, lens_of()) == 0
    for model in (0, 5, 0xFFFFFFFF):
        assert refused(rt3, lens_of(model=model)) == -1
    for bad in (np.nan, np.inf, -np.inf):
        for field in ("origin", "right", "up", "forward"):
            assert refused(rt3, lens_of(**{field: (bad, 0.0, 0.0)})) == -1, (field, bad)
    eps = 2.0 ** -20
    long_axis = float(np.sqrt(1.0 + 4 * eps))
    assert refused(rt3, lens_of(right=(long_axis, 0.0, 0.0))) == -1
    assert refused(rt3, lens_of(up=(0.0, 1.0 / long_axis, 0.0))) == -1
    assert refused(rt3, lens_of(forward=(0.0, 0.0, -2.0))) == -1
    assert refused(rt3, lens_of(forward=(0.0, 0.0, 0.0))) == -1
    assert refused(rt3, lens_of(right=(float(np.sqrt(1.0 + 0.25 * eps)), 0.0, 0.0))) == 0          # inside the band
    assert refused(rt3, lens_of(up=(4 * eps, 1.0, 0.0))) == -1                  # right . up
    assert refused(rt3, lens_of(forward=(0.0, 4 * eps, -1.0))) == -1            # up . forward
    assert refused(rt3, lens_of(right=(1.0, 0.0, 4 * eps))) == -1               # forward . right
    assert refused(rt3, lens_of(up=(0.25 * eps, 1.0, 0.0))) == 0
    for fov in (0.0, -0.1, 0.5000001, np.nan, np.inf):
        assert refused(rt3, lens_of("fisheye", half_fov_turns=fov)) == -1, fov
        assert refused(rt3, lens_of("equirect", half_fov_turns=fov)) == 0      # fields of other models are ignored
    assert refused(rt3, lens_of("fisheye", half_fov_turns=0.5)) == 0 and refused(rt3, lens_of("fisheye", half_fov_turns=1e-6)) == 0
    for ext in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (np.nan, 1.0), (1.0, np.inf)):
        assert refused(rt3, lens_of("ortho", half_extent=ext)) == -1, ext
        assert refused(rt3, lens_of("cube", half_extent=ext), 2, 12) == 0
    assert refused(rt3, lens_of("cube"), 8, 5) == -1 and refused(rt3, lens_of("cube"), 8, 47) == -1 and refused(rt3, lens_of("cube"), 8, 48) == 0
    # a pixel or sample outside the frame, NULL pointers
    out = np.zeros(1, L.RAY)
    fn = rt3.lib().rt3_debug_lens_ray
    lens, p = lens_of(), rt3.make_params(8, 5, spp=2)
    po = out.ctypes.data_as(C.c_void_p)
    assert fn(C.byref(lens), C.byref(p), 8, 0, 0, po) == -1 and fn(C.byref(lens), C.byref(p), 0, 5, 0, po) == -1
    assert fn(C.byref(lens), C.byref(p), 0, 0, 2, po) == -1 and fn(C.byref(lens), C.byref(p), 7, 4, 1, po) == 0
    assert fn(None, C.byref(p), 0, 0, 0, po) == -1 and fn(C.byref(lens), None, 0, 0, 0, po) == -1 and fn(C.byref(lens), C.byref(p), 0, 0, 0, None) == -1
    # the device entry points of the "no device" stubs
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    stubs = C.CDLL(str(so))
    ctx = C.c_void_p(0x10)                                                      # never dereferenced by a stub
    for name, args in (("rt3_lens_rays", (0, 1, po)), ("rt3_lens_rays_device", (0, 1, po, None)), ("rt3_render_lens", (0, 1, po)),
                       ("rt3_render_lens_device", (0, 1, po, None)), ("rt3_render_lens_aov", (po,)), ("rt3_render_lens_aov_device", (po, None))):
        fn = getattr(stubs, name)
        fn.restype = C.c_int
        assert fn(ctx, C.byref(lens), C.byref(p), *args) == -2, name
