"""Lens models (rt3_lens_rays*, rt3_render_lens*, rt3_render_lens_aov*) on the GPU.

Every comparison is by bit pattern.  The device's rays must be the host law's (rt3_debug_lens_ray, itself pinned to tests/lens_ref.py without a device);
a lens frame must be the composition its defining property names — per-sample rt3_radiance calls over those rays with frame-pixel keys, summed in f32
in sample order and divided; every kernel route must equal the unfiltered kernel; batching and sharding must not show; the AOVs must be
test_gpu_aov.expected_aov of the lens rays and their rt3_intersect hits (sphere normals to 2^-20, the tolerance that helper's own test gives the
hit point it rounds twice); the accumulation, the statistics, the device forms, the refusals and the command line."""
import ctypes as C

import numpy as np
import pytest

import environment_ref as E
import lens_ref as L
from test_cli import run
from test_gpu_aov import expected_aov
from test_gpu_radiance import same, scene, set_scene, soup, with_form
from test_gpu_ray_query import FORMS

pytestmark = pytest.mark.gpu

W, H = 37, 29                                                         # 1073 pixels: no multiple of 64 or of the 256-item work chunk, a ragged last row block
N = 5                                                                 # the cube frame: 5 x 30
DEPTH, SEED = 6, 11
E_ARG, E_STATE = -1, -4
MODELS = ("equirect", "fisheye", "ortho", "cube")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def size_of(model):
    return (N, 6 * N) if model == "cube" else (W, H)


INSIDE = ((0.15, 0.35, -2.2), (-0.2, -0.3, -3.6), (0.05, 1.0, 0.0))     # a point inside the Cornell box (x, y in [-1, 1], z in [-4, -2]), clear of its two boxes


def lens_of(rt3, model, cam=None):
    """A lens of the model: at a camera's place, looking where it looks; "inside": within the Cornell box, so that the whole sphere of directions meets
    geometry; default: an off-axis point."""
    if cam == "inside":
        return rt3.make_lens(model, *INSIDE, fov_deg=150.0, extent=(3.0, 2.4))
    if cam is not None:
        o = np.array(list(cam.c.origin), np.float64)
        h, v, l = (np.array(list(x), np.float64) for x in (cam.c.horizontal, cam.c.vertical, cam.c.lower_left_corner))
        at = l + 0.5 * h + 0.5 * v
        return rt3.make_lens(model, o, at, v, fov_deg=150.0, extent=(3.0, 2.4))
    return rt3.make_lens(model, (0.3, 0.4, 0.5), (0.0, -0.1, -3.0), (0.05, 1.0, 0.0), fov_deg=150.0, extent=(3.0, 2.4))


def params_of(rt3, model, spp=4, flags=0, **tiles):
    w, h = size_of(model)
    return rt3.make_params(w, h, spp=spp, max_depth=DEPTH, seed=SEED, flags=flags, t_min=0.001, **tiles)


def host_law(rt3, lens, p, sample_begin=0, sample_count=None):
    """rt3_debug_lens_ray in rt3_lens_rays' order over the pixels the shard owns."""
    rows = [rt3.row_of_local(p, k) for k in range(rt3.rows_owned(p))]
    sc = p.spp - sample_begin if sample_count is None else sample_count
    out = np.zeros((sc, len(rows), p.width), L.RAY)
    for s in range(sc):
        for k, y in enumerate(rows):
            for x in range(p.width):
                out[s, k, x] = rt3.lens_ray(lens, p, x, y, sample_begin + s)
    return out.reshape(-1)


def composition(rt3, r, lens, p, sample_begin=0, sample_count=None):
    """The defining property of rt3_render_lens: per-sample rt3_radiance over the lens rays, keyed by the frame pixel index."""
    sc = p.spp - sample_begin if sample_count is None else sample_count
    rows = [rt3.row_of_local(p, k) for k in range(rt3.rows_owned(p))]
    keys = np.concatenate([y * p.width + np.arange(p.width) for y in rows]).astype(np.uint32)
    flags = p.flags & (rt3.FLAG_BLACK_BACKGROUND | rt3.FLAG_ENV_SAMPLING | rt3.FLAG_LIGHT_SAMPLING)
    total = np.zeros((len(keys), 3), np.float32)
    for s in range(sample_begin, sample_begin + sc):
        rays = r.lens_rays(lens, p, s, 1)
        total = total + r.radiance(rays, keys=keys, sample_begin=s, samples=1, max_depth=p.max_depth, seed=p.seed, flags=flags, t_min=p.t_min)[:, :3]
    return np.concatenate([total / np.float32(sc), np.zeros((len(keys), 1), np.float32)], axis=1)


# ------------------------------------------------------------------------------------------------ 1: the device's rays are the host law's
@pytest.mark.parametrize("spp", (1, 3, 4))
@pytest.mark.parametrize("model", MODELS)
def test_device_rays_equal_the_host_law(rt3, renderer, model, spp):
    lens = lens_of(rt3, model)
    p = params_of(rt3, model, spp=spp)
    got = renderer.lens_rays(lens, p)
    assert got.dtype == rt3.RAY and len(got) == p.width * p.height * spp
    assert got.tobytes() == host_law(rt3, lens, p).tobytes(), (model, spp)
    assert got.tobytes() == L.frame_rays(lens, p).tobytes()
    if spp > 1:                                                       # a sample sub-range, and the three shards of the ragged frame
        assert renderer.lens_rays(lens, p, 1, spp - 1).tobytes() == got[p.width * p.height:].tobytes()
        seen = 0
        for i in range(3):
            q = params_of(rt3, model, spp=spp, tile_rows=4, tile_index=i, tile_count=3)
            tile = renderer.lens_rays(lens, q, spp - 2, 2)
            assert tile.tobytes() == host_law(rt3, lens, q, spp - 2, 2).tobytes(), (model, spp, i)
            seen += len(tile)
        assert seen == 2 * p.width * p.height


# ------------------------------------------------------------------------------------------------ 2: a lens frame is its defining composition
CASES = [("three", 0), ("three", 2), ("cornell4", 0), ("cornell4", 2), ("cornell4+spheres", 0), ("cornell4+spheres", 2)]


@pytest.mark.parametrize("name,flags", CASES)
def test_render_lens_equals_the_composition(rt3, renderer, name, flags):
    kw, cam, _, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    lit = 0
    for model in MODELS:
        lens = lens_of(rt3, model, cam if name == "three" else "inside")
        p = params_of(rt3, model, flags=flags | rt3.FLAG_GAMMA2)      # (GAMMA2: accepted and ignored)
        got = renderer.render_lens(lens, p)
        assert got.shape == (p.height, p.width, 4)
        same(got.reshape(-1, 4), composition(rt3, renderer, lens, p), "%s %s flags %d" % (name, model, flags))
        assert not np.isnan(got).any() and (bits(got[..., 3]) == 0).all()
        lit += int((got[..., :3] != 0).any(axis=-1).sum())
    if name == "three" and flags & rt3.FLAG_BLACK_BACKGROUND:
        assert lit == 0                                               # no emitter and no sky: exactly black
    else:
        assert lit >= 64                                              # not a comparison of zeros with zeros


def test_render_lens_with_a_map_and_with_the_samplers(rt3, renderer):
    kw, cam, _, _ = scene(rt3, "cornell4+spheres")
    set_scene(rt3, renderer, **kw)
    try:
        renderer.set_environment(E.random_cube(5, seed=5))
        for model, flags in (("equirect", 0), ("cube", rt3.FLAG_ENV_SAMPLING), ("fisheye", rt3.FLAG_ENV_SAMPLING), ("ortho", rt3.FLAG_LIGHT_SAMPLING)):
            lens = lens_of(rt3, model, "inside")
            p = params_of(rt3, model, flags=flags)
            got = renderer.render_lens(lens, p)
            same(got.reshape(-1, 4), composition(rt3, renderer, lens, p), "map, %s flags %d" % (model, flags))
            assert (got[..., :3] != 0).any(axis=-1).mean() > 0.3
    finally:
        renderer.clear_environment()
    for model, flags in (("equirect", rt3.FLAG_LIGHT_SAMPLING), ("cube", rt3.FLAG_LIGHT_SAMPLING | rt3.FLAG_BLACK_BACKGROUND)):
        lens = lens_of(rt3, model, "inside")
        p = params_of(rt3, model, flags=flags)
        plain = renderer.render_lens(lens, params_of(rt3, model, flags=flags & rt3.FLAG_BLACK_BACKGROUND))
        got = renderer.render_lens(lens, p)
        same(got.reshape(-1, 4), composition(rt3, renderer, lens, p), "light sampling, %s flags %d" % (model, flags))
        assert (bits(got) != bits(plain)).any()                       # the shadow rays reach the result


# ------------------------------------------------------------------------------------------------ 3: every kernel route equals the unfiltered kernel
@pytest.mark.parametrize("model", ("equirect", "ortho"))
def test_every_kernel_route_equals_the_unfiltered_kernel(rt3, renderer, model, monkeypatch):
    rng = np.random.default_rng(91)
    soup(rt3, renderer, rng, 301, 207, 64)
    lens = rt3.make_lens(model, (0.2, 0.1, -4.0), (0.0, 0.0, -5.0), (0.0, 1.0, 0.0), extent=(7.0, 6.0))     # inside the soup's box
    p = params_of(rt3, model, spp=3)
    call = lambda: renderer.render_lens(lens, p)                      # noqa: E731
    renderer.force_brute(True)
    try:
        ref = call()
        st = renderer.stats()
        assert st.mfma_instructions == 0 and st.ray_casts > 3 * W * H and st.samples == 3 * W * H and st.launches == 3
    finally:
        renderer.force_brute(False)
    assert not np.isnan(ref).any() and (ref[..., :3] != 0).any(axis=-1).mean() > 0.2
    for name, env in FORMS.items():
        same(with_form(renderer, env, monkeypatch, call).reshape(-1, 4), ref.reshape(-1, 4), name)
        assert renderer.stats().mfma_instructions > 0 and renderer.stats().ray_casts == st.ray_casts, name


# ------------------------------------------------------------------------------------------------ 4: batching and sharding do not show
def test_batching_and_shards(rt3, renderer):
    kw, cam, _, _ = scene(rt3, "cornell4+spheres")
    set_scene(rt3, renderer, **kw)
    lens = lens_of(rt3, "equirect", "inside")
    big = rt3.make_params(131, 97, spp=4, max_depth=DEPTH, seed=SEED, t_min=0.001)       # 44 B x 12 707 pixels > half a MiB: the smallest cap holds one sample
    one_batch = renderer.render_lens(lens, big)
    st = renderer.stats()
    assert st.samples == 4 * 131 * 97 and st.launches == 4            # one trace launch per sample
    aov_one_batch = renderer.render_lens_aov(lens, big)
    assert renderer.stats().launches == 1
    try:
        renderer.set_sample_storage_cap(1 << 20)                      # the smallest cap: one sample per batch
        batched = renderer.render_lens(lens, big)
        st1 = renderer.stats()
        aov_batched = renderer.render_lens_aov(lens, big)
        assert renderer.stats().launches == 4
    finally:
        renderer.set_sample_storage_cap(16 << 30)
    assert batched.tobytes() == one_batch.tobytes() and st1.launches == 4 and st1.ray_casts == st.ray_casts
    assert aov_batched.tobytes() == aov_one_batch.tobytes()
    p = params_of(rt3, "equirect", spp=4)
    whole = renderer.render_lens(lens, p)
    aov1 = renderer.render_lens_aov(lens, p)
    ps = [params_of(rt3, "equirect", spp=4, tile_rows=4, tile_index=i, tile_count=3) for i in range(3)]
    for q in ps:
        rows = [rt3.row_of_local(q, k) for k in range(rt3.rows_owned(q))]
        tile = renderer.render_lens(lens, q)
        assert tile.shape == (len(rows), W, 4) and tile.tobytes() == whole[rows].tobytes(), q.tile_index
        assert renderer.render_lens_aov(lens, q).tobytes() == aov1[rows].tobytes(), q.tile_index
    part = renderer.render_lens(lens, p, 1, 2)                        # a sample sub-range is its own composition
    same(part.reshape(-1, 4), composition(rt3, renderer, lens, p, 1, 2), "samples [1, 3)")


# ------------------------------------------------------------------------------------------------ 5: the AOVs
@pytest.mark.parametrize("model", MODELS)
def test_lens_aov_equals_the_composition(rt3, renderer, model):
    kw, cam, _, _ = scene(rt3, "cornell4+spheres")
    set_scene(rt3, renderer, **kw)
    lens = lens_of(rt3, model, "inside")
    for spp, flags in ((1, 0), (4, rt3.FLAG_BLACK_BACKGROUND), (3, 0)):
        p = params_of(rt3, model, spp=spp, flags=flags)
        rays = renderer.lens_rays(lens, p)
        hits = renderer.intersect(rays, p.t_min)
        got = renderer.render_lens_aov(lens, p).reshape(-1)
        assert renderer.stats().samples == p.width * p.height * spp
        want, sph = expected_aov(rt3, rays, hits, spp, flags, kw.get("spheres"), kw.get("smats"), kw.get("faces"), kw.get("fmats"))
        what = "%s spp %d" % (model, spp)
        for f in ("kind", "index"):
            assert np.array_equal(got[f], want[f]), what + " " + f
        for f in ("depth", "coverage", "albedo"):
            assert np.array_equal(bits(got[f]), bits(want[f])), what + " " + f
        assert np.array_equal(bits(got["normal"][~sph]), bits(want["normal"][~sph])), what + " face normals"
        assert np.abs(got["normal"][sph] - want["normal"][sph]).max(initial=0.0) <= 2.0 ** -20, what + " sphere normals"
        assert (got["_pad"] == 0).all() and (got["coverage"] > 0).mean() > 0.2


def test_lens_aov_miss_albedo_with_a_map(rt3, renderer):
    sph, sm = rt3.scene_three_spheres()
    set_scene(rt3, renderer, spheres=sph, smats=sm)
    lens = rt3.make_lens("equirect", (0.0, 0.5, 1.0), (0.0, 0.0, -1.0))
    p = params_of(rt3, "equirect", spp=1)
    before = renderer.render_lens_aov(lens, p)
    cube = E.random_cube(16, seed=8)
    try:
        renderer.set_environment(cube)
        aov = renderer.render_lens_aov(lens, p)
    finally:
        renderer.clear_environment()
    d = renderer.lens_rays(lens, p)["direction"].reshape(H, W, 3)
    miss = aov["kind"] == rt3.HIT_NONE
    assert 50 < miss.sum() < W * H - 50
    assert np.array_equal(bits(aov["albedo"][miss]), bits(E.lookup(cube, d[miss])))
    assert aov[~miss].tobytes() == before[~miss].tobytes()


# ------------------------------------------------------------------------------------------------ 6: context state and statistics
def test_the_accumulation_is_left_alone_and_the_stats_add_up(rt3, renderer):
    kw, cam, lens_radius, _ = scene(rt3, "three")
    set_scene(rt3, renderer, **kw)
    cp = rt3.make_params(W, H, spp=4, max_depth=DEPTH, seed=SEED, flags=1, lens_radius=lens_radius, t_min=0.001)
    want = renderer.render_path(cam.c, cp)
    renderer.render_path_range(cam.c, cp, 0, 2)
    lens = lens_of(rt3, "fisheye", cam)
    p = params_of(rt3, "fisheye", spp=4)
    frame = renderer.render_lens(lens, p)
    st = renderer.stats()
    assert st.samples == 4 * W * H and st.launches == 4 and st.ray_casts > 4 * W * H and st.trace_ms > 0 and st.total_ms >= st.trace_ms
    assert st.filter_tests == st.ray_casts * len(kw["spheres"])       # k_trace_mfma32's rays form: every cast takes the matrix filter
    casts = 0
    for s in range(4):
        renderer.render_lens(lens, p, s, 1)
        one = renderer.stats()
        assert one.samples == W * H and one.launches == 1
        casts += one.ray_casts
    assert casts == st.ray_casts
    renderer.render_lens_aov(lens, p)
    renderer.lens_rays(lens, p)
    assert np.array_equal(renderer.render_path_range(cam.c, cp, 2, 2), want)       # continued bit-exactly across the lens calls
    assert frame.tobytes() == renderer.render_lens(lens, p).tobytes()


# ------------------------------------------------------------------------------------------------ 7: device forms
def test_device_forms_equal_the_host_forms(rt3, renderer):
    import torch
    kw, cam, _, _ = scene(rt3, "cornell4+spheres")
    set_scene(rt3, renderer, **kw)
    for model in ("equirect", "cube"):
        lens = lens_of(rt3, model, "inside")
        p = params_of(rt3, model, spp=4)
        rays, frame, aov = renderer.lens_rays(lens, p), renderer.render_lens(lens, p), renderer.render_lens_aov(lens, p)
        t_rays, t_frame, t_aov = renderer.lens_rays(lens, p, device=True), renderer.render_lens(lens, p, device=True), renderer.render_lens_aov(lens, p, device=True)
        torch.cuda.synchronize()
        assert t_rays.cpu().numpy().tobytes() == rays.tobytes() and t_frame.shape == frame.shape
        assert t_frame.cpu().numpy().tobytes() == frame.tobytes() and t_aov.cpu().numpy().tobytes() == aov.tobytes()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            s_frame = renderer.render_lens(lens, p, 1, 3, device="cuda")
            s_copy = s_frame.clone()                                  # queued behind the render on the side stream
        side.synchronize()
        assert s_copy.cpu().numpy().tobytes() == renderer.render_lens(lens, p, 1, 3).tobytes()
        q = params_of(rt3, model, spp=4, tile_rows=4, tile_index=1, tile_count=3)
        assert renderer.render_lens(lens, q, device=True).cpu().numpy().tobytes() == renderer.render_lens(lens, q).tobytes()


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_argument_errors_leave_the_context_usable(rt3, renderer):
    import torch
    kw, cam, _, _ = scene(rt3, "three")
    set_scene(rt3, renderer, **kw)
    lib, ctx, vp = rt3.lib(), renderer._ctx, C.c_void_p
    lens = lens_of(rt3, "equirect", cam)
    good = params_of(rt3, "equirect", spp=4)
    want = renderer.render_lens(lens, good)
    out = np.zeros((H, W, 12), np.float32)
    o = out.ctypes.data_as(vp)

    def refused(code, word, fn, *args):
        assert fn(ctx, *args) == code, (fn.__name__, word)
        assert word.encode() in lib.rt3_last_error(ctx), (word, lib.rt3_last_error(ctx))

    def render(p, lens_=lens, sb=0, sc=None):
        return (C.byref(lens_), C.byref(p), sb, p.spp if sc is None else sc, o)
    for flag, word in ((rt3.FLAG_REFERENCE_PRIMARY, "REFERENCE_PRIMARY"), (8, "VARIANCE"), (64, "unknown bits")):
        refused(E_ARG, word, lib.rt3_render_lens, *render(params_of(rt3, "equirect", flags=flag)))
    bad = params_of(rt3, "equirect")
    bad.lens_radius = 0.05
    refused(E_ARG, "lens_radius", lib.rt3_render_lens, *render(bad))
    refused(E_ARG, "lens_radius", lib.rt3_render_lens_aov, C.byref(lens), C.byref(bad), o)
    refused(E_ARG, "sample range", lib.rt3_render_lens, *render(good, sb=2, sc=3))
    refused(E_ARG, "sample range", lib.rt3_render_lens, *render(good, sc=0))
    refused(E_ARG, "sample range", lib.rt3_lens_rays, *render(good, sb=4, sc=1))
    refused(E_ARG, "cube", lib.rt3_render_lens, *render(good, lens_=lens_of(rt3, "cube", cam)))
    crooked = lens_of(rt3, "equirect", cam)
    crooked.up[0] += 0.01
    for fn, args in ((lib.rt3_lens_rays, render(good, crooked)), (lib.rt3_render_lens, render(good, crooked)),
                     (lib.rt3_render_lens_aov, (C.byref(crooked), C.byref(good), o))):
        refused(E_ARG, "lens:", fn, *args)
    refused(E_ARG, "NULL", lib.rt3_render_lens, None, C.byref(good), 0, 4, o)
    refused(E_ARG, "NULL", lib.rt3_render_lens, C.byref(lens), None, 0, 4, o)
    refused(E_ARG, "NULL", lib.rt3_render_lens, C.byref(lens), C.byref(good), 0, 4, None)
    refused(E_ARG, "ENV_SAMPLING", lib.rt3_render_lens, *render(params_of(rt3, "equirect", flags=rt3.FLAG_ENV_SAMPLING | rt3.FLAG_LIGHT_SAMPLING)))
    refused(E_ARG, "BLACK_BACKGROUND", lib.rt3_render_lens, *render(params_of(rt3, "equirect", flags=rt3.FLAG_ENV_SAMPLING | rt3.FLAG_BLACK_BACKGROUND)))
    refused(E_STATE, "environment map", lib.rt3_render_lens, *render(params_of(rt3, "equirect", flags=rt3.FLAG_ENV_SAMPLING)))
    dev = torch.zeros(W * H * 12 + 4, dtype=torch.float32, device="cuda")
    for fn, args in ((lib.rt3_lens_rays_device, (C.byref(lens), C.byref(good), 0, 1, vp(dev[1:].data_ptr()), None)),
                     (lib.rt3_render_lens_device, (C.byref(lens), C.byref(good), 0, 4, vp(dev[1:].data_ptr()), None)),
                     (lib.rt3_render_lens_aov_device, (C.byref(lens), C.byref(good), vp(dev[1:].data_ptr()), None))):
        refused(E_ARG, "16-byte aligned", fn, *args)
    with pytest.raises(rt3.Fatal, match="sample range"):
        renderer.render_lens(lens, good, 3, 2)
    set_scene(rt3, renderer)                                           # no scene: the renders refuse, the rays do not need one
    refused(E_STATE, "no scene", lib.rt3_render_lens, *render(good))
    refused(E_STATE, "no scene", lib.rt3_render_lens_aov, C.byref(lens), C.byref(good), o)
    assert len(renderer.lens_rays(lens, good)) == 4 * W * H
    set_scene(rt3, renderer, **kw)
    assert renderer.render_lens(lens, good).tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ 9: the command line
def read_pfm(path):
    with open(path, "rb") as f:
        magic = f.readline().strip()
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0
        ch = 3 if magic == b"PF" else 1
        return np.frombuffer(f.read(), "<f4").reshape(h, w, ch)[::-1]


def test_cli_writes_what_the_python_calls_return(rt3, renderer, tmp_path):
    w, h, spp = 64, 32, 4
    names = {k: str(tmp_path / k) for k in ("o.ppm", "h.pfm", "a", "d.pfm")}
    rc, out, err = run("--scene", "three", "--spp", str(spp), "--depth", "6", "--seed", "3", "-W", str(w), "-H", str(h), "--lens", "equirect",
                       "--hdr", names["h.pfm"], "--aov", names["a"], "--denoise", names["d.pfm"], "-f", "ppm", names["o.ppm"])
    assert rc == 0, err
    sph, sm = rt3.scene_three_spheres()
    set_scene(rt3, renderer, spheres=sph, smats=sm)
    lens = rt3.make_lens("equirect", (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    p = rt3.make_params(w, h, spp=spp, max_depth=6, seed=3, flags=rt3.FLAG_GAMMA2, t_min=0.001)
    frame, aov = renderer.render_lens(lens, p), renderer.render_lens_aov(lens, p)
    assert read_pfm(names["h.pfm"]).tobytes() == np.ascontiguousarray(frame[..., :3]).tobytes()
    assert read_pfm(names["a"] + ".albedo.pfm").tobytes() == np.ascontiguousarray(aov["albedo"]).tobytes()
    assert read_pfm(names["a"] + ".normal.pfm").tobytes() == np.ascontiguousarray(aov["normal"]).tobytes()
    assert read_pfm(names["a"] + ".depth.pfm")[..., 0].tobytes() == np.ascontiguousarray(aov["depth"]).tobytes()
    den = renderer.denoise(frame, aov)
    assert read_pfm(names["d.pfm"]).tobytes() == np.ascontiguousarray(den[..., :3]).tobytes()
    words = renderer.display(frame, curve="clamp", transfer="gamma2")  # the transform that reproduces the ordinary Mode-X pack
    body = open(names["o.ppm"], "rb").read()
    rgb = np.stack([(words >> 24) & 0xFF, (words >> 16) & 0xFF, (words >> 8) & 0xFF], axis=-1).astype(np.uint8)
    assert body.endswith(rgb.tobytes()) and len(body) > 3 * w * h
