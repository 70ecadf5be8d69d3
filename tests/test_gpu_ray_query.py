"""Batched ray queries (rt3_intersect* / rt3_occluded*) on the GPU: every kernel form's query equals the CPU oracle's Mode-X
nearest-hit rule with the t < t_max cut, and the unfiltered query, bit for bit (t compared by bit pattern, -0.0 included; kind and index by
equality); occlusion is exactly kind != NONE; invalid rays are flagged and disturb nothing."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_brute import random_soup

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
FORMS = {                                                             # environment of each kernel form (the scene decides between the rest)
    "default": {}, "nested_tiled": {"RT3_NO_RESIDENT": "1"},
    "levels3_res": {"RT3_LEVELS": "3"}, "levels3_tiled": {"RT3_LEVELS": "3", "RT3_NO_RESIDENT": "1"},
    "levels4_res": {"RT3_LEVELS": "4"}, "levels4_tiled": {"RT3_LEVELS": "4", "RT3_NO_RESIDENT": "1"},
}


# ------------------------------------------------------------------------------------------------ helpers
def upload(rt3, r, spheres=None, faces=None, verts=None):
    if faces is not None and len(faces):
        r.set_mesh(faces, verts)
    else:
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    if spheres is not None and len(spheres):
        m = np.zeros(len(spheres), rt3.MATERIAL)
        r.set_spheres(spheres, m)
    else:
        r.set_spheres(np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))


def query(r, rays, t_min, env=None, brute=False, monkeypatch=None):
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    r.force_brute(brute)
    try:
        hits = r.intersect(rays, t_min)
        occ = r.occluded(rays, t_min)
    finally:
        r.force_brute(False)
        if env:
            for k in env:
                monkeypatch.delenv(k)
    assert (hits["_pad"] == 0).all()
    expect_occ = np.where(hits["kind"] == 3, 0xFFFFFFFF, (hits["kind"] != 0).astype(np.uint32))
    assert np.array_equal(occ, expect_occ), "occlusion != nearest kind != NONE on %d rays" % int((occ != expect_occ).sum())
    return hits


def same(a, b, what=""):
    ta, tb = a["t"].view(np.uint32).copy(), b["t"].view(np.uint32).copy()
    ta[a["kind"] == 3] = tb[b["kind"] == 3] = 0                     # (an invalid ray's t is some NaN)
    bad = (ta != tb) | (a["kind"] != b["kind"]) | (a["index"] != b["index"])
    assert not bad.any(), "%s: %d of %d rays differ, first %s vs %s" % (what, int(bad.sum()), len(a), a[bad][:3], b[bad][:3])


def valid(rays, t_min):
    """rt3.h's validity rule: finite origin and direction, |fma(dz, dz, fma(dy, dy, dx * dx)) - 1| <= 2^-20, t_max > t_min (NaN fails)."""
    d = rays["direction"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dd = (d[:, 0] * d[:, 0]).astype(np.float32).astype(np.float64)
        dd = (d[:, 1] * d[:, 1] + dd).astype(np.float32).astype(np.float64)
        dd = (d[:, 2] * d[:, 2] + dd).astype(np.float32)
        ok = np.isfinite(rays["origin"]).all(axis=1) & np.isfinite(rays["direction"]).all(axis=1)
        return ok & (np.abs(dd - np.float32(1.0)) <= np.float32(2.0 ** -20)) & (rays["t_max"] > t_min)


def oracle_hits(rt3, oracle, rays, t_min, idx, spheres=None, faces=None, verts=None):
    """The oracle's nearest hit (running best from +inf) cut at t < t_max, for rays[idx]."""
    out = np.zeros(len(idx), rt3.HIT)
    ok = valid(rays, t_min)
    for n, i in enumerate(idx):
        ray = rays[i]
        if not ok[i]:
            out[n] = (np.float32(np.nan), 3, 0xFFFFFFFF, 0)
            continue
        kind, t, j = oracle.nearest(ray["origin"], ray["direction"], spheres=spheres, faces=faces, verts=verts, tmin=t_min)
        if kind != 0 and np.float32(t) < ray["t_max"]:
            out[n] = (np.float32(t), kind, j, 0)
        else:
            out[n] = (INF, 0, 0xFFFFFFFF, 0)
    return out


def unit(rng, n):
    v = rng.normal(0.0, 1.0, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def soup_rays(rt3, rng, n, spheres, scale):
    """Origins inside, outside and far (1e3 x extent) from the scene and exactly on sphere surfaces; t_max infinite, random and tiny."""
    lo, hi = np.float32([-3.0, -2.5, -7.5]) * scale, np.float32([3.0, 2.5, -1.0]) * scale
    ext = float(np.linalg.norm(hi - lo))
    k = n // 4
    o_in = rng.uniform(lo, hi, (k, 3))
    o_out = (lo + hi) / 2 + unit(rng, k) * ext * 1.5
    o_far = (lo + hi) / 2 + unit(rng, k) * ext * 1e3
    s = spheres[rng.integers(0, len(spheres), n - 3 * k)]
    o_surf = s[:, :3] + unit(rng, len(s)) * s[:, 3:4]
    o = np.concatenate([o_in, o_out, o_far, o_surf]).astype(np.float32)
    aim = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = np.where(rng.random((n, 1)) < 0.7, aim - o, unit(rng, n))      # most rays aimed into the scene, the rest anywhere
    tm = np.select([rng.random(n) < 0.4, rng.random(n) < 0.7], [np.float32(np.inf), rng.uniform(0.0, 2.0 * ext, n)], rng.uniform(1.5e-3 * scale, 3e-3 * scale, n))
    return rt3.make_rays(o, d, tm.astype(np.float32))


def primary_rays(rt3, cam, w, h):
    c = cam.c
    o, hor, ver, llc = (np.array(getattr(c, f), np.float32) for f in ("origin", "horizontal", "vertical", "lower_left_corner"))
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    u = (x / np.float32(w - 1)).reshape(-1, 1)
    v = ((np.float32(h - 1) - y) / np.float32(h - 1)).reshape(-1, 1)
    d = llc + u * hor + v * ver - o
    return rt3.make_rays(np.broadcast_to(o, d.shape), d)


def surface_rays(rt3, rng, n, spheres=None, faces=None, verts=None):
    """Incoherent rays: origins on the primitives' surfaces, random unit directions."""
    if spheres is not None:
        s = spheres[rng.integers(0, len(spheres), n)]
        o = s[:, :3] + unit(rng, n) * s[:, 3:4] * np.float32(1.0001)
    else:
        f = faces[rng.integers(0, len(faces), n)]
        p = [verts[f[k], :3] for k in ("v1", "v2", "v3")]
        a, b = rng.random((n, 1)), rng.random((n, 1))
        flip = (a + b) > 1.0
        a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
        o = p[0] + a * (p[1] - p[0]) + b * (p[2] - p[0])
    return rt3.make_rays(o.astype(np.float32), unit(rng, n))


# ------------------------------------------------------------------------------------------------ 1 / 6: random soups vs the oracle
@pytest.mark.parametrize("seed,scale,form", [(21, 1.0, "default"), (22, 1e3, "default"), (23, 1.0, "levels3_res"), (24, 1e3, "levels4_tiled")])
def test_random_soups_equal_oracle_and_brute(rt3, renderer, oracle, seed, scale, form, monkeypatch):
    rng = np.random.default_rng(seed)
    faces, verts, _, cr, _ = random_soup(rng, 700, 600, scale, rt3)
    upload(rt3, renderer, cr, faces, verts)
    rays = soup_rays(rt3, rng, 6000, cr, scale)
    for t_min in (np.float32(0.001 * scale), np.float32(0.0)):
        got = query(renderer, rays, t_min, FORMS[form], monkeypatch=monkeypatch)
        same(got, query(renderer, rays, t_min, brute=True), "query vs brute")
        idx = rng.choice(len(rays), 1500, replace=False)
        same(got[idx], oracle_hits(rt3, oracle, rays, t_min, idx, cr, faces, verts), "query vs oracle")
        kinds = np.bincount(got["kind"], minlength=4)
        assert kinds[1] > 100 and kinds[2] > 100 and kinds[0] > 100 and kinds[3] == 0, kinds      # not vacuous


# ------------------------------------------------------------------------------------------------ 2: every kernel form
@pytest.mark.parametrize("n_faces,n_sph", [(0, 480), (900, 0), (1301, 707)])
def test_every_kernel_form_gives_the_same_hits(rt3, renderer, n_faces, n_sph, monkeypatch):
    rng = np.random.default_rng(31 + n_faces + n_sph)
    faces, verts, _, cr, _ = random_soup(rng, n_faces, n_sph, 1.0, rt3)
    upload(rt3, renderer, cr if n_sph else None, faces if n_faces else None, verts)
    src = cr if n_sph else np.concatenate([verts[::3, :3], np.full((len(verts) // 3, 1), 0.1, np.float32)], axis=1)
    rays = soup_rays(rt3, rng, 8000, src, 1.0)
    ref = query(renderer, rays, np.float32(0.001), brute=True)
    forms = dict(FORMS)
    if n_sph and not n_faces:
        forms.update({"tiled_" + k: dict(v, RT3_FORCE_TILED="1") for k, v in FORMS.items()})     # default = k_trace_mfma32 (<= 512 spheres)
    for name, env in forms.items():
        same(query(renderer, rays, np.float32(0.001), env, monkeypatch=monkeypatch), ref, name)
        st = renderer.stats()
        assert st.filter_tests > 0 and st.mfma_instructions > 0, name                          # the matrix filter ran


@pytest.mark.parametrize("n", [112600, 112700])
def test_sphere_counts_around_the_resident_limit(rt3, renderer, oracle, n):
    """Both sides of the resident limit of the nested three-level form; 112 700 spheres reach k_trace_levels without any switch."""
    cr, _ = rt3.scene_stress(n, 3)
    upload(rt3, renderer, cr)
    rng = np.random.default_rng(n)
    cam = rt3.Camera().look_at(320, 180, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)
    rays = np.concatenate([primary_rays(rt3, cam, 320, 180), surface_rays(rt3, rng, 40000, spheres=cr)])
    got = query(renderer, rays, np.float32(0.001))
    st = renderer.stats()
    assert st.filter_tests // st.ray_casts == (-(-n // 64) if n <= 112640 else -(-(-(-n // 64)) // 8))     # which form ran
    same(got, query(renderer, rays, np.float32(0.001), brute=True), "query vs brute")
    if n > 112640:
        idx = rng.choice(len(rays), 2000, replace=False)
        same(got[idx], oracle_hits(rt3, oracle, rays, np.float32(0.001), idx, cr), "query vs oracle")


# ------------------------------------------------------------------------------------------------ 3: the benchmark scenes
@pytest.mark.parametrize("scene", ["weekend", "stress", "cornell"])
def test_benchmark_scenes(rt3, renderer, oracle, scene):
    rng = np.random.default_rng(7)
    sph = faces = verts = None
    if scene == "weekend":
        sph, _ = rt3.scene_weekend(42)
        cam = rt3.weekend_camera(640, 360)
    elif scene == "stress":
        sph, _ = rt3.scene_stress(100000, 43)
        cam = rt3.Camera().look_at(640, 360, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)
    else:
        faces, verts, _ = rt3.scene_cornell(64)
        cam = rt3.Camera().update(512, 288, 2.0, 2.0, 2.0)
    upload(rt3, renderer, sph, faces, verts)
    w, h = (cam.w(), cam.h())
    rays = np.concatenate([primary_rays(rt3, cam, w, h), surface_rays(rt3, rng, 1 << 18, sph, faces, verts)])
    got = query(renderer, rays, np.float32(0.001))
    same(got, query(renderer, rays, np.float32(0.001), brute=True), "query vs brute")
    idx = rng.choice(len(rays), 4096, replace=False)
    same(got[idx], oracle_hits(rt3, oracle, rays, np.float32(0.001), idx, sph, faces, verts), "query vs oracle")
    assert (got["kind"][: w * h] != 0).mean() > 0.3


# ------------------------------------------------------------------------------------------------ 4: t_max edges, grazing rays, |d|^2 = 1 +- 2^-21
def test_t_max_edges(rt3, renderer, oracle):
    rng = np.random.default_rng(41)
    faces, verts, _, cr, _ = random_soup(rng, 500, 400, 1.0, rt3)
    upload(rt3, renderer, cr, faces, verts)
    rays = soup_rays(rt3, rng, 8000, cr, 1.0)
    rays["t_max"] = INF
    t_min = np.float32(0.001)
    hit = query(renderer, rays, t_min)
    sel = np.nonzero(((hit["kind"] == 1) | (hit["kind"] == 2)) & (hit["t"] > t_min))[0]
    assert len(sel) > 1000
    at = rays[sel].copy()
    at["t_max"] = hit["t"][sel]                                       # a hit at exactly t_max is a miss ...
    got = query(renderer, at, t_min)
    assert (got["kind"] == 0).all() and (got["index"] == 0xFFFFFFFF).all() and np.isinf(got["t"]).all()
    at["t_max"] = np.nextafter(hit["t"][sel], INF)                    # ... one ulp beyond it, the same hit
    same(query(renderer, at, t_min), hit[sel], "t_max = nextafter(t)")
    idx = rng.choice(len(at), 500, replace=False)
    same(query(renderer, at, t_min)[idx], oracle_hits(rt3, oracle, at, t_min, idx, cr, faces, verts), "vs oracle")


def test_grazing_rays_and_direction_length_tolerance(rt3, renderer, oracle):
    """Rays that graze spheres at the rounding level of the exact test, with |d|^2 at 1 - 2^-21, 1 and 1 + 2^-21: all equal the oracle."""
    rng = np.random.default_rng(43)
    n = 960
    o = rng.uniform(-5.0, 5.0, (n, 3)).astype(np.float32)
    d = unit(rng, n)
    side = np.cross(d, unit(rng, n))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    dist = rng.uniform(3.0, 30.0, (n, 1))
    r = dist * rng.choice([1e-2, 1e-3], (n, 1))
    delta = rng.choice([-1e-6, -1e-7, 0.0, 1e-7, 1e-6], (n, 1))
    cr = np.concatenate([o + dist * d + r * (1.0 - delta) * side, r], axis=1).astype(np.float32)
    upload(rt3, renderer, cr)
    rays = rt3.make_rays(o, d)
    factor = np.float32(1.0) + np.float32(2.0 ** -22)
    rays["direction"][n // 3: 2 * n // 3] *= factor                  # |d|^2 ~ 1 + 2^-21
    rays["direction"][2 * n // 3:] /= factor                          # |d|^2 ~ 1 - 2^-21
    dd = np.abs((rays["direction"].astype(np.float64) ** 2).sum(axis=1) - 1.0)
    assert dd[n // 3:].min() > 2.0 ** -23 and dd.max() < 2.0 ** -20
    for t_min in (np.float32(0.0), np.float32(0.001)):
        got = query(renderer, rays, t_min)
        assert (got["kind"] != 3).all()
        same(got, oracle_hits(rt3, oracle, rays, t_min, np.arange(n), cr), "grazing vs oracle")
        assert 0.2 < (got["kind"] == 2).mean() < 0.95                # the edge cases go both ways


# ------------------------------------------------------------------------------------------------ 5: invalid rays inside valid waves
def test_invalid_rays_are_flagged_and_disturb_nothing(rt3, renderer):
    rng = np.random.default_rng(51)
    faces, verts, _, cr, _ = random_soup(rng, 300, 300, 1.0, rt3)
    upload(rt3, renderer, cr, faces, verts)
    rays = soup_rays(rt3, rng, 4096, cr, 1.0)
    t_min = np.float32(0.001)
    clean = query(renderer, rays, t_min)
    bad = rays.copy()
    pos = rng.choice(len(rays), 500, replace=False)
    for n, i in enumerate(pos):
        kind = n % 6
        if kind == 0:
            bad["origin"][i, 1] = np.nan
        elif kind == 1:
            bad["direction"][i] = 0.0
        elif kind == 2:
            bad["direction"][i] *= np.float32(1.001)
        elif kind == 3:
            bad["t_max"][i] = np.nan
        elif kind == 4:
            bad["t_max"][i] = t_min                                   # t_max <= t_min
        else:
            bad["direction"][i, 0] = np.inf
    assert not valid(bad, t_min)[pos].any() and valid(bad, t_min).sum() == len(rays) - len(pos)
    got = query(renderer, bad, t_min)
    assert (got["kind"][pos] == 3).all() and (got["index"][pos] == 0xFFFFFFFF).all() and np.isnan(got["t"][pos]).all()
    keep = np.setdiff1d(np.arange(len(rays)), pos)
    same(got[keep], clean[keep], "neighbours of invalid rays")
    assert renderer.stats().ray_casts == len(keep)
    all_bad = bad[pos]                                                # a batch of nothing but invalid rays
    assert (query(renderer, all_bad, t_min)["kind"] == 3).all()
    assert renderer.stats().ray_casts == 0


# ------------------------------------------------------------------------------------------------ 7: API behaviour
def test_stats_errors_and_repeatability(rt3, renderer):
    L = rt3.lib()
    upload(rt3, renderer)                                             # no scene
    rays = rt3.make_rays(np.zeros((8, 3)), np.tile([0.0, 0.0, -1.0], (8, 1)))
    hits = np.zeros(8, rt3.HIT)
    assert L.rt3_intersect(renderer._ctx, rays.ctypes.data_as(C.c_void_p), 8, np.float32(0.001), hits.ctypes.data_as(C.c_void_p)) == -4
    assert L.rt3_intersect(renderer._ctx, None, 0, np.float32(0.001), None) == 0                              # n = 0: nothing to do
    rng = np.random.default_rng(71)
    faces, verts, _, cr, _ = random_soup(rng, 400, 300, 1.0, rt3)
    upload(rt3, renderer, cr, faces, verts)
    assert L.rt3_intersect(renderer._ctx, None, 0, np.float32(0.001), None) == 0
    for bad_tmin in (-1.0, np.inf, np.nan):
        assert L.rt3_intersect(renderer._ctx, rays.ctypes.data_as(C.c_void_p), 8, np.float32(bad_tmin), hits.ctypes.data_as(C.c_void_p)) == -1
    assert L.rt3_intersect(renderer._ctx, rays.ctypes.data_as(C.c_void_p), (1 << 30) + 1, np.float32(0.0), hits.ctypes.data_as(C.c_void_p)) == -1
    rays = soup_rays(rt3, rng, 20000, cr, 1.0)
    a = renderer.intersect(rays)
    st = renderer.stats()
    valid = int((a["kind"] != 3).sum())
    assert st.ray_casts == valid and st.prim_tests == valid * 700 and st.samples == 0 and st.launches == 1
    assert st.trace_ms > 0 and st.filter_tests > 0 and st.exact_tests > 0 and st.n_spheres == 300 and st.n_faces == 400
    same(renderer.intersect(rays), a, "second run")
    import torch
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    buf = torch.zeros(len(rays) * 8 + 4, dtype=torch.float32, device="cuda")
    out = torch.zeros(len(rays) * 4 + 4, dtype=torch.int32, device="cuda")
    bad_rays = buf[1:1 + 8 * len(rays)]                              # 4-byte offset: misaligned
    assert L.rt3_intersect_device(renderer._ctx, C.c_void_p(bad_rays.data_ptr()), len(rays), np.float32(0.001), C.c_void_p(out.data_ptr()), None) == -1
    assert L.rt3_intersect_device(renderer._ctx, C.c_void_p(dev.data_ptr()), len(rays), np.float32(0.001), C.c_void_p(out[1:].data_ptr()), None) == -1
    assert L.rt3_occluded_device(renderer._ctx, C.c_void_p(dev.data_ptr()), len(rays), np.float32(0.001), C.c_void_p(out[1:].data_ptr()), None) == 0
    torch.cuda.synchronize()


def test_torch_round_trip_on_a_side_stream(rt3, renderer):
    import torch
    rng = np.random.default_rng(81)
    faces, verts, _, cr, _ = random_soup(rng, 400, 300, 1.0, rt3)
    upload(rt3, renderer, cr, faces, verts)
    rays = soup_rays(rt3, rng, 30000, cr, 1.0)
    want = renderer.intersect(rays)
    want_occ = renderer.occluded(rays)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda", non_blocking=False)
        t, kind, index = renderer.intersect(dev)
        occ = renderer.occluded(dev)
        t2 = t * 1.0                                                  # consumed on the same stream
    s.synchronize()
    host = lambda x: x.contiguous().cpu().numpy().view(np.uint32)   # noqa: E731
    assert np.array_equal(host(t), want["t"].view(np.uint32))
    assert np.array_equal(host(kind), want["kind"]) and np.array_equal(host(index), want["index"])
    assert np.array_equal(host(occ), want_occ)
    assert torch.equal(t2.isinf(), t.isinf())


def test_query_between_progressive_calls_leaves_the_accumulation(rt3, renderer):
    rng = np.random.default_rng(91)
    faces, verts, fm, cr, sm = random_soup(rng, 300, 200, 1.0, rt3)
    renderer.set_mesh(faces, verts, fm)
    renderer.set_spheres(cr, sm)
    cam = rt3.Camera().update(64, 48, 1.0, 3.0, 2.0)
    p = rt3.make_params(64, 48, spp=4, max_depth=6, seed=9, flags=1)
    whole = renderer.render_path(cam.c, p)
    renderer.render_path_range(cam.c, p, 0, 2)
    rays = soup_rays(rt3, rng, 50000, cr, 1.0)
    renderer.intersect(rays)
    renderer.occluded(rays)
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 2), whole)
