"""Image textures (rt3_set_texture*, rt3_bind_*_textures*) on the GPU.

Every comparison is by bit pattern.  oracle/ has no textures, so nothing here is compared with it: the first hit is pinned to the numpy restatement of
the law (tests/texture_ref.py) through the engine's own rays and hits, and deep paths are pinned by the law's two exact consequences — a white texture
changes no bit, a one-colour texture is a scaled material — under every kernel form, with the ties between the entry points on top."""
import ctypes as C
import os

import numpy as np
import pytest

import environment_ref as E
import texture_ref as T
from environment_sample_ref import fma32
from test_cli import run
from test_gpu_radiance import DEPTH, H, SEED, SPP, W, bits, params_of, same, scene, set_scene, soup, with_form
from test_gpu_ray_query import FORMS

pytestmark = pytest.mark.gpu

F = np.float32
E_ARG, E_STATE = -1, -4
DEEP = 8
ALL_FORMS = dict(FORMS, brute={"RT3_BRUTE": "1"})
WHITE = np.ones((1, 1, 3), F)
# slot -> (image, wrap): 8 x 8 beside the odd sizes 5 x 3 and 1 x 1, both wraps
TEXTURES = {0: (T.random_image(8, 8, seed=1), "repeat"), 1: (T.random_image(5, 3, seed=2), "clamp"), 2: (T.random_image(1, 1, seed=3), "repeat"),
            7: (T.random_image(5, 3, seed=4), "repeat"), 255: (T.random_image(8, 8, seed=5), "clamp")}
SLOTS = np.array(sorted(TEXTURES) + [T.NONE], np.uint32)


@pytest.fixture(autouse=True)
def nothing_afterwards(renderer):
    """The session's renderer is shared: whatever a test of this file did, and however it ended, no later test sees a texture, a binding or a map."""
    yield
    renderer.clear_textures()
    renderer.clear_environment()


def same_words(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%s: %d of %d bytes differ" % (what, int((a.view(np.uint8) != b.view(np.uint8)).sum()), a.nbytes)


def set_textures(r):
    for slot, (image, wrap) in TEXTURES.items():
        r.set_texture(slot, image, wrap)


def random_uv(n_faces, seed):
    """Six floats per face, reaching outside [0, 1]."""
    return np.random.default_rng(seed).uniform(-1.5, 2.5, (n_faces, 6)).astype(F)


def bind(r, kw, sph_slots=None, tri_slots=None, uv=None):
    if kw.get("spheres") is not None and len(kw["spheres"]):
        r.bind_sphere_textures(sph_slots)
    if kw.get("faces") is not None and len(kw["faces"]):
        r.bind_mesh_textures(tri_slots, uv)


def bind_everything(r, kw, slot, seed=0):
    n_sph = len(kw["spheres"]) if kw.get("spheres") is not None else 0
    n_faces = len(kw["faces"]) if kw.get("faces") is not None else 0
    s, t = T.bound_everything(n_sph, n_faces, slot)
    bind(r, kw, s, t, random_uv(n_faces, seed))


def first_hit_albedo(rt3, kw, rays, hits, sph_slots, tri_slots, uv, textures=TEXTURES):
    """rgb x texel of every ray's first hit by the law, from the engine's own rays and hits: float32 (n, 3) — a dielectric 1, a miss 0 — and the hit
    mask.  The sphere's hit point is fma(t, d, o) and its normal (p - C) * (1 / r), the face's point o + t d unfused: shade_lane's own."""
    o, d, t = rays["origin"].astype(F), rays["direction"].astype(F), hits["t"].astype(F)[:, None]
    out = np.zeros((len(rays), 3), F)
    for kind, mats, slots in ((rt3.HIT_SPHERE, kw.get("smats"), sph_slots), (rt3.HIT_FACE, kw.get("fmats"), tri_slots)):
        sel = np.nonzero(hits["kind"] == kind)[0]
        if not len(sel):
            continue
        idx = hits["index"][sel]
        m = mats[idx]
        if kind == rt3.HIT_SPHERE:
            cr = kw["spheres"][idx].astype(F)
            p = fma32(np.broadcast_to(t[sel], (len(sel), 3)), d[sel], o[sel])
            n = ((p - cr[:, :3]) * (F(1.0) / cr[:, 3:4])).astype(F)
            tex_uv = T.sphere_uv(n)
        else:
            f, v = kw["faces"][idx], kw["verts"].astype(F)
            p = (o[sel] + t[sel] * d[sel]).astype(F)
            tex_uv = T.face_uv(v[f["v1"], :3], v[f["v2"], :3], v[f["v3"], :3], uv[idx], p)
        rgb = m["rgb"].astype(F).copy()
        s = np.full(len(sel), T.NONE, np.uint32) if slots is None else slots[idx]
        for slot in np.unique(s[s != T.NONE]):
            image, wrap = textures[int(slot)]
            w = s == slot
            rgb[w] = T.modulate(rgb[w], T.lookup(image, tex_uv[w], T.CLAMP if wrap == "clamp" else T.REPEAT))
        rgb[m["kind"] == rt3.MAT_DIELECTRIC] = 1.0
        out[sel] = rgb
    return out, hits["kind"] != rt3.HIT_NONE


def flat(rt3, mats, seed):
    m = mats.copy()
    m["kind"] = rt3.MAT_FLAT
    m["rgb"] = np.random.default_rng(seed).uniform(0.1, 2.0, (len(m), 3))
    return m


# ------------------------------------------------------------------------------------------------ 1: the first hit is the law
@pytest.mark.parametrize("name", ["spheres61", "cornell4"])
def test_the_first_hit_is_the_law(rt3, renderer, name):
    """FLAT primitives, one sample, depth 1, a black background: the radiance of a pixel is rgb x texel of its first hit and nothing else."""
    if name == "spheres61":                                             # a ground sphere of radius 1000 and 60 small ones over it, seen from above the ground
        rng = np.random.default_rng(3)
        sph = np.zeros((61, 4), F)
        sph[0] = (0.0, -1000.0, 0.0, 1000.0)
        sph[1:, :3] = rng.uniform([-2.5, 0.2, -2.5], [2.5, 2.0, 1.0], (60, 3))
        sph[1:, 3] = rng.uniform(0.15, 0.5, 60)
        kw = dict(spheres=sph, smats=flat(rt3, np.zeros(61, rt3.MATERIAL), 1))
        cam = rt3.Camera().look_at(W, H, (0.0, 1.0, 4.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 50.0, 4.0)
    else:
        kw, cam, _, _ = scene(rt3, name)
        kw = dict(kw, fmats=flat(rt3, kw["fmats"], 2))
    set_scene(rt3, renderer, **kw)
    set_textures(renderer)
    rng = np.random.default_rng(5)
    n_sph, n_faces = len(kw.get("spheres", ())), len(kw.get("faces", ()))
    sph_slots, tri_slots, uv = rng.choice(SLOTS, n_sph), rng.choice(SLOTS, n_faces), random_uv(n_faces, 6)
    bind(renderer, kw, sph_slots, tri_slots, uv)
    p = rt3.make_params(W, H, spp=1, max_depth=1, seed=SEED, flags=rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)
    rays = renderer.camera_rays(cam.c, p, 0, 1)
    hits = renderer.intersect(rays, t_min=0.001)
    want, hit = first_hit_albedo(rt3, kw, rays, hits, sph_slots, tri_slots, uv)
    assert 100 < hit.sum() and len(np.unique(hits["index"][hit])) >= 8             # the frame shows many primitives
    want4 = np.concatenate([want, np.zeros((len(rays), 1), F)], axis=1)
    got = renderer.radiance(rays, samples=1, max_depth=1, seed=SEED, flags=rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)
    same(got, want4, name + ": rt3_radiance")
    renderer.render_path(cam.c, p)
    same(renderer.accum_resolve(p).reshape(-1, 4), want4, name + ": rt3_accum_resolve")
    bind(renderer, kw, None, None, None)                                # unbound: the plain colours, and they differ
    plain = renderer.radiance(rays, samples=1, max_depth=1, seed=SEED, flags=rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)
    assert (bits(plain) != bits(want4)).any(axis=1).sum() > 50


# ------------------------------------------------------------------------------------------------ 2: a white texture is no texture
def every_result(rt3, r, cam, lens_radius, flags):
    """What the entry points that read textures return for the scene on the context: a list of (name, array)."""
    p = rt3.make_params(W, H, spp=SPP, max_depth=DEEP, seed=SEED, flags=flags, lens_radius=lens_radius, t_min=0.001)
    out = [("render", r.render_path(cam.c, p)), ("resolve", r.accum_resolve(p))]
    r.render_path_range(cam.c, p, 0, 2)
    out.append(("range", r.render_path_range(cam.c, p, 2, 2)))
    ps = [rt3.make_params(W, H, spp=SPP, max_depth=DEEP, seed=SEED, flags=flags, lens_radius=lens_radius, t_min=0.001, tile_rows=4, tile_index=i, tile_count=3)
          for i in range(3)]
    out.append(("shards", rt3.deinterleave([r.render_path(cam.c, q) for q in ps], ps, H, W)))
    p8 = rt3.make_params(W, H, spp=8, max_depth=DEEP, seed=SEED, flags=flags, lens_radius=lens_radius, t_min=0.001)
    pixels, counts = r.render_adaptive(cam.c, p8, threshold=0.02, min_spp=2, step_spp=2)
    out += [("adaptive", pixels), ("counts", counts)]
    rays = r.camera_rays(cam.c, p, 0, 1)
    out.append(("radiance", r.radiance(rays, samples=2, max_depth=DEEP, seed=SEED, flags=flags & rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)))
    out.append(("aov", r.render_aov(cam.c, p)))
    lens = rt3.make_lens("fisheye", tuple(cam.c.origin), (0.0, 0.0, -3.0), fov_deg=170.0)
    pl = rt3.make_params(W, H, spp=2, max_depth=DEEP, seed=SEED, flags=flags & rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)
    out.append(("lens", r.render_lens(lens, pl)))
    return out


@pytest.mark.parametrize("name", ["weekend", "three", "cornell4"])
def test_a_white_texture_is_no_texture(rt3, renderer, name):
    """Each texture form is its twin with ONE difference, and a texel of (1, 1, 1) makes that difference vanish: rgb * 1 = rgb."""
    kw, cam, lens_radius, _ = scene(rt3, name)
    set_scene(rt3, renderer, **kw)
    renderer.set_texture(3, WHITE)
    cube = E.random_cube(5, seed=11)
    for with_map in (False, True):
        if with_map:
            renderer.set_environment(cube)
        for flags in (rt3.FLAG_GAMMA2, rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND):
            bind(renderer, kw, None, None, None)
            want = every_result(rt3, renderer, cam, lens_radius, flags)
            bind_everything(renderer, kw, 3)
            got = every_result(rt3, renderer, cam, lens_radius, flags)
            for (what, a), (_, b) in zip(got, want):
                same_words(a, b, "%s, map %s, flags %d: %s" % (name, with_map, flags, what))
            if not flags & rt3.FLAG_BLACK_BACKGROUND:                   # (weekend and the three spheres have no light of their own)
                assert (dict(want)["counts"] > 2).any()                 # the list rounds ran


# ------------------------------------------------------------------------------------------------ 3: a constant texture is a scaled material
@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_a_constant_texture_is_a_scaled_material(rt3, renderer, name):
    kw, cam, lens_radius, _ = scene(rt3, name)
    c = np.array([0.7, 0.45, 1.25], F)
    scaled = dict(kw)
    for k in ("smats", "fmats"):
        if kw.get(k) is not None:
            m = kw[k].copy()
            m["rgb"] = np.float32(m["rgb"]) * np.float32(c)
            scaled[k] = m
    p = rt3.make_params(W, H, spp=SPP, max_depth=DEEP, seed=SEED, flags=rt3.FLAG_GAMMA2, lens_radius=lens_radius, t_min=0.001)
    rays = renderer.camera_rays(cam.c, p, 0, 1)

    def results():
        return [renderer.render_path(cam.c, p), renderer.accum_resolve(p), renderer.radiance(rays, samples=2, max_depth=DEEP, seed=SEED, t_min=0.001),
                renderer.render_aov(cam.c, p)]
    set_scene(rt3, renderer, **scaled)
    want = results()
    set_scene(rt3, renderer, **kw)
    plain = results()
    assert (plain[0] != want[0]).mean() > 0.2
    for w_, h_ in ((1, 1), (5, 3)):
        renderer.set_texture(4, np.broadcast_to(c, (h_, w_, 3)), "clamp" if w_ == 5 else "repeat")
        bind_everything(renderer, kw, 4)
        for g, w, what in zip(results(), want, ("pixels", "accum_resolve", "radiance", "aov")):
            same_words(g, w, "%s, %d x %d: %s" % (name, w_, h_, what))


# ------------------------------------------------------------------------------------------------ 4: the forms agree
@pytest.mark.parametrize("n_faces,n_sph", [(0, 480), (900, 0), (1301, 707)])
def test_every_kernel_form_equals_the_unfiltered_form(rt3, renderer, n_faces, n_sph, monkeypatch):
    rng = np.random.default_rng(261 + n_faces + n_sph)
    rays, (faces, verts, fm, cr, sm) = soup(rt3, renderer, rng, n_faces, n_sph, 2048)
    kw = dict(spheres=cr if n_sph else None, faces=faces if n_faces else None)
    set_textures(renderer)
    bind(renderer, kw, rng.choice(SLOTS, n_sph), rng.choice(SLOTS, n_faces), random_uv(n_faces, 9))
    if n_faces and n_sph:
        renderer.set_environment(E.random_cube(5, seed=4))              # one class of scenes with a map: the forms' run-time branch at a miss
    call = lambda: renderer.radiance(rays, samples=2, max_depth=DEPTH, seed=5)      # noqa: E731
    ref = with_form(renderer, {"RT3_BRUTE": "1"}, monkeypatch, call)
    st = renderer.stats()
    assert st.mfma_instructions == 0 and st.ray_casts > 2 * 2048 and not np.isnan(ref).any()
    forms = dict(FORMS)
    if n_sph and not n_faces:
        forms.update({"tiled_" + k: dict(v, RT3_FORCE_TILED="1") for k, v in FORMS.items()})     # default = k_trace_mfma32 (<= 512 spheres)
    for name, env in forms.items():
        same(with_form(renderer, env, monkeypatch, call), ref, name)
        assert renderer.stats().mfma_instructions > 0 and renderer.stats().ray_casts == st.ray_casts, name
    for env in ({"RT3_NO_MFMA": "1"}, {"RT3_NO_GROUPS": "1"}, {"RT3_MFMA_K64": "1"}):              # switches of families without such a form: ignored
        same(with_form(renderer, env, monkeypatch, call), ref, str(env))
        assert renderer.stats().mfma_instructions > 0
    bind(renderer, kw, None, None, None)
    assert (bits(call()) != bits(ref)).any()                           # the textures reach the result


# ------------------------------------------------------------------------------------------------ 5: the ties hold
def textured_scene(rt3, r, name, seed):
    kw, cam, lens_radius, _ = scene(rt3, name)
    set_scene(rt3, r, **kw)
    set_textures(r)
    rng = np.random.default_rng(seed)
    n_sph = len(kw["spheres"]) if kw.get("spheres") is not None else 0
    n_faces = len(kw["faces"]) if kw.get("faces") is not None else 0
    sph_slots, tri_slots, uv = rng.choice(SLOTS, n_sph), rng.choice(SLOTS, n_faces), random_uv(n_faces, seed + 1)
    bind(r, kw, sph_slots, tri_slots, uv)
    return kw, cam, lens_radius, (sph_slots, tri_slots, uv)


@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_radiance_over_camera_rays_is_the_render(rt3, renderer, name):
    kw, cam, lens_radius, _ = textured_scene(rt3, renderer, name, 31)
    p = params_of(rt3, 1, lens_radius)
    keys = np.arange(W * H, dtype=np.uint32)                           # the pixel index: the defining property of rt3.h
    total = np.zeros((W * H, 3), F)
    for s in range(SPP):
        rays = renderer.camera_rays(cam.c, p, s, 1)
        total = total + renderer.radiance(rays, keys=keys, sample_begin=s, samples=1, max_depth=DEPTH, seed=SEED, t_min=0.001)[:, :3]
    want = np.concatenate([total / F(SPP), np.zeros((W * H, 1), F)], axis=1)
    renderer.render_path(cam.c, p)
    same(renderer.accum_resolve(p).reshape(-1, 4), want, "%s: render vs summed single samples" % name)


@pytest.mark.parametrize("name", ["weekend", "stress3000", "cornell4+spheres"])
def test_adaptive_pixels_are_their_own_sample_range(rt3, renderer, name, monkeypatch):
    kw, cam, lens_radius, _ = textured_scene(rt3, renderer, name, 41)
    p = rt3.make_params(W, H, spp=8, max_depth=DEPTH, seed=SEED, flags=1, lens_radius=lens_radius, t_min=0.001)
    adaptive = lambda: renderer.render_adaptive(cam.c, p, threshold=0.02, min_spp=2, step_spp=2)     # noqa: E731
    pixels, counts = adaptive()
    assert set(np.unique(counts)) <= {2, 4, 6, 8} and len(np.unique(counts)) >= 2 and (counts > 2).sum() > 64       # list rounds ran
    for n in np.unique(counts):
        whole = renderer.render_path_range(cam.c, p, 0, int(n))
        assert np.array_equal(pixels[counts == n], whole[counts == n]), n
    for form, env in ALL_FORMS.items():
        px, ct = with_form(renderer, env, monkeypatch, adaptive)
        assert np.array_equal(ct, counts) and np.array_equal(px, pixels), form


# ------------------------------------------------------------------------------------------------ 6: AOVs
@pytest.mark.parametrize("name", ["weekend", "cornell4+spheres"])
def test_aov_albedo_is_the_modulated_one(rt3, renderer, name):
    kw, cam, lens_radius, (sph_slots, tri_slots, uv) = textured_scene(rt3, renderer, name, 51)
    p = rt3.make_params(W, H, spp=1, max_depth=DEPTH, seed=SEED, flags=rt3.FLAG_GAMMA2 | rt3.FLAG_BLACK_BACKGROUND, lens_radius=lens_radius, t_min=0.001)
    aov = renderer.render_aov(cam.c, p).reshape(-1)
    rays = renderer.camera_rays(cam.c, p, 0, 1)
    hits = renderer.intersect(rays, t_min=0.001)
    want, hit = first_hit_albedo(rt3, kw, rays, hits, sph_slots, tri_slots, uv)
    assert np.array_equal(aov["kind"], hits["kind"]) and np.array_equal(aov["index"][hit], hits["index"][hit]) and 100 < hit.sum()
    same(aov["albedo"], want, name + ": albedo")
    mats = kw["smats"]
    glass = hit & (hits["kind"] == rt3.HIT_SPHERE) & (mats["kind"][np.minimum(hits["index"], len(mats) - 1)] == rt3.MAT_DIELECTRIC)
    assert glass.sum() > 0 and (aov["albedo"][glass] == 1.0).all()     # a dielectric stays 1 whatever its binding
    bind(renderer, kw, None, None, None)
    before = renderer.render_aov(cam.c, p).reshape(-1)
    assert (bits(before["albedo"]) != bits(aov["albedo"])).any()
    for f in ("coverage", "normal", "depth", "kind", "index"):
        assert np.array_equal(aov[f].tobytes(), before[f].tobytes()), f


# ------------------------------------------------------------------------------------------------ 7: state
def test_bindings_survive_updates_and_go_with_uploads(rt3, renderer):
    kw, cam, lens_radius, (sph_slots, tri_slots, uv) = textured_scene(rt3, renderer, "cornell4+spheres", 61)
    p = params_of(rt3, 1, lens_radius)
    lit = renderer.render_path(cam.c, p)
    renderer.update_spheres(kw["spheres"])
    renderer.update_mesh(kw["verts"])
    renderer.regroup()
    same_words(renderer.render_path(cam.c, p), lit, "after no-op updates and a regroup")
    renderer.set_spheres(kw["spheres"], kw["smats"])                    # a full upload of the spheres: their binding goes, the faces' stays
    half = renderer.render_path(cam.c, p)
    assert (half != lit).any()
    renderer.bind_sphere_textures(sph_slots)
    same_words(renderer.render_path(cam.c, p), lit, "the spheres bound again")
    renderer.set_mesh(kw["faces"], kw["verts"], kw["fmats"])            # and the other way round
    assert (renderer.render_path(cam.c, p) != lit).any()
    renderer.bind_mesh_textures(tri_slots, uv)
    same_words(renderer.render_path(cam.c, p), lit, "the faces bound again")
    renderer.set_spheres(kw["spheres"], kw["smats"])
    renderer.set_mesh(kw["faces"], kw["verts"], kw["fmats"])
    plain = renderer.render_path(cam.c, p)
    renderer.clear_textures()                                           # no binding: the slots do not matter
    same_words(renderer.render_path(cam.c, p), plain, "no binding")
    assert renderer.texture_size(0) == (0, 0, "repeat")
    set_textures(renderer)
    assert renderer.texture_size(1) == (5, 3, "clamp") and renderer.texture_size(255) == (8, 8, "clamp") and renderer.texture_size(9) == (0, 0, "repeat")
    bind(renderer, kw, sph_slots, tri_slots, uv)
    same_words(renderer.render_path(cam.c, p), lit, "everything set again")
    bind(renderer, kw, np.full(len(sph_slots), T.NONE, np.uint32), np.full(len(tri_slots), T.NONE, np.uint32), uv)
    same_words(renderer.render_path(cam.c, p), plain, "bindings of RT3_TEX_NONE alone")


def test_refusals_leave_the_state_alone(rt3, renderer):
    L, ctx, vp = rt3.lib(), renderer._ctx, C.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                                # noqa: E731
    kw, cam, lens_radius, (sph_slots, tri_slots, uv) = textured_scene(rt3, renderer, "cornell4+spheres", 71)
    p = params_of(rt3, 1, lens_radius)
    lit = renderer.render_path(cam.c, p)
    out = np.zeros((H, W), np.uint32)
    err = lambda: L.rt3_last_error(ctx).decode()                        # noqa: E731
    rgba = np.ascontiguousarray(np.concatenate([T.random_image(5, 3, seed=9)[..., :3], np.zeros((3, 5, 1), F)], axis=2))
    bad = rgba.copy()
    bad[2, 1, 1] = np.nan                                               # texel 2 * 5 + 1 = 11
    bad[2, 3, 0] = np.inf
    bad[0, 0, 3] = np.nan                                               # the fourth channel is ignored
    assert L.rt3_set_texture(ctx, 1, ptr(bad), 5, 3, 0) == E_ARG and "texel 11 " in err()
    with pytest.raises(rt3.Fatal, match="texel 11 "):
        renderer.set_texture(1, bad)
    for args in ((256, ptr(rgba), 5, 3, 0), (1, None, 5, 3, 0), (1, ptr(rgba), 8193, 1, 0), (1, ptr(rgba), 1, 8193, 0), (1, ptr(rgba), 5, 3, 2)):
        assert L.rt3_set_texture(ctx, *args) == E_ARG, args
    import torch
    dev = torch.zeros(5 * 3 * 4 + 4, dtype=torch.float32, device="cuda")
    assert L.rt3_set_texture_device(ctx, 1, vp(dev[1:].data_ptr()), 5, 3, 0, None) == E_ARG          # 4 bytes off
    assert L.rt3_set_texture_device(ctx, 1, None, 5, 3, 0, None) == E_ARG
    assert L.rt3_set_texture_device(ctx, 256, vp(dev.data_ptr()), 5, 3, 0, None) == E_ARG
    w = C.c_uint32(9)
    assert L.rt3_texture_size(ctx, 256, C.byref(w), None, None) == E_ARG and w.value == 9
    # bindings: a slot index out of range (the lowest is named), a wrong count, a NULL uv, a uv that is not finite
    s_bad = sph_slots.copy()
    s_bad[[5, 17]] = (256, 300)
    assert L.rt3_bind_sphere_textures(ctx, ptr(s_bad), len(s_bad)) == E_ARG and "sphere 5:" in err()
    assert L.rt3_bind_sphere_textures(ctx, ptr(sph_slots), len(sph_slots) - 1) == E_ARG
    t_bad = tri_slots.copy()
    t_bad[[9, 3]] = (0xFFFFFFFE, 256)
    assert L.rt3_bind_mesh_textures(ctx, ptr(t_bad), ptr(uv), len(t_bad)) == E_ARG and "face 3:" in err()
    assert L.rt3_bind_mesh_textures(ctx, ptr(tri_slots), None, len(tri_slots)) == E_ARG
    assert L.rt3_bind_mesh_textures(ctx, ptr(tri_slots), ptr(uv), len(tri_slots) + 1) == E_ARG
    uv_bad = uv.copy()
    uv_bad[7, 4], uv_bad[20, 0] = np.inf, np.nan
    assert L.rt3_bind_mesh_textures(ctx, ptr(tri_slots), ptr(uv_bad), len(tri_slots)) == E_ARG and "face 7:" in err()
    d_bad = torch.from_numpy(s_bad.view(np.int32)).to("cuda")
    assert L.rt3_bind_sphere_textures_device(ctx, vp(d_bad.data_ptr()), len(s_bad), None) == E_ARG and "sphere 5:" in err()
    assert L.rt3_bind_sphere_textures_device(ctx, vp(d_bad.data_ptr() + 2), len(s_bad), None) == E_ARG
    same_words(renderer.render_path(cam.c, p), lit, "after the refused calls")
    assert renderer.texture_size(1) == (5, 3, "clamp")
    # the flags refused while textured
    for flag, word in ((rt3.FLAG_ENV_SAMPLING, "SAMPLING"), (rt3.FLAG_LIGHT_SAMPLING, "SAMPLING")):
        q = rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=SEED, flags=1 | flag, lens_radius=lens_radius, t_min=0.001)
        renderer.set_environment(E.random_cube(2, seed=1))
        assert L.rt3_render_path(ctx, C.byref(cam.c), C.byref(q), ptr(out)) == E_ARG and word in err() and "textures" in err()
        renderer.clear_environment()
    rays = renderer.camera_rays(cam.c, p, 0, 1)
    with pytest.raises(rt3.Fatal, match="textures"):
        renderer.radiance(rays, samples=1, max_depth=2, flags=rt3.FLAG_LIGHT_SAMPLING)
    renderer.set_spheres(np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))       # a face-only scene for RT3_FLAG_REFERENCE_PRIMARY
    cam0 = rt3.main_camera(W, H)
    pr = rt3.make_params(W, H, spp=1, max_depth=1, seed=1, flags=rt3.FLAG_REFERENCE_PRIMARY, t_min=0.0)
    assert L.rt3_render_path(ctx, C.byref(cam0.c), C.byref(pr), ptr(out)) == E_ARG and "textures" in err()
    renderer.bind_mesh_textures(None, None)
    assert L.rt3_render_path(ctx, C.byref(cam0.c), C.byref(pr), ptr(out)) == 0
    # a binding that names an empty slot: RT3_E_STATE from every reader, until the slot is set again
    set_scene(rt3, renderer, **kw)
    bind(renderer, kw, sph_slots, tri_slots, uv)
    renderer.set_texture(7, None)
    assert renderer.texture_size(7) == (0, 0, "repeat")
    assert L.rt3_render_path(ctx, C.byref(cam.c), C.byref(p), ptr(out)) == E_STATE and "slot 7" in err()
    for call in (lambda: renderer.render_aov(cam.c, p), lambda: renderer.radiance(rays, samples=1, max_depth=2),
                 lambda: renderer.render_adaptive(cam.c, p, min_spp=2, step_spp=2)):
        with pytest.raises(rt3.Fatal, match="slot 7"):
            call()
    renderer.intersect(rays)                                            # the queries read no texture
    renderer.set_texture(7, *TEXTURES[7])
    same_words(renderer.render_path(cam.c, p), lit, "the slot set again")
    # binding a class that has no scene
    set_scene(rt3, renderer, spheres=kw["spheres"], smats=kw["smats"])
    assert L.rt3_bind_mesh_textures(ctx, ptr(tri_slots), ptr(uv), len(tri_slots)) == E_STATE
    assert L.rt3_bind_mesh_textures(ctx, None, None, 0) == 0
    set_scene(rt3, renderer, faces=kw["faces"], verts=kw["verts"], fmats=kw["fmats"])
    assert L.rt3_bind_sphere_textures(ctx, ptr(sph_slots), len(sph_slots)) == E_STATE
    assert L.rt3_bind_sphere_textures(ctx, None, 0) == 0


def test_device_forms_equal_the_host_forms(rt3, renderer):
    import torch
    kw, cam, lens_radius, (sph_slots, tri_slots, uv) = textured_scene(rt3, renderer, "cornell4+spheres", 81)
    p = params_of(rt3, 1, lens_radius)
    lit = renderer.render_path(cam.c, p)
    renderer.clear_textures()
    set_scene(rt3, renderer, **kw)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for slot, (image, wrap) in TEXTURES.items():
            t = torch.from_numpy(np.ascontiguousarray(image)).to("cuda")
            renderer.set_texture(slot, t, wrap)
            t.zero_()                                                  # queued behind the copy: the context owns its own
        ds = torch.from_numpy(sph_slots.view(np.int32)).to("cuda")
        dt = torch.from_numpy(tri_slots.view(np.int32)).to("cuda")
        du = torch.from_numpy(uv).to("cuda")
        renderer.bind_sphere_textures(ds)
        renderer.bind_mesh_textures(dt, du)
        ds.fill_(-1), dt.fill_(-1), du.zero_()
    s.synchronize()
    assert renderer.texture_size(1) == (5, 3, "clamp")
    same_words(renderer.render_path(cam.c, p), lit, "torch device forms")
    renderer.set_texture(0, T.random_image(3, 2, seed=12))              # another size into a slot that is bound, and back
    assert (renderer.render_path(cam.c, p) != lit).any()
    renderer.set_texture(0, *TEXTURES[0])
    same_words(renderer.render_path(cam.c, p), lit, "a slot replaced and restored")
    with pytest.raises(rt3.Fatal):
        renderer.set_texture(0, torch.zeros((3, 2, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(rt3.Fatal):
        renderer.bind_mesh_textures(dt, du[:5])


# ------------------------------------------------------------------------------------------------ 8: the command line
def test_cli_textures_give_the_frame_of_the_api_render(rt3, renderer, tmp_path):
    w, h = 32, 18
    a, b = T.random_image(5, 3, seed=21, channels=3), T.random_image(8, 8, seed=22, channels=3)
    (tmp_path / "a.pfm").write_bytes(rt3.pfm_bytes(a))
    (tmp_path / "b.pfm").write_bytes(rt3.pfm_bytes(b))
    rc, out, err = run("-f", "ppm", "-W", str(w), "-H", str(h), "--scene", "three", "--spp", "4", "--depth", "6", "--seed", "9",
                       "--texture", str(tmp_path / "a.pfm") + ",clamp", "--texture", str(tmp_path / "b.pfm"), "--bind-sphere", "all=1", "--bind-sphere", "0=0",
                       "--hdr", str(tmp_path / "lin.pfm"), "--aov", str(tmp_path / "A"), str(tmp_path / "three.ppm"))
    assert rc == 0, err
    sph, sm = rt3.scene_three_spheres()
    set_scene(rt3, renderer, sph, sm)
    renderer.set_texture(0, a, "clamp")
    renderer.set_texture(1, b)
    slots = np.full(len(sph), 1, np.uint32)
    slots[0] = 0
    renderer.bind_sphere_textures(slots)
    cam = rt3.Camera().update(w, h, 1.0, F(w) / F(h) * F(2.0), 2.0)
    p = rt3.make_params(w, h, spp=4, max_depth=6, seed=9, flags=rt3.FLAG_GAMMA2, t_min=0.001)
    frame = rt3.Frame(w, h)
    frame.data[:] = renderer.render_path(cam.c, p)
    assert (tmp_path / "three.ppm").read_bytes() == frame.ppm_bytes()
    assert (tmp_path / "lin.pfm").read_bytes() == rt3.pfm_bytes(renderer.accum_resolve(p)[..., :3])
    assert (tmp_path / "A.albedo.pfm").read_bytes() == rt3.pfm_bytes(renderer.render_aov(cam.c, p)["albedo"])
    renderer.bind_sphere_textures(None)
    assert (renderer.render_path(cam.c, p) != frame.data).any()
    rc, out, err = run("-f", "ppm", "-W", str(w), "-H", str(h), "--scene", "three", "--spp", "4", "--texture", str(tmp_path / "a.pfm"),
                       "--bind-sphere", "99=0", str(tmp_path / "no.ppm"))
    assert rc == -1 and "fatal:" in err and "no sphere 99" in err and not os.path.exists(tmp_path / "no.ppm")
    rc, out, err = run("-f", "ppm", "--scene", "three", "--spp", "4", "--texture", str(tmp_path / "none.pfm"), str(tmp_path / "no.ppm"))
    assert rc == -1 and "Could not open" in err
