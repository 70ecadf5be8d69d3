"""Specular-chain AOVs (rt3_render_aov_specular*, rt3_render_lens_aov_specular*) on the GPU.

Zero bounces are the first-hit AOVs byte for byte; every other output is the numpy restatement of the law (aov_chain_ref.py) with the engine's own
rt3_intersect as its tracer, bit for bit, and where a chain ends on an emitter or the sky its albedo is the radiance the path tracer returns."""
import ctypes as C

import numpy as np
import pytest

import aov_chain_ref as R
import cases
import environment_ref
import texture_ref as T

pytestmark = pytest.mark.gpu

F = np.float32
E_ARG, E_STATE = -1, -4
DEFAULT_CAP = 16 << 30


@pytest.fixture(autouse=True)
def nothing_afterwards(renderer):
    """The session's renderer is shared: no later test sees a texture, a map or a small sample storage cap."""
    yield
    renderer.clear_textures()
    renderer.clear_environment()
    renderer.set_sample_storage_cap(DEFAULT_CAP)


def same_bytes(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%s: %d of %d records differ" % (what, int((a.reshape(-1) != b.reshape(-1)).sum()), a.size)


def upload(rt3, r, scene):
    cases.hip_upload(r, scene)
    r.clear_textures()
    r.clear_environment()
    tex = scene.get("textures")
    if tex is not None:
        for slot, (image, wrap) in tex["images"].items():
            r.set_texture(slot, image, wrap)
        if tex.get("sph_tex") is not None:
            r.bind_sphere_textures(tex["sph_tex"])
        if tex.get("tri_tex") is not None:
            r.bind_mesh_textures(tex["tri_tex"], tex["tri_uv"])
    if scene.get("env") is not None:
        r.set_environment(scene["env"])


# ------------------------------------------------------------------------------------------------ scenes
def weekend(rt3):
    c = cases.mode_x_cases()["weekend_96x54x4_d50_lens"]
    return dict(spheres=c["spheres"], smats=c["smats"]), c["cam"], dict(c["params"])


def cornell(rt3):
    c = cases.mode_x_cases()["cornell_g4_48x48x8_d6_black"]
    return dict(faces=c["faces"], verts=c["verts"], fmats=c["fmats"]), c["cam"], dict(c["params"])


def cornell_mirror_glass(rt3):
    """The Cornell box with every third face a fuzz-0 mirror, every third a pane of glass."""
    scene, cam, params = cornell(rt3)
    fm = scene["fmats"].copy()
    k = np.arange(len(fm))
    fm["kind"][k % 3 == 0], fm["param"][k % 3 == 0] = rt3.MAT_METAL, 0.0
    fm["kind"][k % 3 == 1], fm["param"][k % 3 == 1] = rt3.MAT_DIELECTRIC, 1.5
    return dict(scene, fmats=fm), cam, params


def textured(rt3, metal_only=False):
    """The three spheres, every one bound to a texture (the metal one among them), under an environment map."""
    cr, sm = rt3.scene_three_spheres()
    sm = sm.copy()
    if metal_only:
        sm["kind"], sm["param"] = rt3.MAT_METAL, 0.0
    images = {0: (T.random_image(8, 8, seed=1), "repeat"), 3: (T.random_image(5, 3, seed=2), "clamp")}
    sph_tex = np.array([0, 3, 0, 3, 0, 3][:len(cr)], np.uint32)
    scene = dict(spheres=cr, smats=sm, textures=dict(images=images, sph_tex=sph_tex), env=environment_ref.random_cube(8, seed=3))
    cam = rt3.Camera().update(48, 48, 1.0, 2.0, 2.0)
    return scene, cam.c, dict(width=48, height=48, spp=2, max_depth=8, seed=3, flags=0)


def anchor_scene(rt3):
    """Two fuzz-0 mirrors that face each other across a row of emitters of distinct colours."""
    rng = np.random.default_rng(11)
    cr = [[-1.6, 0.0, -4.0, 1.2], [1.6, 0.0, -4.0, 1.2]]
    kinds = [rt3.MAT_METAL, rt3.MAT_METAL]
    for k in range(12):
        cr.append([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(-6.5, -1.5), rng.uniform(0.15, 0.4)])
        kinds.append(rt3.MAT_FLAT)
    cr.append([0.0, -101.5, -4.0, 100.0])
    kinds.append(rt3.MAT_FLAT)
    sm = np.zeros(len(cr), rt3.MATERIAL)
    sm["rgb"], sm["kind"] = rng.uniform(0.2, 0.95, (len(cr), 3)), kinds
    cam = rt3.Camera().update(48, 48, 1.0, 2.0, 2.0)
    return dict(spheres=np.array(cr, F), smats=sm), cam.c


def restate(rt3, r, scene, rays, p, max_bounces, max_fuzz):
    return R.chain_aov(rays, lambda q: r.intersect(q, p.t_min), scene, max_bounces, max_fuzz, p.spp, rt3.AOV, rt3.RAY,
                       black=bool(p.flags & rt3.FLAG_BLACK_BACKGROUND))


# ------------------------------------------------------------------------------------------------ 1: zero bounces
@pytest.mark.parametrize("name", ["weekend", "cornell", "textured"])
def test_zero_bounces_are_the_first_hit_aovs(rt3, renderer, name):
    scene, cam, params = {"weekend": weekend, "cornell": cornell, "textured": textured}[name](rt3)
    upload(rt3, renderer, scene)
    p = rt3.make_params(**params)
    first = renderer.render_aov(cam, p)
    same_bytes(renderer.render_aov_specular(cam, p, max_bounces=0, max_fuzz=0.0), first, name)
    same_bytes(renderer.render_aov_specular(cam, p, max_bounces=0, max_fuzz=1.0), first, name)
    lens = rt3.make_lens("equirect", (0.0, 1.0, 3.0), (0.0, 0.5, -1.0))
    lp = rt3.make_params(32, 16, spp=3, seed=2, flags=params["flags"] & rt3.FLAG_BLACK_BACKGROUND)
    same_bytes(renderer.render_lens_aov_specular(lens, lp, max_bounces=0), renderer.render_lens_aov(lens, lp), name + " lens")


def test_a_scene_without_mirrors_or_glass_has_nothing_to_follow(rt3, renderer):
    scene, cam, params = cornell(rt3)
    assert not np.isin(scene["fmats"]["kind"], (rt3.MAT_METAL, rt3.MAT_DIELECTRIC)).any()
    upload(rt3, renderer, scene)
    p = rt3.make_params(**params)
    same_bytes(renderer.render_aov_specular(cam, p, max_bounces=8, max_fuzz=1.0), renderer.render_aov(cam, p))
    assert renderer.stats().ray_casts == 48 * 48 * p.spp              # one query's worth: every chain ended at its first hit


# ------------------------------------------------------------------------------------------------ 2: the restatement
@pytest.mark.parametrize("max_fuzz", [0.0, 1.0])
@pytest.mark.parametrize("max_bounces", [1, 4, 16])
def test_weekend_is_the_restatement(rt3, renderer, max_bounces, max_fuzz):
    scene, cam, params = weekend(rt3)
    upload(rt3, renderer, scene)
    p = rt3.make_params(**dict(params, spp=3))
    rays = renderer.camera_rays(cam, p)
    want, info = restate(rt3, renderer, scene, rays, p, max_bounces, max_fuzz)
    got = renderer.render_aov_specular(cam, p, max_bounces=max_bounces, max_fuzz=max_fuzz)
    st = renderer.stats()
    same_bytes(got.reshape(-1), want, "weekend")
    assert st.ray_casts == info["casts"] and st.samples == 96 * 54 * 3
    assert st.launches <= max_bounces + 1
    assert info["bounces"].max() >= min(max_bounces, 2)               # through the glass sphere and out again


@pytest.mark.parametrize("name", ["mesh", "textured_metal"])
def test_mesh_and_textured_metal_are_the_restatement(rt3, renderer, name):
    scene, cam, params = cornell_mirror_glass(rt3) if name == "mesh" else textured(rt3, metal_only=True)
    upload(rt3, renderer, scene)
    p = rt3.make_params(**dict(params, spp=2))
    rays = renderer.camera_rays(cam, p)
    want, info = restate(rt3, renderer, scene, rays, p, 6, 0.0)
    got = renderer.render_aov_specular(cam, p, max_bounces=6, max_fuzz=0.0)
    assert renderer.stats().ray_casts == info["casts"]
    same_bytes(got.reshape(-1), want, name)
    assert (info["bounces"] >= 2).sum() > 0                           # chains of several bounces
    if name == "textured_metal":                                      # the texel is in the throughput: the albedo differs from the untextured scene's
        plain = dict(scene, textures=None)
        assert not np.array_equal(restate(rt3, renderer, plain, rays, p, 6, 0.0)[0]["albedo"], want["albedo"])


@pytest.mark.parametrize("model,w,h", [("equirect", 32, 16), ("cube", 8, 48)])
def test_lens_frames_are_the_restatement(rt3, renderer, model, w, h):
    scene, _, _ = weekend(rt3)
    upload(rt3, renderer, scene)
    lens = rt3.make_lens(model, (3.0, 1.0, 2.5), (0.0, 1.0, 0.0))
    p = rt3.make_params(w, h, spp=3, seed=4)
    rays = renderer.lens_rays(lens, p)
    want, info = restate(rt3, renderer, scene, rays, p, 8, 0.0)
    got = renderer.render_lens_aov_specular(lens, p, max_bounces=8, max_fuzz=0.0)
    assert renderer.stats().ray_casts == info["casts"]
    same_bytes(got.reshape(-1), want, model)
    assert (info["bounces"] >= 1).sum() > 20


# ------------------------------------------------------------------------------------------------ 3: the anchor to the renderer
@pytest.mark.parametrize("flags", [0, 2])
def test_albedo_is_the_radiance_where_the_path_is_deterministic(rt3, renderer, flags):
    scene, cam = anchor_scene(rt3)
    upload(rt3, renderer, scene)
    p = rt3.make_params(48, 48, spp=1, seed=9, flags=flags)
    rays = renderer.camera_rays(cam, p)
    want, info = restate(rt3, renderer, scene, rays, p, 8, 0.0)
    got = renderer.render_aov_specular(cam, p, max_bounces=8, max_fuzz=0.0).reshape(-1)
    same_bytes(got, want)
    rad = renderer.radiance(rays, samples=1, max_depth=9, seed=9, flags=flags)
    ended = (info["end"] == R.END_MISS) | ((info["end"] == R.END_SURFACE) & (info["end_kind"] == rt3.MAT_FLAT))
    assert ended.sum() > 0.8 * len(rays)
    assert ((info["bounces"] >= 2) & ended).sum() >= 10               # not vacuous: chains of two and more bounces among them
    assert ((info["bounces"] == 1) & ended).sum() >= 100
    same_bytes(got["albedo"][ended], rad[ended, :3], "albedo against rt3_radiance")


# ------------------------------------------------------------------------------------------------ 4: batching and forms
def test_batches_device_form_shards_and_the_accumulation(rt3, renderer):
    import torch
    scene, cam, params = weekend(rt3)
    upload(rt3, renderer, scene)
    p = rt3.make_params(**params)
    whole = renderer.render_aov_specular(cam, p, max_bounces=4, max_fuzz=0.0)
    launches = renderer.stats().launches
    # several batches: 96 B per pixel and sample, 1 MiB holds two of the four samples of 96 x 54 pixels
    renderer.set_sample_storage_cap(1 << 20)
    same_bytes(renderer.render_aov_specular(cam, p, max_bounces=4, max_fuzz=0.0), whole, "two batches")
    assert renderer.stats().launches > launches
    renderer.set_sample_storage_cap(DEFAULT_CAP)
    # the device form on a stream of the caller's
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = torch.zeros((54, 96, 12), dtype=torch.float32, device="cuda")
        renderer.render_aov_specular_device(cam, p, out.data_ptr(), stream.cuda_stream, max_bounces=4, max_fuzz=0.0)
    stream.synchronize()
    same_bytes(out.cpu().numpy().view(rt3.AOV).reshape(54, 96), whole, "device form")
    lens = rt3.make_lens("equirect", (3.0, 1.0, 2.5), (0.0, 1.0, 0.0))
    lp = rt3.make_params(32, 16, spp=2, seed=4)
    dev = renderer.render_lens_aov_specular(lens, lp, max_bounces=4, device=True)
    torch.cuda.synchronize()
    same_bytes(dev.cpu().numpy().view(rt3.AOV).reshape(16, 32), renderer.render_lens_aov_specular(lens, lp, max_bounces=4), "lens device form")
    # the three shards are the rows of the whole frame
    for i in range(3):
        sp = rt3.make_params(**dict(params, tile_rows=4, tile_index=i, tile_count=3))
        shard = renderer.render_aov_specular(cam, sp, max_bounces=4, max_fuzz=0.0)
        rows = [rt3.lib().rt3_row_of_local(C.byref(sp), k) for k in range(len(shard))]
        assert len(rows) > 0
        same_bytes(shard, whole[rows], "shard %d" % i)
    # a progressive render continues across the call
    straight = renderer.render_path_range(cam, p, 0, 2)
    straight = renderer.render_path_range(cam, p, 2, 2)
    renderer.render_path_range(cam, p, 0, 2)
    renderer.render_aov_specular(cam, p, max_bounces=4, max_fuzz=0.0)
    same_bytes(renderer.render_path_range(cam, p, 2, 2), straight, "accumulation")


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals_name_their_argument_and_change_nothing(rt3, renderer):
    scene, cam, params = weekend(rt3)
    upload(rt3, renderer, scene)
    L, ctx = rt3.lib(), renderer._ctx
    p = rt3.make_params(**dict(params, spp=1))
    before = renderer.render_aov_specular(cam, p, max_bounces=3, max_fuzz=0.0)
    out = np.zeros((54, 96), rt3.AOV)
    lens = rt3.make_lens("equirect", (3.0, 1.0, 2.5), (0.0, 1.0, 0.0))
    lp = rt3.make_params(32, 16, spp=1)
    lens_before = renderer.render_lens_aov_specular(lens, lp, max_bounces=3)
    P = rt3.rt3_aov_chain_params
    bad = [(P(17, 0.0, 0, 0), "max_bounces"), (P(1, float("nan"), 0, 0), "max_fuzz"), (P(1, -1.0, 0, 0), "max_fuzz"),
           (P(1, float("inf"), 0, 0), "max_fuzz"), (P(1, 0.0, 1, 0), "flags"), (P(1, 0.0, 0, 1), "_pad"), (None, "chain")]
    ptr = out.ctypes.data_as(C.c_void_p)
    for chain, word in bad:
        ref = C.byref(chain) if chain is not None else None
        calls = [lambda: L.rt3_render_aov_specular(ctx, C.byref(cam), C.byref(p), ref, ptr),
                 lambda: L.rt3_render_aov_specular_device(ctx, C.byref(cam), C.byref(p), ref, ptr, None),
                 lambda: L.rt3_render_lens_aov_specular(ctx, C.byref(lens), C.byref(lp), ref, ptr),
                 lambda: L.rt3_render_lens_aov_specular_device(ctx, C.byref(lens), C.byref(lp), ref, ptr, None)]
        for call in calls:
            assert call() == E_ARG, word
            assert word in L.rt3_last_error(ctx).decode(), (word, L.rt3_last_error(ctx).decode())
        same_bytes(renderer.render_aov_specular(cam, p, max_bounces=3, max_fuzz=0.0), before, word)
    same_bytes(renderer.render_lens_aov_specular(lens, lp, max_bounces=3), lens_before)
    # the twins' own refusal
    ref_p = rt3.make_params(**dict(params, spp=1, flags=rt3.FLAG_REFERENCE_PRIMARY))
    chain = P(3, 0.0, 0, 0)
    assert L.rt3_render_aov_specular(ctx, C.byref(cam), C.byref(ref_p), C.byref(chain), ptr) == E_ARG
    assert "RT3_FLAG_REFERENCE_PRIMARY" in L.rt3_last_error(ctx).decode()
    same_bytes(renderer.render_aov_specular(cam, p, max_bounces=3, max_fuzz=0.0), before)


def test_without_a_scene_it_is_a_state_error(rt3):
    r = rt3.initialize_renderer(0)
    try:
        cam = rt3.weekend_camera(96, 54)
        p = rt3.make_params(96, 54, spp=1)
        out = np.zeros((54, 96), rt3.AOV)
        chain = rt3.rt3_aov_chain_params(2, 0.0, 0, 0)
        assert rt3.lib().rt3_render_aov_specular(r._ctx, C.byref(cam.c), C.byref(p), C.byref(chain), out.ctypes.data_as(C.c_void_p)) == E_STATE
        lens = rt3.make_lens("equirect", (3.0, 1.0, 2.5), (0.0, 1.0, 0.0))
        lp = rt3.make_params(32, 16, spp=1)
        assert rt3.lib().rt3_render_lens_aov_specular(r._ctx, C.byref(lens), C.byref(lp), C.byref(chain), out.ctypes.data_as(C.c_void_p)) == E_STATE
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 6: the command line
def test_cli_writes_the_chain_guides_and_denoises_with_them(rt3, renderer, tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-3_amd", "rt3")
    w, h = 32, 18
    common = ["-f", "ppm", "-W", str(w), "-H", str(h), "--scene", "weekend", "--spp", "4", "--depth", "6", "--seed", "9"]
    p = subprocess.run([exe, *common, "--aov-specular", "4,1", "--aov", str(tmp_path / "S"), "--denoise", str(tmp_path / "S.den.pfm"),
                        str(tmp_path / "s.ppm")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    q = subprocess.run([exe, *common, "--aov", str(tmp_path / "F"), "--denoise", str(tmp_path / "F.den.pfm"), str(tmp_path / "f.ppm")],
                       capture_output=True, text=True)
    assert q.returncode == 0, q.stderr
    sph, sm = rt3.scene_weekend(42)                                   # the command line's weekend scene: its camera and thin lens
    upload(rt3, renderer, dict(spheres=sph, smats=sm))
    cam = rt3.weekend_camera(w, h)
    params = rt3.make_params(w, h, spp=4, max_depth=6, seed=9, flags=rt3.FLAG_GAMMA2, lens_radius=0.05, t_min=0.001)
    renderer.render_path(cam.c, params)
    lin = renderer.accum_resolve(params)
    first, chain = renderer.render_aov(cam.c, params), renderer.render_aov_specular(cam.c, params, max_bounces=4, max_fuzz=1.0)
    assert (first["albedo"] != chain["albedo"]).any()                 # the scene has something to follow
    for prefix, aov in (("S", chain), ("F", first)):                  # with the option the chain's guides, without it what it always wrote
        assert (tmp_path / (prefix + ".albedo.pfm")).read_bytes() == rt3.pfm_bytes(aov["albedo"])
        assert (tmp_path / (prefix + ".normal.pfm")).read_bytes() == rt3.pfm_bytes(aov["normal"])
        assert (tmp_path / (prefix + ".depth.pfm")).read_bytes() == rt3.pfm_bytes(aov["depth"])
        assert (tmp_path / (prefix + ".den.pfm")).read_bytes() == rt3.pfm_bytes(renderer.denoise(lin, aov)[..., :3])
    assert (tmp_path / "s.ppm").read_bytes() == (tmp_path / "f.ppm").read_bytes()
