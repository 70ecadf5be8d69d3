"""The host forms of the C ABI (the entry points that take host pointers), across features: a shard that owns no pixel through six of them, the staging
buffer growing and being reused across different host forms on one context, and the order of the argument checks — the return code and rt3_last_error
text of a table of bad calls over the host and device forms, copied from the source.  The tests of the single features (test_gpu_motion, _radiance,
_adaptive, _update) compare a host form with its device form, optional inputs present and absent, on the small scene defined here.

Every comparison is by bit pattern.  The scene is three spheres plus a mesh of two faces; the frames are 8 x 4 at 2 spp and depth 3."""
import ctypes as C

import numpy as np
import pytest

from test_denoise_abi import synthetic

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, SEED = 8, 4, 2, 3, 9
E_ARG, E_STATE = -1, -4
F = np.float32
vp = C.c_void_p


def two_faces(rt3):
    tris = [rt3.create_triangle((1.5, -0.5, -3.0), (0.2, -0.5, -3.0), (0.8, 0.9, -3.5), (1.0, 0.0, 0.0)),
            rt3.create_triangle((-1.6, -0.4, -2.5), (-0.3, -0.6, -2.8), (-0.9, 0.8, -3.0), (0.0, 1.0, 0.0))]
    return rt3.merge_entities([rt3.pre_render_entity(e) for e in tris])


def mixed_scene(rt3, r):
    """Three spheres and two faces on r -> (center_radius, faces, vertices, camera, params)."""
    cr, mats = rt3.scene_three_spheres()
    faces, verts = two_faces(rt3)
    assert len(faces) == 2 and len(cr) == 3
    r.set_mesh(faces, verts, None)
    r.set_spheres(cr, mats)
    cam = rt3.Camera().update(W, H, 1.0, F(W) / F(H) * F(2.0), 2.0)
    return cr, faces, verts, cam, rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=SEED, t_min=0.001)


def dev(a):
    """A host array -> a GPU tensor of its bytes as float32 rows of 16 bytes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(np.float32).reshape(-1, 4).copy()).cuda()


def records(a, h, w):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(h, w, -1).copy()).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()












# ------------------------------------------------------------------------------------------------ 2: a shard that owns nothing
def test_a_shard_that_owns_no_pixel_copies_nothing(rt3, renderer):
    _, _, _, _, _ = mixed_scene(rt3, renderer)
    L, ctx = rt3.lib(), renderer._ctx
    p = rt3.make_params(W, 2, spp=SPP, max_depth=DEPTH, seed=SEED, t_min=0.001, tile_rows=1, tile_index=3, tile_count=4)
    assert rt3.rows_owned(p) == 0
    cam = rt3.Camera().update(W, 2, 1.0, 8.0, 2.0)
    lens = rt3.make_lens("ortho", (0.0, 0.0, 1.0), (0.0, 0.0, -3.0), extent=(3.0, 2.0))
    c, q, l = C.byref(cam.c), C.byref(p), C.byref(lens)
    calls = (("rt3_render_path_range", (c, q, 0, SPP)), ("rt3_camera_rays", (c, q, 0, SPP)), ("rt3_render_aov", (c, q)),
             ("rt3_render_lens", (l, q, 0, SPP)), ("rt3_render_lens_aov", (l, q)), ("rt3_lens_rays", (l, q, 0, SPP)))
    for name, args in calls:
        guard = np.full(64, 0xA5A5A5A5, np.uint32)
        assert getattr(L, name)(ctx, *args, guard.ctypes.data_as(vp)) == 0, (name, L.rt3_last_error(ctx))
        assert (guard == 0xA5A5A5A5).all(), name


# ------------------------------------------------------------------------------------------------ 3: the staging buffer grows and is reused
def test_small_large_small_across_host_forms_equals_fresh_contexts(rt3):
    small, large = (5, 3), (64, 64)
    frames = {s: synthetic(rt3, s[1], s[0], 11 + s[0]) for s in (small, large)}

    def display(r, s):
        return r.display(frames[s][0], auto=True).tobytes()

    def denoise(r, s):
        return r.denoise(frames[s][0], frames[s][1], iterations=2).tobytes()

    def rays(r, s):
        cam = rt3.Camera().update(s[0], s[1], 1.0, 2.0 * s[0] / s[1], 2.0)
        return r.camera_rays(cam.c, rt3.make_params(s[0], s[1], spp=SPP, max_depth=DEPTH, seed=SEED), 0, SPP).tobytes()

    sequence = [(display, small), (rays, large), (display, small), (denoise, small), (display, large), (denoise, small),
                (rays, small), (denoise, large), (rays, small)]
    one = rt3.initialize_renderer(0)
    try:
        got = [fn(one, s) for fn, s in sequence]
    finally:
        one.close()
    for i, (fn, s) in enumerate(sequence):
        fresh = rt3.initialize_renderer(0)
        try:
            assert fn(fresh, s) == got[i], (i, fn.__name__, s)
        finally:
            fresh.close()


# ------------------------------------------------------------------------------------------------ 4: refusals, in the order the source checks
LIGHT_ENV = "RT3_FLAG_LIGHT_SAMPLING cannot be combined with RT3_FLAG_ENV_SAMPLING (one shadow ray per scatter)"
LIGHT_REF = "RT3_FLAG_LIGHT_SAMPLING cannot be combined with RT3_FLAG_REFERENCE_PRIMARY"
NO_SCENE = "no scene: call rt3_set_spheres / rt3_set_mesh first"
RANGE = "sample range outside [0, spp)"


def test_refusals_keep_their_code_text_and_order(rt3, renderer):
    import torch
    cr, faces, verts, cam, p = mixed_scene(rt3, renderer)
    renderer.clear_environment()
    L, ctx = rt3.lib(), renderer._ctx
    empty = rt3.initialize_renderer(0)                                  # a context without a scene and without an accumulation
    n = W * H
    buf = np.zeros(n * 16, F)
    o = buf.ctypes.data_as(vp)
    other = np.zeros(n * 16, F).ctypes.data_as(vp)
    d = torch.zeros(8 * 1024, dtype=torch.float32, device="cuda")    # regions of 4 KiB: no frame's array here is longer than 1.5 KiB
    d_ok, d_other, d_odd = vp(d.data_ptr()), vp(d[1024:].data_ptr()), vp(d[5 * 1024 + 1:].data_ptr())
    c, q = C.byref(cam.c), C.byref(p)

    def flagged(flags, **kw):
        x = rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=SEED, flags=flags, t_min=0.001)
        for k, v in kw.items():
            setattr(x, k, v)
        return C.byref(x)
    light_env, light_ref = rt3.FLAG_LIGHT_SAMPLING | rt3.FLAG_ENV_SAMPLING, rt3.FLAG_LIGHT_SAMPLING | rt3.FLAG_REFERENCE_PRIMARY
    lens = rt3.make_lens("ortho", (0.0, 0.0, 1.0), (0.0, 0.0, -3.0), extent=(3.0, 2.0))
    l = C.byref(lens)
    ap = C.byref(rt3.ADAPTIVE_PARAMS(2, 1, 0.05, 0.01))
    dn = C.byref(rt3.DENOISE_PARAMS(2, 128, 4.0, 1.0))
    tp = C.byref(rt3.TEMPORAL_PARAMS(rt3.DENOISE_PARAMS(2, 128, 4.0, 1.0), 0.2, 0.2, 2.0, 0.9))
    dp = C.byref(rt3.display_params())
    rp = lambda flags=0: C.byref(rt3.RADIANCE_PARAMS(DEPTH, SEED, flags, 0, SPP, F(0.001)))      # noqa: E731
    cr_p, v_p = cr.ctypes.data_as(vp), verts.ctypes.data_as(vp)
    t_min = F(0.001)
    table = [
        # the updates
        (ctx, "rt3_update_spheres", (None, 3), E_ARG, "center_radius is NULL"),
        (ctx, "rt3_update_spheres", (cr_p, 2), E_ARG, "n must equal the context's sphere count"),
        (empty._ctx, "rt3_update_spheres", (cr_p, 3), E_STATE, "no spheres to update: call rt3_set_spheres first"),
        (ctx, "rt3_update_spheres_device", (d_odd, 3, None), E_ARG, "device buffers must be 16-byte aligned"),
        (ctx, "rt3_update_mesh", (None, None, len(verts)), E_ARG, "vertices is NULL"),
        (ctx, "rt3_update_mesh", (None, v_p, len(verts) - 1), E_ARG, "n_vertices must equal the vertex count of the merged entity buffers"),
        (ctx, "rt3_update_mesh_device", (None, d_odd, len(verts), None), E_ARG, "device buffers must be 16-byte aligned"),
        # Mode R and the renders
        (ctx, "rt3_render", (c, W, H, None), E_ARG, "out_pixels is NULL"),
        (ctx, "rt3_render", (c, 1, H, o), E_ARG, "bad frame size"),
        (ctx, "rt3_render", (None, W, H, o), E_ARG, "cam / d_out_pixels is NULL"),
        (ctx, "rt3_render_path_range", (c, q, 0, 1, None), E_ARG, "out_pixels is NULL"),
        (ctx, "rt3_render_path_range", (c, None, 0, 1, o), E_ARG, "params is NULL"),
        (ctx, "rt3_render_path_range", (None, q, 0, 1, o), E_ARG, "cam / d_out_pixels is NULL"),
        (ctx, "rt3_render_path_range", (c, flagged(light_env), 0, 0, o), E_ARG, LIGHT_ENV),
        (ctx, "rt3_render_path_range", (c, flagged(light_ref), 0, 0, o), E_ARG, LIGHT_REF),
        (ctx, "rt3_render_path_range", (c, q, 1, SPP, o), E_ARG, RANGE),
        (empty._ctx, "rt3_render_path_range", (c, q, 0, 0, o), E_ARG, RANGE),
        (empty._ctx, "rt3_render_path_range", (c, q, 0, 1, o), E_STATE, NO_SCENE),
        (ctx, "rt3_render_path_range", (c, flagged(rt3.FLAG_ENV_SAMPLING), 0, 1, o), E_STATE,
         "RT3_FLAG_ENV_SAMPLING needs an environment map: call rt3_set_environment first"),
        (ctx, "rt3_render_path_adaptive", (c, q, ap, None, None), E_ARG, "out_pixels is NULL"),
        (ctx, "rt3_render_path_adaptive", (c, q, None, o, None), E_ARG, "cam / adaptive params / d_out_pixels is NULL"),
        (ctx, "rt3_render_path_adaptive", (c, flagged(light_env), ap, o, None), E_ARG,
         "RT3_FLAG_LIGHT_SAMPLING is not available to the adaptive render (the light sampling forms have no list form)"),
        (ctx, "rt3_render_path_adaptive_device", (c, q, ap, d_odd, None, None), E_ARG, "d_out_pixels must be 16-byte aligned"),
        # queries, camera rays, AOVs, the resolve
        (ctx, "rt3_intersect", (None, 5, t_min, o), E_ARG, "rays / results array is NULL"),
        (ctx, "rt3_intersect", (o, 5, F(-1.0), other), E_ARG, "t_min must be finite and >= 0"),
        (empty._ctx, "rt3_intersect", (o, 5, t_min, other), E_STATE, NO_SCENE),
        (ctx, "rt3_intersect_device", (d_odd, 5, t_min, d_other, None), E_ARG, "rays and hits must be 16-byte aligned"),
        (ctx, "rt3_intersect_device", (None, 5, t_min, d_other, None), E_ARG, "rays / results buffer is NULL"),
        (ctx, "rt3_camera_rays", (c, q, 0, 1, None), E_ARG, "out_rays is NULL"),
        (ctx, "rt3_camera_rays", (c, q, SPP, 1, o), E_ARG, RANGE),
        (ctx, "rt3_camera_rays", (None, q, 0, 1, o), E_ARG, "cam / rays is NULL"),
        (ctx, "rt3_camera_rays_device", (c, q, 0, 1, d_odd, None), E_ARG, "rays must be 16-byte aligned"),
        (ctx, "rt3_render_aov", (c, q, None), E_ARG, "out_aov is NULL"),
        (ctx, "rt3_render_aov", (None, q, o), E_ARG, "cam / d_out_aov is NULL"),
        (empty._ctx, "rt3_render_aov", (c, q, o), E_STATE, NO_SCENE),
        (empty._ctx, "rt3_accum_resolve", (None,), E_ARG, "rgba is NULL"),
        (empty._ctx, "rt3_accum_resolve", (o,), E_STATE, "no accumulation on this context"),
        (empty._ctx, "rt3_accum_resolve_device", (d_odd, None), E_ARG, "d_out_rgba must be 16-byte aligned"),
        # the denoisers and the motion plane
        (ctx, "rt3_denoise", (W, H, o, other, None, o), E_ARG, "p is NULL"),
        (ctx, "rt3_denoise", (W, H, None, other, dn, o), E_ARG, "colour / aov / out is NULL"),
        (ctx, "rt3_denoise_device", (W, H, d_odd, d_other, dn, d_ok, None), E_ARG, "d_colour_rgba, d_aov and d_out_rgba must be 16-byte aligned"),
        (ctx, "rt3_denoise_device", (W, H, d_ok, d_other, dn, d_ok, None), E_ARG, "d_out_rgba overlaps an input"),
        (ctx, "rt3_denoise_temporal_motion", (W, H, c, o, other, c, None, None, tp, o, other), E_ARG,
         "prev_cam and prev_history must both be NULL or both be non-NULL"),
        (ctx, "rt3_denoise_temporal_motion", (W, H, c, o, other, None, None, None, tp, o, other), E_ARG, "an output overlaps an input"),
        (ctx, "rt3_denoise_temporal_motion_device", (W, H, c, d_ok, d_other, None, None, d_odd, tp, vp(d[2048:].data_ptr()), vp(d[3072:].data_ptr()), None),
         E_ARG, "device buffers must be 16-byte aligned"),
        (ctx, "rt3_motion", (W, H, c, o, None, 3, None, 0, other), E_ARG, "a NULL previous array must have a count of 0"),
        (ctx, "rt3_motion", (W, H, c, o, None, 0, None, 0, o), E_ARG, "out_motion overlaps an input"),
        (ctx, "rt3_motion", (W, H, c, o, cr_p, 2, None, 0, other), E_ARG, "n_prev_spheres must equal the context's sphere count"),
        (empty._ctx, "rt3_motion", (W, H, c, o, cr_p, 3, None, 0, other), E_STATE, "previous spheres were given, but the context has no spheres"),
        (ctx, "rt3_motion_device", (W, H, c, d_ok, d_odd, 3, None, 0, d_other, None), E_ARG, "device buffers must be 16-byte aligned"),
        # radiance
        (ctx, "rt3_radiance", (o, None, 5, None, other), E_ARG, "radiance params is NULL"),
        (ctx, "rt3_radiance", (o, None, 5, rp(light_env), other), E_ARG, LIGHT_ENV),
        (ctx, "rt3_radiance", (o, None, 5, rp(rt3.FLAG_GAMMA2), other), E_ARG,
         "rt3_radiance: flags may only hold RT3_FLAG_BLACK_BACKGROUND, RT3_FLAG_ENV_SAMPLING or RT3_FLAG_LIGHT_SAMPLING"),
        (ctx, "rt3_radiance", (None, None, 5, rp(), other), E_ARG, "rays / out_rgba array is NULL"),
        (empty._ctx, "rt3_radiance", (o, None, 5, rp(), other), E_STATE, NO_SCENE),
        (ctx, "rt3_radiance_device", (None, None, 5, rp(), d_other, None), E_ARG, "rays / out_rgba buffer is NULL"),
        (ctx, "rt3_radiance_device", (d_ok, None, 5, rp(), d_odd, None), E_ARG, "rays and out_rgba must be 16-byte and keys 4-byte aligned"),
        (ctx, "rt3_radiance_device", (d_ok, None, 5, rp(), d_ok, None), E_ARG, "out_rgba overlaps the rays or the keys"),
        (empty._ctx, "rt3_radiance_device", (d_ok, None, 5, rp(), d_other, None), E_STATE, NO_SCENE),
        # the lens forms
        (ctx, "rt3_lens_rays", (None, q, 0, 1, o), E_ARG, "lens / out_rays is NULL"),
        (ctx, "rt3_lens_rays", (l, q, SPP, 1, o), E_ARG, RANGE),
        (ctx, "rt3_lens_rays_device", (l, q, 0, 1, d_odd, None), E_ARG, "rays must be 16-byte aligned"),
        (ctx, "rt3_render_lens", (l, flagged(light_env), 0, 0, o), E_ARG, LIGHT_ENV),
        (ctx, "rt3_render_lens", (l, flagged(light_ref), 0, 0, o), E_ARG, LIGHT_REF),
        (ctx, "rt3_render_lens", (l, flagged(rt3.FLAG_VARIANCE), 0, 0, o), E_ARG,
         "rt3_render_lens: RT3_FLAG_REFERENCE_PRIMARY and RT3_FLAG_VARIANCE do not apply to a lens frame"),
        (ctx, "rt3_render_lens", (l, q, 0, 0, o), E_ARG, RANGE),
        (empty._ctx, "rt3_render_lens", (l, q, 0, 1, o), E_STATE, NO_SCENE),
        (ctx, "rt3_render_lens_device", (l, q, 0, 1, d_odd, None), E_ARG, "d_out_rgba must be 16-byte aligned"),
        (ctx, "rt3_render_lens_aov", (l, flagged(0, lens_radius=0.05), o), E_ARG,
         "rt3_render_lens_aov: lens_radius must be 0 (no depth of field for the lens models)"),
        (ctx, "rt3_render_lens_aov", (l, q, None), E_ARG, "lens / out_aov is NULL"),
        (empty._ctx, "rt3_render_lens_aov", (l, q, o), E_STATE, NO_SCENE),
        # the display transform
        (ctx, "rt3_display", (W, H, o, None, other), E_ARG, "p is NULL"),
        (ctx, "rt3_display", (W, H, None, dp, other), E_ARG, "rgba / out_pixels is NULL"),
        (ctx, "rt3_display", (W, H, o, dp, o), E_ARG, "out_pixels overlaps rgba"),
        (ctx, "rt3_display_device", (W, H, d_odd, dp, d_other, None), E_ARG, "d_rgba must be 16-byte and d_out_pixels 4-byte aligned"),
    ]
    try:
        want = renderer.render_path(cam.c, p).tobytes()
        for i, (x, name, args, code, text) in enumerate(table):
            rc = getattr(L, name)(x, *args)
            assert rc == code and L.rt3_last_error(x).decode() == text, (i, name, rc, L.rt3_last_error(x))
        assert renderer.render_path(cam.c, p).tobytes() == want         # the refused calls left the scene and the context usable
    finally:
        empty.close()
