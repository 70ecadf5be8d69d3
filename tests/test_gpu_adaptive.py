"""Adaptive sampling (rt3_render_path_adaptive*) through the C ABI against the numpy restatement over the CPU oracle
(tests/adaptive_ref.py, pinned by tests/test_adaptive_ref.py): the count map is the restatement's exactly, every pixel is the oracle's pixel over
its own prefix of the sample law bit for bit, and rt3_accum_resolve divides by the pixel's own count."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
from cases import hip_upload

pytestmark = pytest.mark.gpu


def scene_kw(oracle, case):
    kw = dict(threads=16)
    if case.get("spheres") is not None:
        kw.update(spheres=case["spheres"], smats=np.ascontiguousarray(case["smats"]).view(oracle.MATERIAL))
    if case.get("faces") is not None:
        kw.update(faces=np.ascontiguousarray(case["faces"]).view(oracle.GFACE), verts=case["verts"],
                  fmats=np.ascontiguousarray(case["fmats"]).view(oracle.MATERIAL))
    return kw


def restatement(oracle, case, threshold, min_spp, step_spp, dark=0.01):
    op = oracle.make_params(**dict(case["params"], flags=case["params"]["flags"] | oracle.FLAG_VARIANCE))
    return adaptive_ref.render_adaptive(oracle.copy_camera(case["cam"]), op, threshold, min_spp, step_spp, dark, **scene_kw(oracle, case))


def check_against(ref, pixels, counts, resolved=None):
    """counts == the restatement's; per level n the pixels with count n are the oracle's frame over [0, n); the resolve is o_acc / n."""
    want = ref["counts"]
    print("levels %s, pixels per level %s, active per round %s" % (sorted(ref["levels"]), [int((want == n).sum()) for n in sorted(ref["levels"])],
                                                                 ref["active_counts"]))
    assert counts.dtype == np.uint32 and counts.shape == want.shape
    assert np.array_equal(counts, want), "%d counts differ" % int((counts != want).sum())
    for n, (img, acc, _) in ref["levels"].items():
        at = want == n
        assert np.array_equal(pixels[at], img[at]), "level %d: %d pixels differ from the oracle's [0, %d) frame" % (n, int((pixels[at] != img[at]).sum()), n)
        if resolved is not None:
            o = acc[at][:, :3] / np.float32(n)
            assert resolved[at][:, :3].tobytes() == o.tobytes() and not resolved[at][:, 3].any(), "level %d: accum_resolve != o_acc / n" % n
    assert np.array_equal(pixels, adaptive_ref.expected_frame(ref))


def weekend(rt3, w, h, spp):
    cr, mats = rt3.scene_weekend(42)
    return dict(spheres=cr, smats=mats, cam=rt3.weekend_camera(w, h).c,
                params=dict(width=w, height=h, spp=spp, max_depth=50, seed=1, flags=1, lens_radius=0.05))


@pytest.mark.parametrize("budget", [128, 64])
def test_weekend_counts_pixels_and_resolve_equal_the_restatement(rt3, renderer, oracle, budget):
    """160 x 90, min 16, step 16, threshold 0.05, dark 0.01; budget 128 (no strata) and 64 (a perfect square: strata on)."""
    case = weekend(rt3, 160, 90, budget)
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    ref = restatement(oracle, case, 0.05, 16, 16)
    pixels, counts = renderer.render_adaptive(case["cam"], p, threshold=0.05, min_spp=16, step_spp=16, dark=0.01)
    st = renderer.stats()
    resolved = renderer.accum_resolve(p)
    check_against(ref, pixels, counts, resolved)
    # the case is not a vacuous one: several levels, and neither everything nor nothing leaves after the first round
    assert len(np.unique(counts)) >= 3
    for n in (16, budget):
        share = float((counts == n).mean())
        print("share of pixels at %d samples: %.3f" % (n, share))
        assert 0.05 <= share <= 0.60
    assert st.samples == int(counts.sum(dtype=np.uint64))
    assert st.launches == len(ref["active_counts"]) and st.ray_casts >= st.samples
    # RT3_FLAG_VARIANCE changes nothing
    pv, cv = renderer.render_adaptive(case["cam"], rt3.make_params(**dict(case["params"], flags=1 | rt3.FLAG_VARIANCE)), 0.05, 16, 16, 0.01)
    assert np.array_equal(pv, pixels) and np.array_equal(cv, counts)


def test_min_spp_equal_to_spp_is_render_path(rt3, renderer):
    case = weekend(rt3, 96, 54, 16)
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    want = renderer.render_path(case["cam"], p)
    pixels, counts = renderer.render_adaptive(case["cam"], p, threshold=0.05, min_spp=16, step_spp=16)
    assert np.array_equal(pixels, want) and (counts == 16).all()
    assert renderer.stats().samples == 96 * 54 * 16


def test_triangles_on_a_shard_in_several_batches_per_round(rt3, renderer, oracle):
    """cornell(4), shard 1 of 3 in row blocks of 4 (the 3 x 3 neighbourhood stops at the shard's row-block edges), a ragged last round
    (8 + 4 x 7 = 36) and a sample storage cap that splits every round into batches."""
    faces, verts, fmats = rt3.scene_cornell(4)
    cam = rt3.Camera().update(256, 256, 2.0, 2.0, 2.0)
    case = dict(faces=faces, verts=verts, fmats=fmats, cam=cam.c,
                params=dict(width=256, height=256, spp=36, max_depth=6, seed=3, flags=1 | 2, tile_rows=4, tile_index=1, tile_count=3))
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    ref = restatement(oracle, case, 0.5, 8, 7)
    assert len(np.unique(ref["counts"])) >= 2 and len(ref["active_counts"]) == 5
    renderer.set_sample_storage_cap(1 << 20)                # 1 MiB: 21504 owned pixels x 12 B -> 4 samples per dense batch
    try:
        pixels, counts = renderer.render_adaptive(case["cam"], p, threshold=0.5, min_spp=8, step_spp=7)
        st = renderer.stats()
        resolved = renderer.accum_resolve(p)
    finally:
        renderer.set_sample_storage_cap(16 << 30)
    check_against(ref, pixels, counts, resolved)
    assert st.launches > len(ref["active_counts"]) and st.samples == int(counts.sum(dtype=np.uint64))


def test_more_than_512_spheres_and_every_other_trace_kernel(rt3, renderer, oracle, monkeypatch):
    """3000 spheres take the resident three-level kernel; the same counts and pixels from k_trace_levels (RT3_LEVELS=3), the tiled rows
    (RT3_FORCE_TILED=1 is a no-op here, RT3_NO_RESIDENT=1 streams them), the VALU scan (RT3_NO_MFMA=1) and the unfiltered kernel."""
    cr, mats = rt3.scene_stress(3000, 7)
    cam = rt3.Camera().look_at(96, 54, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)
    case = dict(spheres=cr, smats=mats, cam=cam.c, params=dict(width=96, height=54, spp=32, max_depth=8, seed=2, flags=1))
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    ref = restatement(oracle, case, 0.05, 8, 8)
    pixels, counts = renderer.render_adaptive(case["cam"], p, threshold=0.05, min_spp=8, step_spp=8)
    check_against(ref, pixels, counts, renderer.accum_resolve(p))
    assert len(np.unique(counts)) >= 3
    for name in ("RT3_LEVELS", "RT3_FORCE_TILED", "RT3_NO_RESIDENT", "RT3_NO_MFMA"):
        with monkeypatch.context() as m:
            m.setenv(name, "3" if name == "RT3_LEVELS" else "1")
            px, cn = renderer.render_adaptive(case["cam"], p, threshold=0.05, min_spp=8, step_spp=8)
        assert np.array_equal(cn, counts) and np.array_equal(px, pixels), name
    renderer.force_brute(True)
    try:
        px, cn = renderer.render_adaptive(case["cam"], p, threshold=0.05, min_spp=8, step_spp=8)
    finally:
        renderer.force_brute(False)
    assert np.array_equal(cn, counts) and np.array_equal(px, pixels)


def test_at_most_512_spheres_under_the_other_kernels(rt3, renderer, oracle, monkeypatch):
    """The three-sphere scene takes k_trace_mfma32 (strip lists in round 0 only); RT3_FORCE_TILED=1, RT3_PRIMARY_LISTS=0, RT3_MFMA_K64=1 and
    RT3_NO_MFMA=1 give the same counts and pixels, and the restatement's."""
    cr, mats = rt3.scene_three_spheres()
    cam = rt3.Camera().update(64, 36, 1.0, np.float32(64) / np.float32(36) * np.float32(2.0), 2.0)
    case = dict(spheres=cr, smats=mats, cam=cam.c, params=dict(width=64, height=36, spp=64, max_depth=8, seed=1, flags=1))
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    ref = restatement(oracle, case, 0.05, 8, 8)
    assert ref["active_counts"] == [2304, 1499, 1311, 1000, 802, 668, 539, 466]
    pixels, counts = renderer.render_adaptive(case["cam"], p, threshold=0.05, min_spp=8, step_spp=8)
    check_against(ref, pixels, counts, renderer.accum_resolve(p))
    for name, value in (("RT3_FORCE_TILED", "1"), ("RT3_PRIMARY_LISTS", "0"), ("RT3_MFMA_K64", "1"), ("RT3_NO_MFMA", "1")):
        with monkeypatch.context() as m:
            m.setenv(name, value)
            px, cn = renderer.render_adaptive(case["cam"], p, threshold=0.05, min_spp=8, step_spp=8)
        assert np.array_equal(cn, counts) and np.array_equal(px, pixels), name


def test_device_form_on_a_torch_stream_then_the_denoiser_and_the_state_rules(rt3, renderer, oracle):
    import torch
    case = weekend(rt3, 160, 90, 64)
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    before = renderer.render_path(case["cam"], p)
    ref = restatement(oracle, case, 0.05, 16, 16)
    dev = torch.device("cuda:0")
    d_pixels = torch.zeros((90, 160), dtype=torch.int32, device=dev)
    d_counts = torch.zeros((90, 160), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        renderer.render_adaptive_device(case["cam"], p, d_pixels, d_counts, threshold=0.05, min_spp=16, step_spp=16, dark=0.01)
        colour = torch.zeros((90, 160, 4), dtype=torch.float32, device=dev)
        renderer.accum_resolve_device(colour.data_ptr(), stream.cuda_stream)
        aov = torch.zeros((90, 160, 12), dtype=torch.float32, device=dev)
        renderer.render_aov_device(case["cam"], p, aov.data_ptr(), stream.cuda_stream)
        out = renderer.denoise(colour, aov)
    stream.synchronize()
    pixels = d_pixels.cpu().numpy().view(np.uint32)
    counts = d_counts.cpu().numpy().view(np.uint32)
    check_against(ref, pixels, counts, colour.cpu().numpy())
    out = out.cpu().numpy()
    assert np.isfinite(out).all() and out[..., :3].max() > 0.1 and not out[..., 3].any()
    # counts are optional; raw pointers on the renderer's own stream
    d_again = torch.zeros((90, 160), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    renderer.render_adaptive_device(case["cam"], p, d_again.data_ptr(), None, threshold=0.05, min_spp=16, step_spp=16)
    renderer.synchronize()
    assert np.array_equal(d_again.cpu().numpy().view(np.uint32), pixels)
    # an adaptive accumulation has no checkpoint form and cannot be continued
    with pytest.raises(rt3.Fatal, match="adaptive"):
        renderer.accum_download(p)
    with pytest.raises(rt3.Fatal, match="adaptive"):
        renderer.render_path_range(case["cam"], p, 64 - 16, 16)
    with pytest.raises(rt3.Fatal, match="adaptive"):
        renderer.render_path_range(case["cam"], p, 16, 16)
    assert np.array_equal(renderer.accum_resolve(p), colour.cpu().numpy())       # the refused calls left it alone
    # an ordinary render starts over, as it always did
    assert np.array_equal(renderer.render_path(case["cam"], p), before)
    acc, _, done = renderer.accum_download(p)
    assert done == 64
    renderer.render_path_range(case["cam"], p, 0, 16)
    assert np.array_equal(renderer.render_path_range(case["cam"], p, 16, 48), before)


def test_argument_refusals(rt3, renderer):
    L = rt3.lib()
    case = weekend(rt3, 32, 18, 32)
    hip_upload(renderer, case)
    cam = case["cam"]
    p = rt3.make_params(**case["params"])
    n = 32 * 18
    out = np.zeros(n, np.uint32); cnt = np.zeros(n, np.uint32)
    po, pc = out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)
    good = rt3.ADAPTIVE_PARAMS(16, 16, 0.05, 0.01)
    ctx = renderer._ctx
    host, dev = L.rt3_render_path_adaptive, L.rt3_render_path_adaptive_device
    assert host(ctx, C.byref(cam), C.byref(p), C.byref(good), po, pc) == 0
    assert host(ctx, C.byref(cam), C.byref(p), C.byref(good), po, None) == 0            # counts may be NULL
    E_ARG, E_STATE = -1, -4
    assert host(None, C.byref(cam), C.byref(p), C.byref(good), po, pc) == E_ARG
    assert host(ctx, None, C.byref(p), C.byref(good), po, pc) == E_ARG
    assert host(ctx, C.byref(cam), None, C.byref(good), po, pc) == E_ARG
    assert host(ctx, C.byref(cam), C.byref(p), None, po, pc) == E_ARG
    assert host(ctx, C.byref(cam), C.byref(p), C.byref(good), None, pc) == E_ARG
    inf, nan = float("inf"), float("nan")
    for bad in ((1, 16, 0.05, 0.01), (0, 16, 0.05, 0.01), (33, 16, 0.05, 0.01), (16, 0, 0.05, 0.01), (16, 16, 0.0, 0.01), (16, 16, -0.05, 0.01),
                (16, 16, inf, 0.01), (16, 16, nan, 0.01), (16, 16, 0.05, -0.01), (16, 16, 0.05, inf), (16, 16, 0.05, nan)):
        assert host(ctx, C.byref(cam), C.byref(p), C.byref(rt3.ADAPTIVE_PARAMS(*bad)), po, pc) == E_ARG, bad
        assert b"min_spp" in L.rt3_last_error(ctx) or b"step_spp" in L.rt3_last_error(ctx) or b"threshold" in L.rt3_last_error(ctx) \
            or b"dark" in L.rt3_last_error(ctx), bad
    for ok in ((2, 1, 1e-30, 0.0), (32, 1, 0.05, 0.01), (2, 1000, 5.0, 10.0)):
        assert host(ctx, C.byref(cam), C.byref(p), C.byref(rt3.ADAPTIVE_PARAMS(*ok)), po, pc) == 0, ok
    pref = rt3.make_params(**dict(case["params"], flags=1 | rt3.FLAG_REFERENCE_PRIMARY))
    assert host(ctx, C.byref(cam), C.byref(pref), C.byref(good), po, pc) == E_ARG
    assert b"REFERENCE_PRIMARY" in L.rt3_last_error(ctx)
    # device pointers: 16-byte aligned pixels, 4-byte aligned counts
    d = L.rt3_device_alloc_words(ctx, 2 * n + 8)
    try:
        assert dev(ctx, C.byref(cam), C.byref(p), C.byref(good), C.c_void_p(d), C.c_void_p(d + 4 * n + 4), None) == 0
        assert dev(ctx, C.byref(cam), C.byref(p), C.byref(good), C.c_void_p(d), None, None) == 0
        assert dev(ctx, C.byref(cam), C.byref(p), C.byref(good), C.c_void_p(d + 4), C.c_void_p(d + 4 * n + 16), None) == E_ARG
        assert dev(ctx, C.byref(cam), C.byref(p), C.byref(good), C.c_void_p(d), C.c_void_p(d + 4 * n + 2), None) == E_ARG
        assert dev(ctx, C.byref(cam), C.byref(p), C.byref(good), None, None, None) == E_ARG
        assert L.rt3_synchronize(ctx) == 0
    finally:
        L.rt3_device_free(ctx, C.c_void_p(d))
    # no scene
    other = rt3.initialize_renderer(0)
    try:
        assert host(other._ctx, C.byref(cam), C.byref(p), C.byref(good), po, pc) == E_STATE
    finally:
        other.close()
    # the refusals left the renderer usable
    px, cn = renderer.render_adaptive(cam, p, min_spp=32)
    assert np.array_equal(px, renderer.render_path(cam, p)) and (cn == 32).all()


def test_a_threshold_nothing_reaches_keeps_every_pixel_to_the_budget(rt3, renderer):
    """threshold 1e-30: every pixel with any variance stays active, so a pixel either has the whole budget — and is render_path's pixel — or
    it and its whole neighbourhood show no variance in f32 (few pixels of this scene: every one is jittered over a gradient); stats().samples is the sum of the counts."""
    case = weekend(rt3, 96, 54, 40)
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    want = renderer.render_path(case["cam"], p)
    pixels, counts = renderer.render_adaptive(case["cam"], p, threshold=1e-30, min_spp=8, step_spp=12)
    assert set(np.unique(counts)) <= {8, 20, 32, 40}
    full = counts == 40
    assert full.mean() > 0.5 and np.array_equal(pixels[full], want[full])
    assert renderer.stats().samples == int(counts.sum(dtype=np.uint64))


# ------------------------------------------------------------------------------------------------ host form = device form, optional inputs present and absent
def test_adaptive_render_with_and_without_counts(rt3, renderer):
    from test_gpu_host_forms import H, W, host, mixed_scene, vp
    import torch
    _, _, _, cam, p = mixed_scene(rt3, renderer)
    p.spp = 6
    L, ctx = rt3.lib(), renderer._ctx
    ap = rt3.ADAPTIVE_PARAMS(2, 1, 1e-6, 0.0)
    for with_counts in (False, True):
        out, counts = np.zeros((H, W), np.uint32), np.full((H, W), 0xA5A5A5A5, np.uint32)
        assert L.rt3_render_path_adaptive(ctx, C.byref(cam.c), C.byref(p), C.byref(ap), out.ctypes.data_as(vp),
                                          counts.ctypes.data_as(vp) if with_counts else None) == 0
        d_out = torch.zeros(H * W, dtype=torch.int32, device="cuda")
        d_counts = torch.full((H * W,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        renderer.render_adaptive_device(cam.c, p, d_out, d_counts if with_counts else None, threshold=1e-6, min_spp=2, step_spp=1, dark=0.0)
        assert host(d_out) == out.tobytes()
        if with_counts:
            assert host(d_counts) == counts.tobytes() and counts.min() >= 2 and counts.max() <= 6
        else:
            assert (counts == 0xA5A5A5A5).all() and (d_counts.cpu().numpy() == 0x5A5A5A5A).all()
