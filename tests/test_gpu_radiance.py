"""Radiance along caller-supplied rays (rt3_radiance*) on the GPU.

Every comparison is by bit pattern.  rt3_camera_rays exports the exact primary ray of every (pixel, sample), so a radiance query over those rays
with the pixel index as key must reproduce the CPU oracle's per-sample radiance and the render's accumulation; every kernel form must equal the
unfiltered one on rays no camera makes; depth 1 follows from first principles; sample ranges, batching, keys, invalid rays, context state and
the command line."""
import ctypes as C
import os

import numpy as np
import pytest

from test_cli import run
from test_gpu_brute import random_soup
from test_gpu_ray_query import FORMS, soup_rays

pytestmark = pytest.mark.gpu

W, H = 37, 29                                                         # 1073 rays: no multiple of 64 or of the 256-item work chunk
SPP, DEPTH, SEED = 4, 6, 11
E_ARG, E_STATE = -1, -4


# ------------------------------------------------------------------------------------------------ helpers
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what=""):
    """(n, 4) radiance arrays equal by bit pattern (any NaN equals any NaN: an invalid ray's rgb is some NaN)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), "%s: %d of %d values differ, first rows %s: %s vs %s" % (
        what, int(bad.sum()), bad.size, np.nonzero(bad.any(axis=-1))[0][:3], a[bad.any(axis=-1)][:3], b[bad.any(axis=-1)][:3])


def set_scene(rt3, r, spheres=None, smats=None, faces=None, verts=None, fmats=None):
    if faces is not None and len(faces):
        r.set_mesh(faces, verts, fmats)
    else:
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    if spheres is not None and len(spheres):
        r.set_spheres(spheres, smats)
    else:
        r.set_spheres(np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))


def scene(rt3, name):
    """(kwargs of set_scene, an off-axis look-at camera, lens radius, what tells the kernel that ran) of the oracle scenes."""
    if name == "three":
        sph, sm = rt3.scene_three_spheres()
        return dict(spheres=sph, smats=sm), rt3.Camera().look_at(W, H, (-1.5, 1.0, 1.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 2.5), 0.05, "mfma32"
    if name == "weekend":
        sph, sm = rt3.scene_weekend(42)
        return dict(spheres=sph, smats=sm), rt3.Camera().look_at(W, H, (13.0, 2.0, 3.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 20.0, 10.0), 0.1, "mfma32"
    if name == "stress3000":
        sph, sm = rt3.scene_stress(3000, 43)
        return dict(spheres=sph, smats=sm), rt3.Camera().look_at(W, H, (3.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 20.0), 0.2, "rows"
    faces, verts, fm = rt3.scene_cornell(4)
    cam = rt3.Camera().look_at(W, H, (0.3, 0.2, 0.5), (0.0, -0.1, -3.0), (0.0, 1.0, 0.0), 50.0, 3.5)
    if name == "cornell4":
        return dict(faces=faces, verts=verts, fmats=fm), cam, 0.03, "rows"
    assert name == "cornell4+spheres"
    rng = np.random.default_rng(40)
    cr = np.zeros((40, 4), np.float32)
    cr[:, :3] = rng.uniform([-0.8, -0.8, -3.8], [0.8, 0.8, -2.2], (40, 3))
    cr[:, 3] = rng.uniform(0.05, 0.25, 40)
    sm = np.zeros(40, rt3.MATERIAL)
    sm["kind"] = np.arange(40) % 4                                    # flat, Lambert, metal, dielectric
    sm["rgb"] = rng.uniform(0.2, 1.0, (40, 3))
    sm["param"] = np.where(sm["kind"] == 3, 1.5, rng.uniform(0.0, 0.5, 40)).astype(np.float32)
    return dict(spheres=cr, smats=sm, faces=faces, verts=verts, fmats=fm), cam, 0.03, "rows"


def params_of(mod, flags, lens, **tiles):
    return mod.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=SEED, flags=flags, lens_radius=lens, t_min=0.001, **tiles)


_SINGLE = {}                                                          # (scene, flags) -> the four single-sample radiance arrays, computed once


def single_samples(rt3, r, name, flags):
    """Uploads the scene and returns, for each sample s, radiance(camera_rays(cam, P, s, 1), sample_begin = s, samples = 1): [SPP] of (W * H, 4).
    The results are computed once per (scene, flags) and shared; nobody writes to them."""
    kw, cam, lens, form = scene(rt3, name)
    set_scene(rt3, r, **kw)
    p = params_of(rt3, flags, lens)
    if (name, flags) not in _SINGLE:
        out = []
        for s in range(SPP):
            rays = r.camera_rays(cam.c, p, s, 1)
            assert len(rays) == W * H and np.isinf(rays["t_max"]).all()
            got = r.radiance(rays, sample_begin=s, samples=1, max_depth=DEPTH, seed=SEED, flags=flags & rt3.FLAG_BLACK_BACKGROUND, t_min=0.001)
            st = r.stats()
            assert st.samples == W * H and st.ray_casts > W * H and st.launches == 1 and st.mfma_instructions > 0       # some path went on
            if form == "mfma32":                                      # k_trace_mfma32's rays form: no strip lists, every cast takes the matrix filter
                assert st.filter_tests == st.ray_casts * len(kw["spheres"]) and st.bound_tests == 0
            else:                                                     # the multi-level forms count their bound tests
                assert st.bound_tests > 0 and st.filter_tests > 0
            got.setflags(write=False)
            out.append(got)
        _SINGLE[(name, flags)] = out
    return kw, cam, p, _SINGLE[(name, flags)]


# (flags 3: RT3_FLAG_BLACK_BACKGROUND, on the scenes that have emitters — the box's light, the flat spheres)
ORACLE_CASES = [("three", 1), ("weekend", 1), ("stress3000", 1), ("cornell4", 3), ("cornell4+spheres", 1), ("cornell4+spheres", 3)]


# ------------------------------------------------------------------------------------------------ 1: against the oracle
@pytest.mark.parametrize("name,flags", ORACLE_CASES)
def test_single_samples_equal_the_oracle(rt3, renderer, oracle, name, flags):
    kw, cam, p, got = single_samples(rt3, renderer, name, flags)
    okw = dict(kw)
    for k in ("smats", "fmats"):
        if k in okw:
            okw[k] = okw[k].view(oracle.MATERIAL)
    op = params_of(oracle, flags, p.lens_radius)
    ocam = oracle.copy_camera(cam.c)
    lit = 0
    for s in range(SPP):
        acc = np.zeros((H, W, 4), np.float32)
        _, acc, _, casts = oracle.render_path_range(ocam, op, s, 1, acc=acc, threads=16, **okw)      # 0 + L(pixel, s)
        want = acc.reshape(-1, 4)
        assert (bits(want[:, 3]) == 0).all()
        same(got[s], want, "%s sample %d vs the oracle" % (name, s))
        lit += int((want[:, :3] != 0).any(axis=1).sum())
    assert lit >= 16                                                  # not vacuous: lit samples rule out a comparison of zeros with zeros


# ------------------------------------------------------------------------------------------------ 2: against the render
@pytest.mark.parametrize("name,flags", ORACLE_CASES)
def test_summed_samples_equal_the_render(rt3, renderer, name, flags):
    kw, cam, p, got = single_samples(rt3, renderer, name, flags)
    total = np.zeros((W * H, 3), np.float32)
    for s in range(SPP):
        total = total + got[s][:, :3]                                 # f32, in sample order, from +0
    want = np.concatenate([total / np.float32(SPP), np.zeros((W * H, 1), np.float32)], axis=1)
    renderer.render_path(cam.c, p)
    same(renderer.accum_resolve(p).reshape(-1, 4), want, "%s: render vs summed single samples" % name)


def test_a_shard_with_frame_pixel_keys_equals_its_render(rt3, renderer):
    kw, cam, lens, _ = scene(rt3, "weekend")
    set_scene(rt3, renderer, **kw)
    p = params_of(rt3, 1, lens, tile_rows=4, tile_index=1, tile_count=2)
    rows = rt3.rows_owned(p)
    assert 0 < rows < H
    keys = np.concatenate([rt3.row_of_local(p, lr) * W + np.arange(W) for lr in range(rows)]).astype(np.uint32)
    total = np.zeros((rows * W, 3), np.float32)
    for s in range(SPP):
        rays = renderer.camera_rays(cam.c, p, s, 1)                   # the shard's records, compact rows
        assert len(rays) == rows * W
        total = total + renderer.radiance(rays, keys=keys, sample_begin=s, samples=1, max_depth=DEPTH, seed=SEED, t_min=0.001)[:, :3]
    renderer.render_path(cam.c, p)
    want = np.concatenate([total / np.float32(SPP), np.zeros((rows * W, 1), np.float32)], axis=1)
    same(renderer.accum_resolve(p).reshape(-1, 4), want, "shard")


# ------------------------------------------------------------------------------------------------ 3: every form equals the unfiltered form
def soup(rt3, r, rng, n_faces, n_sph, n_rays):
    faces, verts, fm, cr, sm = random_soup(rng, n_faces, n_sph, 1.0, rt3)
    assert set(np.concatenate([fm["kind"], sm["kind"]])) == {0, 1, 2, 3}
    set_scene(rt3, r, cr if n_sph else None, sm, faces if n_faces else None, verts, fm)
    src = cr if n_sph else np.concatenate([verts[::3, :3], np.full((len(verts) // 3, 1), 0.1, np.float32)], axis=1)
    rays = soup_rays(rt3, rng, n_rays, src, 1.0)                      # origins inside, outside, far from and on the surfaces; aimed and random directions
    rays["t_max"] = np.inf
    return rays, (faces, verts, fm, cr, sm)


def with_form(r, env, monkeypatch, fn):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return fn()
    finally:
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("n_faces,n_sph", [(0, 480), (900, 0), (1301, 707)])
def test_every_kernel_form_equals_the_unfiltered_form(rt3, renderer, n_faces, n_sph, monkeypatch):
    rng = np.random.default_rng(61 + n_faces + n_sph)
    rays, _ = soup(rt3, renderer, rng, n_faces, n_sph, 2048)
    call = lambda: renderer.radiance(rays, samples=3, max_depth=DEPTH, seed=5)      # noqa: E731
    renderer.force_brute(True)
    try:
        ref = call()
        st = renderer.stats()
        assert st.mfma_instructions == 0 and st.ray_casts > 3 * 2048 and st.samples == 3 * 2048      # the unfiltered kernel; some paths went on
    finally:
        renderer.force_brute(False)
    assert not np.isnan(ref).any() and (ref[:, :3] != 0).any(axis=1).mean() > 0.2
    forms = dict(FORMS)
    if n_sph and not n_faces:
        forms.update({"tiled_" + k: dict(v, RT3_FORCE_TILED="1") for k, v in FORMS.items()})     # default = k_trace_mfma32 (<= 512 spheres)
    for name, env in forms.items():
        same(with_form(renderer, env, monkeypatch, call), ref, name)
        assert renderer.stats().mfma_instructions > 0 and renderer.stats().ray_casts == st.ray_casts, name
    for env in ({"RT3_NO_MFMA": "1"}, {"RT3_NO_GROUPS": "1"}, {"RT3_MFMA_K64": "1"}):              # switches of forms this call has none of: ignored
        same(with_form(renderer, env, monkeypatch, call), ref, str(env))
        assert renderer.stats().mfma_instructions > 0


# ------------------------------------------------------------------------------------------------ 4: depth 1 from first principles
@pytest.mark.parametrize("flags", [0, 2])
def test_depth_one_is_the_first_hit_material_or_the_sky(rt3, renderer, oracle, flags):
    rng = np.random.default_rng(71)
    rays, (faces, verts, fm, cr, sm) = soup(rt3, renderer, rng, 500, 400, 2048)
    got = renderer.radiance(rays, samples=1, max_depth=1, seed=3, flags=flags)
    hits = renderer.intersect(rays, 0.001)
    want = np.zeros((len(rays), 4), np.float32)
    for kind, mats in ((1, fm), (2, sm)):
        m = (hits["kind"] == kind)
        flat = m.copy()
        flat[m] = mats["kind"][hits["index"][m]] == 0
        want[flat, :3] = mats["rgb"][hits["index"][flat]]             # a hit on a FLAT primitive gives its rgb; any other hit gives 0
    miss = np.nonzero(hits["kind"] == 0)[0]
    if not flags:
        for i in miss:
            want[i, :3] = oracle.sky(rays["direction"][i])
    assert len(miss) > 100 and (hits["kind"] == 1).sum() > 100 and (hits["kind"] == 2).sum() > 100 and (hits["kind"] == 3).sum() == 0
    same(got, want, "depth 1")
    assert renderer.stats().ray_casts == len(rays)


# ------------------------------------------------------------------------------------------------ 5: sample ranges and batching
def test_sample_ranges_and_batching(rt3, renderer):
    rng = np.random.default_rng(81)
    n = 45056                                                         # 12 B x n > half a MiB: the smallest cap holds one sample per batch
    rays, _ = soup(rt3, renderer, rng, 500, 400, n)
    whole = renderer.radiance(rays, samples=5, sample_begin=3, max_depth=DEPTH, seed=7)
    st = renderer.stats()
    assert st.launches == 1 and st.samples == 5 * n
    total = np.zeros((n, 3), np.float32)
    casts = 0
    for s in range(3, 8):
        total = total + renderer.radiance(rays, samples=1, sample_begin=s, max_depth=DEPTH, seed=7)[:, :3]
        casts += renderer.stats().ray_casts
    same(whole, np.concatenate([total / np.float32(5.0), np.zeros((n, 1), np.float32)], axis=1), "5 samples vs five calls")
    assert casts == st.ray_casts
    renderer.set_sample_storage_cap(1 << 20)
    try:
        same(renderer.radiance(rays, samples=5, sample_begin=3, max_depth=DEPTH, seed=7), whole, "one sample per batch")
        sb = renderer.stats()
        assert sb.launches == 5 and sb.samples == 5 * n and sb.ray_casts == st.ray_casts and sb.trace_ms > 0
    finally:
        renderer.set_sample_storage_cap(16 << 30)                     # the context's default


def test_sample_begin_continues_where_the_render_does(rt3, renderer):
    kw, cam, p, got = single_samples(rt3, renderer, "three", 1)
    renderer.render_path_range(cam.c, p, 0, 2)
    acc, _, done = renderer.accum_download(p)
    assert done == 2
    renderer.render_path_range(cam.c, p, 2, 2)
    acc4, _, done = renderer.accum_download(p)
    assert done == 4
    want = (acc.reshape(-1, 4)[:, :3] + got[2][:, :3]) + got[3][:, :3]
    assert np.array_equal(bits(acc4.reshape(-1, 4)[:, :3]), bits(want))


# ------------------------------------------------------------------------------------------------ 6: keys
@pytest.mark.parametrize("n_faces,n_sph", [(0, 480), (500, 400)])
def test_keys_make_the_result_independent_of_order_and_splitting(rt3, renderer, n_faces, n_sph):
    rng = np.random.default_rng(91 + n_sph)
    n = 5000                                                          # more than the 4096 items of a 1024-thread workgroup's first chunks
    rays, _ = soup(rt3, renderer, rng, n_faces, n_sph, n)
    kw = dict(samples=2, max_depth=DEPTH, seed=13)
    whole = renderer.radiance(rays, **kw)
    same(renderer.radiance(rays, keys=np.arange(n, dtype=np.uint32), **kw), whole, "keys = index")
    perm = rng.permutation(n).astype(np.uint32)
    same(renderer.radiance(rays[perm], keys=perm, **kw), whole[perm], "permuted")
    h = 2333
    halves = np.concatenate([renderer.radiance(rays[:h], keys=np.arange(h, dtype=np.uint32), **kw),
                             renderer.radiance(rays[h:], keys=np.arange(h, n, dtype=np.uint32), **kw)])
    same(halves, whole, "split in two")
    other = renderer.radiance(rays, keys=np.arange(n, dtype=np.uint32) + 1, **kw)
    assert (bits(other) != bits(whole)).any()                         # the key does reach the RNG


# ------------------------------------------------------------------------------------------------ 7: invalid rays
@pytest.mark.parametrize("n_bad", [1, 63, 65, 257])
def test_invalid_rays_are_nan_and_disturb_nothing(rt3, renderer, n_bad):
    rng = np.random.default_rng(101)
    rays, _ = soup(rt3, renderer, rng, 500, 400, 2048 + n_bad)
    pos = np.sort(rng.choice(len(rays), n_bad, replace=False))
    bad = rays.copy()
    for k, i in enumerate(pos):
        kind = k % 5
        if kind == 0:
            bad["origin"][i, 1] = np.nan
        elif kind == 1:
            bad["direction"][i] = 0.0
        elif kind == 2:
            bad["direction"][i] *= np.float32(1.01)
        elif kind == 3:
            bad["t_max"][i] = 1e6                                     # a finite t_max is reserved
        else:
            bad["t_max"][i] = np.nan
    keep = np.setdiff1d(np.arange(len(rays)), pos)
    kw = dict(samples=3, max_depth=DEPTH, seed=17)
    clean = renderer.radiance(bad[keep], keys=keep.astype(np.uint32), **kw)
    casts = renderer.stats().ray_casts
    assert not np.isnan(clean).any()
    got = renderer.radiance(bad, **kw)
    st = renderer.stats()
    assert np.isnan(got[pos, :3]).all() and (bits(got[:, 3]) == 0).all()
    same(got[keep], clean, "the valid rays beside %d invalid ones" % n_bad)
    assert st.ray_casts == casts and st.samples == 3 * len(bad)
    only = renderer.radiance(bad[pos], **kw)                          # a batch of nothing but invalid rays
    assert np.isnan(only[:, :3]).all() and (bits(only[:, 3]) == 0).all() and renderer.stats().ray_casts == 0


# ------------------------------------------------------------------------------------------------ 8: context state
def test_radiance_between_progressive_calls_leaves_the_accumulation(rt3, renderer):
    rng = np.random.default_rng(111)
    rays, _ = soup(rt3, renderer, rng, 300, 200, 3000)
    cam = rt3.Camera().update(64, 48, 1.0, 3.0, 2.0)
    p = rt3.make_params(64, 48, spp=4, max_depth=6, seed=9, flags=1)
    whole = renderer.render_path(cam.c, p)
    renderer.render_path_range(cam.c, p, 0, 2)
    renderer.radiance(rays, samples=3, max_depth=DEPTH)
    assert np.array_equal(renderer.render_path_range(cam.c, p, 2, 2), whole)


def test_argument_errors_leave_the_context_usable(rt3, renderer):
    import torch
    L = rt3.lib()
    rng = np.random.default_rng(121)
    rays, _ = soup(rt3, renderer, rng, 300, 200, 1000)
    n = len(rays)
    good = renderer.radiance(rays, samples=2, max_depth=DEPTH)
    out = np.zeros((n, 4), np.float32)
    ctx, vp = renderer._ctx, C.c_void_p

    def host(rp, count=n):
        return L.rt3_radiance(ctx, rays.ctypes.data_as(vp), None, count, C.byref(rp), out.ctypes.data_as(vp))
    RP = rt3.RADIANCE_PARAMS
    assert host(RP(6, 1, 1, 0, 2, 0.001)) == E_ARG                    # a bad flag (GAMMA2 means nothing here)
    assert host(RP(6, 1, 4, 0, 2, 0.001)) == E_ARG
    assert host(RP(0, 1, 0, 0, 2, 0.001)) == E_ARG                    # max_depth 0
    assert host(RP(6, 1, 0, 0, 0, 0.001)) == E_ARG                    # sample_count 0
    assert host(RP(6, 1, 0, 1 << 31, 1, 0.001)) == E_ARG              # sample_begin + sample_count > 2^31
    assert host(RP(6, 1, 0, (1 << 31) - 1, 1, 0.001)) == 0
    for t_min in (-1.0, np.inf, np.nan):
        assert host(RP(6, 1, 0, 0, 2, t_min)) == E_ARG
    assert host(RP(6, 1, 0, 0, 2, 0.001), (1 << 27) + 1) == E_ARG     # n > 2^27 (refused before anything is read)
    assert L.rt3_radiance(ctx, None, None, 0, C.byref(RP(6, 1, 0, 0, 2, 0.001)), None) == 0          # n == 0: nothing to do
    assert L.rt3_radiance(ctx, rays.ctypes.data_as(vp), None, n, None, out.ctypes.data_as(vp)) == E_ARG
    assert L.rt3_radiance(ctx, None, None, n, C.byref(RP(6, 1, 0, 0, 2, 0.001)), out.ctypes.data_as(vp)) == E_ARG
    # the device form: misaligned pointers, an output that overlaps an input
    rp = RP(6, 1, 0, 0, 2, 0.001)
    buf = torch.zeros(8 * n + 8, dtype=torch.float32, device="cuda")
    dev = buf[:8 * n]
    dev.copy_(torch.from_numpy(rays.view(np.float32).reshape(-1).copy()))
    res = torch.zeros(4 * n + 8, dtype=torch.float32, device="cuda")
    keys = torch.arange(n + 8, dtype=torch.int32, device="cuda")
    keys8 = keys.view(torch.int8)

    def device(d_rays, d_keys, d_out):
        return L.rt3_radiance_device(ctx, vp(d_rays), vp(d_keys), n, C.byref(rp), vp(d_out), None)
    assert device(buf[1:].data_ptr(), None, res.data_ptr()) == E_ARG                               # rays 4 bytes off
    assert device(dev.data_ptr(), None, res[1:].data_ptr()) == E_ARG                                # output 4 bytes off
    assert device(dev.data_ptr(), keys8[2:].data_ptr(), res.data_ptr()) == E_ARG                    # keys 2 bytes off
    assert device(dev.data_ptr(), None, dev.data_ptr()) == E_ARG                                    # output on the rays
    assert device(dev.data_ptr(), None, buf[8 * n - 4:].data_ptr()) == E_ARG                        # ... on their last 16 bytes
    assert device(dev.data_ptr(), res.view(torch.int32)[4:].data_ptr(), res.data_ptr()) == E_ARG    # ... on the keys
    assert device(dev.data_ptr(), None, None) == E_ARG
    assert device(dev.data_ptr(), keys[1:].data_ptr(), res.data_ptr()) == 0                         # keys need 4-byte alignment only
    torch.cuda.synchronize()
    same(renderer.radiance(rays, samples=2, max_depth=DEPTH), good, "after the refused calls")
    set_scene(rt3, renderer)                                          # no scene
    assert host(RP(6, 1, 0, 0, 2, 0.001)) == E_STATE
    assert device(dev.data_ptr(), None, res.data_ptr()) == E_STATE
    assert L.rt3_radiance(ctx, None, None, 0, C.byref(RP(6, 1, 0, 0, 2, 0.001)), None) == 0
    rays2, _ = soup(rt3, renderer, np.random.default_rng(121), 300, 200, 1000)
    same(renderer.radiance(rays2, samples=2, max_depth=DEPTH), good, "after no scene")


def test_torch_tensor_in_tensor_out_on_a_side_stream(rt3, renderer):
    import torch
    rng = np.random.default_rng(131)
    rays, _ = soup(rt3, renderer, rng, 400, 300, 5000)
    keys = rng.integers(0, 1 << 31, len(rays)).astype(np.uint32)
    kw = dict(samples=3, sample_begin=1, max_depth=DEPTH, seed=19, flags=2)
    want, want_keyed = renderer.radiance(rays, **kw), renderer.radiance(rays, keys=keys, **kw)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda")
        dkeys = torch.from_numpy(keys.view(np.int32).copy()).to("cuda")
        got = renderer.radiance(dev, **kw)
        got_keyed = renderer.radiance(dev, keys=dkeys, **kw)
        twice = got * 2.0                                             # consumed on the same stream
    s.synchronize()
    assert got.device == dev.device and got.dtype == torch.float32 and tuple(got.shape) == (len(rays), 4)
    same(got.cpu().numpy(), want, "torch vs numpy")
    same(got_keyed.cpu().numpy(), want_keyed, "torch vs numpy, keys")
    same(twice.cpu().numpy(), want * np.float32(2.0), "consumer on the stream")
    with pytest.raises(rt3.Fatal):
        renderer.radiance(dev, keys=keys)                             # host keys with device rays


# ------------------------------------------------------------------------------------------------ 9: the command line
def test_cli_radiance_equals_the_python_call(rt3, renderer, tmp_path):
    sph, sm = rt3.scene_three_spheres()
    set_scene(rt3, renderer, sph, sm)
    rng = np.random.default_rng(141)
    rays = soup_rays(rt3, rng, 1073, sph, 0.3)
    rays["t_max"] = np.inf
    rays["t_max"][5] = 2.0                                            # one invalid ray: NaN in the file
    (tmp_path / "rays.bin").write_bytes(rays.tobytes())
    rc, out, err = run("-f", "ppm", "-W", "32", "-H", "18", "--scene", "three", "--spp", "4", "--depth", "6", "--seed", "9",
                       "--rays", str(tmp_path / "rays.bin"), "--radiance", str(tmp_path / "rad.pfm"), str(tmp_path / "three.ppm"))
    assert rc == 0, err
    assert os.path.exists(tmp_path / "three.ppm")
    data = (tmp_path / "rad.pfm").read_bytes()
    header = b"PF\n%d 1\n-1.0\n" % len(rays)
    assert data.startswith(header) and len(data) == len(header) + 12 * len(rays)
    got = np.frombuffer(data[len(header):], "<f4").reshape(-1, 3)
    want = renderer.radiance(rays, samples=4, max_depth=6, seed=9, flags=0, t_min=0.001)
    same(got, want[:, :3], "rt3 --rays --radiance")
    assert np.isnan(got[5]).all() and not np.isnan(np.delete(got, 5, axis=0)).any()
    rc, out, err = run("-f", "ppm", "-W", "32", "-H", "18", "--scene", "three", "--spp", "4", "--rays", str(tmp_path / "none.bin"),
                       "--radiance", str(tmp_path / "rad2.pfm"), str(tmp_path / "three.ppm"))
    assert rc == -1 and "Could not open" in err


# ------------------------------------------------------------------------------------------------ host form = device form, optional inputs present and absent
def test_radiance_on_five_rays_with_and_without_keys(rt3, renderer):
    from test_gpu_host_forms import DEPTH, SEED, SPP, dev, host, mixed_scene
    import torch
    _, _, _, cam, p = mixed_scene(rt3, renderer)
    rays = renderer.camera_rays(cam.c, p, 0, 1)[9:14]                  # 5 rays: 20 bytes of keys, no whole number of 16-byte units (the staged segments stay aligned)
    keys = np.array([40, 3, 77, 12, 5], np.uint32)
    t_rays = dev(rays).reshape(5, 8)
    for k in (None, keys):
        out = renderer.radiance(rays, keys=k, samples=SPP, max_depth=DEPTH, seed=SEED)
        t = renderer.radiance(t_rays, keys=None if k is None else torch.from_numpy(k.view(np.int32)).cuda(), samples=SPP, max_depth=DEPTH, seed=SEED)
        assert host(t) == out.tobytes(), k is not None
