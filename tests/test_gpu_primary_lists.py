"""Primary rays traced against per-strip sphere lists when k_trace_mfma32 refills its stock (rt3_primary_lists.hpp,
refill_from_traced_stock in rt3_matrix_filter.hpp).  The frame may not depend on it: every frame here is compared, bit for bit, with the
unfiltered kernel (force_brute) and with the CPU oracle — lists on (default threshold), off (RT3_PRIMARY_LISTS=0), and with
RT3_PRIMARY_LIST_MAX 0 / 1 / 1000 (only restocks with an empty list are traced | lists of at most one sphere | every list, the long ones too).
The lists themselves (rt3_debug_primary_lists) must hold every sphere that a primary ray of their group can pass sphere_root's candidate rule
for: random rays by start_path's law, a third of them at the extremes of jitter and lens, 0 misses."""
import contextlib
import os
import sys

import numpy as np
import pytest

from cases import ROOT, hip_render, hip_upload, oracle_render

sys.path.insert(0, os.path.join(ROOT, "tools"))
import primary_list_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ({}, {"RT3_PRIMARY_LISTS": "0"}, {"RT3_PRIMARY_LIST_MAX": "0"}, {"RT3_PRIMARY_LIST_MAX": "1"}, {"RT3_PRIMARY_LIST_MAX": "1000"})


@contextlib.contextmanager
def env(knobs):
    old = {k: os.environ.get(k) for k in ("RT3_PRIMARY_LISTS", "RT3_PRIMARY_LIST_MAX")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(knobs)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def moved(cr, scale, shift):
    out = np.array(cr, np.float32)
    out[:, :3] = out[:, :3] * np.float32(scale) + np.float32(shift)
    out[:, 3] *= np.float32(scale)
    return out


def book_camera(rt3, w, h, scale=1.0, shift=(0.0, 0.0, 0.0), look_from=(13.0, 2.0, 3.0), vfov=20.0, focus=10.0):
    s, t = np.float64(scale), np.float64(shift)
    return rt3.Camera().look_at(w, h, tuple(np.float64(look_from) * s + t), tuple(t), (0.0, 1.0, 0.0), vfov, focus * scale).c


def make_cases(rt3):
    cases = {}
    cr, mats = rt3.scene_weekend(42)

    def add(name, w, h, spheres=cr, smats=mats, cam=None, **params):
        kw = dict(width=w, height=h, spp=4, max_depth=12, seed=3, flags=1, lens_radius=0.05)
        kw.update(params)
        cases[name] = dict(spheres=spheres, smats=smats, cam=cam if cam is not None else rt3.weekend_camera(w, h).c, params=kw)

    add("weekend_320x180", 320, 180, max_depth=50)
    for w in (17, 63, 65, 100):                                 # groups of 64 pixels that straddle frame rows
        add("weekend_w%d" % w, w, 40)
    for rows in (1, 5):
        for idx in range(3):
            add("weekend_shard%d_rows%d" % (idx, rows), 100, 57, tile_rows=rows, tile_index=idx, tile_count=3)
    add("weekend_spp1", 100, 56, spp=1)
    add("weekend_spp9_stratified", 100, 56, spp=9)
    add("weekend_spp5", 100, 56, spp=5)
    for lens in (0.0, 0.5):
        add("weekend_lens%g" % lens, 100, 56, lens_radius=lens)
    # the camera inside a sphere (glass, then a diffuse one); spheres behind the camera, on the lens, on and beyond the focus plane
    view = np.float32([-13.0, -2.0, -3.0]) / np.linalg.norm(np.float32([13.0, 2.0, 3.0]))
    eye = np.float32([13.0, 2.0, 3.0])
    extra = np.float32([[*eye, 2.5], [*(eye - 1.5 * view), 0.7], [*(eye + np.float32([0.04, 0.0, 0.0])), 0.02], [*(eye + 10.0 * view), 0.8],
                        [*(eye + 25.0 * view + np.float32([0.0, 2.0, 0.0])), 1.5]])
    for kind, name in ((rt3.MAT_DIELECTRIC, "glass"), (rt3.MAT_LAMBERT, "diffuse")):
        em = np.zeros(len(extra), rt3.MATERIAL)
        em["kind"] = [kind, rt3.MAT_LAMBERT, rt3.MAT_METAL, rt3.MAT_LAMBERT, rt3.MAT_FLAT]
        em["rgb"] = np.float32([[0.9, 0.9, 0.9], [0.8, 0.2, 0.2], [0.7, 0.7, 0.9], [0.2, 0.8, 0.3], [0.9, 0.8, 0.1]])
        em["param"] = [1.5, 0.0, 0.1, 0.0, 0.0]
        add("camera_inside_%s_sphere" % name, 100, 56, spheres=np.concatenate([cr[:300], extra]), smats=np.concatenate([mats[:300], em]))
    three, three_mats = rt3.scene_three_spheres()
    add("camera_update_three_spheres", 160, 90, spheres=three, smats=three_mats, lens_radius=0.0,
        cam=rt3.Camera().update(160, 90, 1.0, np.float32(160) / np.float32(90) * np.float32(2.0), 2.0).c)
    add("camera_update_weekend_wide", 65, 50, lens_radius=0.02, cam=rt3.Camera().update(65, 50, 0.5, 3.0, 2.5).c)
    for scale, tag in ((1e3, "x1000"), (1e-2, "x0.01")):
        shift = (3000.0, -2000.0, 5000.0)
        add("weekend_moved_%s" % tag, 100, 56, spheres=moved(cr, scale, shift), cam=book_camera(rt3, 100, 56, scale, shift),
            lens_radius=0.05 * scale, t_min=0.001 * scale)
    rng = np.random.default_rng(5)
    big = np.zeros((500, 4), np.float32)
    big[:, :3] = rng.uniform(-6.0, 6.0, (500, 3)) * np.float32([1.0, 0.3, 1.0])
    big[:, 3] = rng.uniform(1.5, 3.0, 500)
    bm = np.zeros(500, rt3.MATERIAL)
    bm["kind"] = rng.choice([rt3.MAT_LAMBERT, rt3.MAT_METAL, rt3.MAT_DIELECTRIC, rt3.MAT_FLAT], 500)
    bm["rgb"] = rng.uniform(0.2, 0.9, (500, 3))
    bm["param"] = np.where(bm["kind"] == rt3.MAT_DIELECTRIC, 1.5, 0.2)
    add("500_large_overlapping_spheres", 100, 56, spheres=big, smats=bm, max_depth=6)
    return cases


_CASES = None


def get_cases(rt3):
    global _CASES
    if _CASES is None:
        _CASES = make_cases(rt3)
    return _CASES


CASE_NAMES = (["weekend_320x180"] + ["weekend_w%d" % w for w in (17, 63, 65, 100)] +
              ["weekend_shard%d_rows%d" % (i, r) for r in (1, 5) for i in range(3)] +
              ["weekend_spp1", "weekend_spp9_stratified", "weekend_spp5", "weekend_lens0", "weekend_lens0.5",
               "camera_inside_glass_sphere", "camera_inside_diffuse_sphere", "camera_update_three_spheres", "camera_update_weekend_wide",
               "weekend_moved_x1000", "weekend_moved_x0.01", "500_large_overlapping_spheres"])


def test_the_case_list_is_complete(rt3):
    assert sorted(CASE_NAMES) == sorted(get_cases(rt3))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_frames_equal_the_unfiltered_kernel_and_the_oracle_whatever_the_lists_do(rt3, renderer, name):
    case = get_cases(rt3)[name]
    want, casts = oracle_render(case)
    renderer.force_brute(True)
    try:
        brute = hip_render(renderer, case)
    finally:
        renderer.force_brute(False)
    assert np.array_equal(brute, want)
    n_sph = len(case["spheres"])
    seen = {}
    for knobs in KNOBS:
        with env(knobs):
            got = hip_render(renderer, case, upload=False)
            st = renderer.stats()
        tag = repr(knobs)
        assert np.array_equal(got, brute), tag
        assert st.ray_casts == casts and st.prim_tests == casts * n_sph, tag
        assert st.filter_tests % n_sph == 0 and st.filter_tests <= casts * n_sph, tag
        seen[tag] = st
    off, zero = seen[repr(KNOBS[1])], seen[repr(KNOBS[2])]
    assert off.filter_tests == off.ray_casts * n_sph                    # lists off: every cast takes the matrix filter, as before
    assert zero.filter_tests <= off.filter_tests and zero.exact_tests <= off.exact_tests     # threshold 0: only empty lists are traced at restock time
    everything = seen[repr(KNOBS[4])]
    assert everything.filter_tests == (casts - case_samples(rt3, case)) * n_sph      # every primary ray was traced at restock time


def case_samples(rt3, case):
    p = rt3.make_params(**case["params"])
    return rt3.rows_owned(p) * p.width * p.spp


def test_lists_save_matrix_work_on_the_book_scene(rt3, renderer):
    case = get_cases(rt3)["weekend_320x180"]
    hip_upload(renderer, case)
    st = {}
    for tag, knobs in (("on", {}), ("off", {"RT3_PRIMARY_LISTS": "0"})):
        with env(knobs):
            hip_render(renderer, case, upload=False)
            st[tag] = renderer.stats()
    assert st["on"].ray_casts == st["off"].ray_casts
    assert st["on"].mfma_instructions < st["off"].mfma_instructions
    assert st["on"].filter_tests < st["off"].filter_tests == st["off"].ray_casts * len(case["spheres"])


def test_progressive_render_in_two_unequal_parts(rt3, renderer):
    case = dict(get_cases(rt3)["weekend_w100"])
    case["params"] = dict(case["params"], spp=7)
    want, _ = oracle_render(case)
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    for knobs in KNOBS:
        with env(knobs):
            renderer.render_path_range(case["cam"], p, 0, 2)
            got = renderer.render_path_range(case["cam"], p, 2, 5)
        assert np.array_equal(got, want), knobs


@pytest.mark.parametrize("field,value", [("origin", float("nan")), ("horizontal", float("inf")), ("lower_left_corner", float("nan"))])
def test_a_non_finite_camera_behaves_as_with_lists_off(rt3, renderer, field, value):
    case = dict(get_cases(rt3)["weekend_w100"])
    cam = rt3.rt3_camera.from_buffer_copy(bytes(case["cam"]))
    getattr(cam, field)[1] = value
    case["cam"] = cam
    hip_upload(renderer, case)
    results = []
    for knobs in ({"RT3_PRIMARY_LISTS": "0"}, {}, {"RT3_PRIMARY_LIST_MAX": "1000"}):
        with env(knobs):
            try:
                results.append(("frame", hip_render(renderer, case, upload=False)))
            except rt3.Fatal as e:
                results.append(("error", str(e)))
    for kind, what in results[1:]:
        assert kind == results[0][0]
        assert np.array_equal(what, results[0][1]) if kind == "frame" else what == results[0][1]


def unpack(masks, n_sph):
    bits = (masks[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(len(masks), -1)[:, :n_sph].astype(bool)


SUPERSET_CASES = ["weekend_320x180", "weekend_w17", "weekend_w63", "weekend_w65", "weekend_shard1_rows1", "weekend_shard2_rows5", "weekend_lens0",
                  "weekend_lens0.5", "camera_inside_glass_sphere", "camera_update_three_spheres", "camera_update_weekend_wide", "weekend_moved_x1000",
                  "weekend_moved_x0.01", "500_large_overlapping_spheres"]


@pytest.mark.parametrize("name", SUPERSET_CASES)
def test_the_lists_hold_every_sphere_a_primary_ray_can_meet(rt3, renderer, name):
    case = get_cases(rt3)[name]
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    masks = renderer.debug_primary_lists(case["cam"], p)
    cr = case["spheres"]
    assert masks.shape == (-(-rt3.rows_owned(p) * p.width // 64), -(-len(cr) // 32))
    lists = unpack(masks, len(cr))
    direct = M.direct_list(cr)
    no_list = (masks == 0xFFFFFFFF).all(1)                              # "no list" (a beam too wide for the closed form): every bit set
    never = np.flatnonzero(~lists[~no_list].any(0))
    assert set(direct) <= set(never.tolist())                           # the direct spheres are on no list (every ray tests them anyway)
    mp = M.params(p.width, p.height, p.lens_radius, p.tile_rows, p.tile_index, p.tile_count)
    pix, o, d = M.primary_rays(case["cam"], mp, 200000, np.random.default_rng(11))
    hits, missed = M.misses(lists, pix, o, d, cr, direct)
    print("%s: %d groups, list lengths %s; %d candidate pairs of 200000 rays, %d missed" % (name, len(lists), M.length_stats(lists), hits, missed))
    assert missed == 0                                                  # (hits can be 0: every sphere of a tiny scene may be a direct one)
    # and the CPU model of the builder lists the same spheres, up to pairs that sit within rounding of the rule's edge
    model = M.build_lists(case["cam"], mp, cr, direct)
    assert (model != lists).mean() < 1e-4
