"""k_trace_mfma32's wave-uniform bookkeeping (refill_from_traced_stock in rt3_matrix_filter.hpp, shade_lane in rt3_path.hpp): the
counter-hash table, restocks whose 64 items share one sample (the first item's decomposition plus the lane index, with the row wrap) or one aligned
pixel group (the list in scalar registers), and the skipped compaction.  None of it may change a bit: every case renders with k_trace_mfma32 and with
the arbiter (rt3_debug_force_brute: k_trace_brute, which has none of these paths); frames are equal word for word and so are the ray casts.  The cases
are the smallest at which each branch, and each fallback next to it, runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cases import hip_upload

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def weekend(rt3, w, h, **params):
    cr, mats = rt3.scene_weekend(42)
    kw = dict(width=w, height=h, spp=4, max_depth=12, seed=3, flags=1, lens_radius=0.05)
    kw.update(params)
    return dict(spheres=cr, smats=mats, cam=rt3.weekend_camera(w, h).c, params=kw)


def hall_of_mirrors(rt3, w, h, **params):
    """The camera inside a slightly fuzzy metal shell, with a glass and a diffuse sphere: hardly a path ends before max_depth, and every path draws
    the random numbers of its depth — the unit vector's two (metal fuzz, Lambert) and the dielectric's one."""
    cr = np.float32([[0.0, 0.0, 0.0, 50.0], [0.0, 0.0, -3.0, 1.0], [2.2, 0.0, -3.0, 1.0], [-2.2, 0.0, -3.0, 1.0]])
    mats = np.zeros(4, rt3.MATERIAL)
    mats["kind"] = [rt3.MAT_METAL, rt3.MAT_DIELECTRIC, rt3.MAT_LAMBERT, rt3.MAT_DIELECTRIC]
    mats["rgb"] = np.float32([[0.95, 0.95, 0.95], [1.0, 1.0, 1.0], [0.9, 0.8, 0.7], [1.0, 1.0, 1.0]])
    mats["param"] = [0.05, 1.5, 0.0, 1.3]
    kw = dict(width=w, height=h, spp=4, max_depth=12, seed=5, flags=1)
    kw.update(params)
    cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0).c
    return dict(spheres=cr, smats=mats, cam=cam, params=kw)


def render_both(rt3, renderer, case, render):
    """render(renderer, params) -> (what to compare, ray casts), with the arbiter and with k_trace_mfma32."""
    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    renderer.force_brute(True)
    try:
        want = render(renderer, p)
    finally:
        renderer.force_brute(False)
    return want, render(renderer, p)


def one_render(case):
    def render(r, p):
        frame = r.render_path(case["cam"], p)
        return frame, r.stats().ray_casts
    return render


def check(rt3, renderer, case):
    (want, want_casts), (got, casts) = render_both(rt3, renderer, case, one_render(case))
    print("%s: %d ray casts, %d of %d pixels differ" % (case["params"], casts, int((got != want).sum()), got.size))
    assert np.array_equal(got, want)
    assert casts == want_casts
    return got, casts


def test_restocks_over_three_rows_and_two_samples(rt3, renderer):
    """50 x 3, 5 spp: 150 owned pixels, so restocks of 64 items span three rows and the third one two samples — the row wrap runs more than once per
    restock, and the per-lane fallback runs next to the one-sample path."""
    check(rt3, renderer, weekend(rt3, 50, 3, spp=5))


@pytest.mark.parametrize("spp", [4, 5])
def test_every_restock_uniform(rt3, renderer, spp):
    """128 x 2: every restock is one sample, one aligned group, no row wrap.  4 spp is a perfect square (strata: edge != 0), 5 is not."""
    check(rt3, renderer, weekend(rt3, 128, 2, spp=spp))


def test_interleaved_rows_of_a_shard(rt3, renderer):
    """64 x 9, the middle shard of three in blocks of one row: frame_row maps the incremental row index."""
    check(rt3, renderer, weekend(rt3, 64, 9, tile_rows=1, tile_count=3, tile_index=1))


def test_counter_hash_table_and_its_fallback(rt3, renderer):
    """max_depth 1, 2, the table's cap and cap + 6, in a closed hall of mirrors with glass in it: paths reach every depth, those at or beyond the
    cap compute their hashes."""
    cap = len(rt3.debug_ctr_table())
    deepest = 0
    for depth in (1, 2, cap, cap + 6):
        case = hall_of_mirrors(rt3, 64, 6, max_depth=depth)
        _, casts = check(rt3, renderer, case)
        deepest = max(deepest, casts / (64 * 6 * 4))
    # mean casts per path above the cap means some path ran past it.  This relies on the closed shell: no ray reaches the sky, the fuzz is small, so
    # nearly every path lives to max_depth.  (A wrong fallback would show in the frames, which the arbiter computes without a table.)
    assert deepest > cap


@pytest.mark.parametrize("lens", [0.0, 0.05])
def test_both_ray_generation_branches(rt3, renderer, lens):
    check(rt3, renderer, weekend(rt3, 128, 4, lens_radius=lens))


def test_frame_width_not_a_multiple_of_64(rt3, renderer):
    """100 x 5: restocks that straddle two pixel groups (the ballot loop and the lane-held words) and wrap a row once."""
    check(rt3, renderer, weekend(rt3, 100, 5))


def test_a_render_continued_across_calls(rt3, renderer):
    """Samples [0, 3) then [3, 5) against one render of 5, under the arbiter."""
    case = weekend(rt3, 100, 5, spp=5)

    def whole(r, p):
        frame = r.render_path(case["cam"], p)
        return frame, r.stats().ray_casts

    def in_two(r, p):
        r.render_path_range(case["cam"], p, 0, 3)
        casts = r.stats().ray_casts
        frame = r.render_path_range(case["cam"], p, 3, 2)
        return frame, casts + r.stats().ray_casts

    hip_upload(renderer, case)
    p = rt3.make_params(**case["params"])
    renderer.force_brute(True)
    try:
        want, want_casts = whole(renderer, p)
    finally:
        renderer.force_brute(False)
    got, casts = in_two(renderer, p)
    assert np.array_equal(got, want)
    assert casts == want_casts


def test_the_list_form_keeps_the_per_lane_index_path(rt3, renderer):
    """rt3_render_path_adaptive: after the first round the items are (sample, active[j]) — no consecutive pixels.  Same call under the arbiter."""
    case = weekend(rt3, 96, 54, spp=24, max_depth=50, seed=1)

    def render(r, p):
        pixels, counts = r.render_adaptive(case["cam"], p, threshold=0.05, min_spp=8, step_spp=8, dark=0.01)
        return (pixels, counts), r.stats().ray_casts

    ((want, want_counts), want_casts), ((got, counts), casts) = render_both(rt3, renderer, case, render)
    share = float((counts > 8).mean())
    print("pixels that took more than the first round: %.3f" % share)
    assert 0.02 < share < 0.9                                     # a sparse active list, not an empty or a full one
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(got, want)
    assert casts == want_casts


CHILD_CASE = dict(w=100, h=6, spp=5)


@pytest.mark.parametrize("knobs", [{}, {"RT3_PRIMARY_LISTS": "0"}, {"RT3_PRIMARY_LIST_MAX": "0"}], ids=["default", "lists_off", "list_max_0"])
def test_list_fetch_variants_in_a_fresh_process(rt3, renderer, tmp_path, knobs):
    """Lists on, off, and on with only empty lists traced: each in a child process of its own, against the arbiter in this one."""
    case = weekend(rt3, CHILD_CASE["w"], CHILD_CASE["h"], spp=CHILD_CASE["spp"])
    hip_upload(renderer, case)
    renderer.force_brute(True)
    try:
        want = renderer.render_path(case["cam"], rt3.make_params(**case["params"]))
        want_casts = renderer.stats().ray_casts
    finally:
        renderer.force_brute(False)
    out = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RT3_PRIMARY_LISTS", "RT3_PRIMARY_LIST_MAX", "RT3_BRUTE")}
    env.update(knobs)
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, cwd=HERE, timeout=120)
    z = np.load(out)
    assert np.array_equal(z["frame"], want)
    assert int(z["casts"]) == want_casts


def child(out):
    from cases import rt3
    r = rt3.initialize_renderer(0)
    case = weekend(rt3, CHILD_CASE["w"], CHILD_CASE["h"], spp=CHILD_CASE["spp"])
    hip_upload(r, case)
    frame = r.render_path(case["cam"], rt3.make_params(**case["params"]))
    np.savez(out, frame=frame, casts=np.uint64(r.stats().ray_casts))
    r.close()


if __name__ == "__main__":
    child(sys.argv[1])
