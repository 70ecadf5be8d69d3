"""The numpy restatement of adaptive sampling (tests/adaptive_ref.py) pinned on the CPU: the active pixels per round it yields on two scenes are
the ones measured on the oracle when the rule was specified.  The GPU tests compare against this restatement; these pins keep them from
passing vacuously (a restatement in which no pixel ever left, or every pixel left at once, would satisfy a bit-exact comparison too)."""
import numpy as np

import adaptive_ref
from cases import rt3


def run(oracle, cr, mats, cam, min_spp, step_spp, **params):
    p = oracle.make_params(**params)
    return adaptive_ref.render_adaptive(oracle.copy_camera(cam), p, 0.05, min_spp, step_spp, 0.01,
                                        spheres=cr, smats=np.ascontiguousarray(mats).view(oracle.MATERIAL), threads=16)


def test_weekend_160x90_budget_128(oracle):
    cr, mats = rt3.scene_weekend(42)
    cam = rt3.weekend_camera(160, 90).c
    ref = run(oracle, cr, mats, cam, 16, 16, width=160, height=90, spp=128, max_depth=50, seed=1, flags=1 | oracle.FLAG_VARIANCE, lens_radius=0.05)
    assert ref["active_counts"] == [14400, 10586, 8532, 6967, 5663, 4642, 3866, 3091]
    counts = ref["counts"]
    assert abs((counts == 16).mean() - 0.265) < 0.001 and abs((counts == 128).mean() - 0.215) < 0.001
    assert abs(counts.sum() / (14400 * 128) - 0.50) < 0.01
    assert sorted(ref["levels"]) == list(range(16, 129, 16))
    # a pixel's sums are the oracle's sums of its own level, and the frame is put together the same way
    for n, (img, acc, sq) in ref["levels"].items():
        at = counts == n
        assert np.array_equal(ref["acc"][at], acc[at]) and np.array_equal(ref["sq"][at], sq[at])
    assert adaptive_ref.expected_frame(ref).min() > 0


def test_three_spheres_64x36_budget_64(oracle):
    cr, mats = rt3.scene_three_spheres()
    cam = rt3.Camera().update(64, 36, 1.0, np.float32(64) / np.float32(36) * np.float32(2.0), 2.0).c
    ref = run(oracle, cr, mats, cam, 8, 8, width=64, height=36, spp=64, max_depth=8, seed=1, flags=1 | oracle.FLAG_VARIANCE)
    assert ref["active_counts"] == [2304, 1499, 1311, 1000, 802, 668, 539, 466]
    assert abs(ref["counts"].sum() / (2304 * 64) - 0.47) < 0.01


def test_the_rule_in_float32():
    """Known answers of the rule: a constant pixel is converged, a NaN compares false, the clamp of a negative variance, and the dilation
    stops at a row-block edge of a shard."""
    acc = np.zeros((1, 4, 4), np.float32); sq = np.zeros((1, 4, 4), np.float32)
    n = np.full((1, 4), 16, np.uint32)
    acc[0, 0, :3] = 8.0; sq[0, 0, :3] = 4.0                               # 16 samples of 0.5: variance 0
    acc[0, 1, :3] = 8.0; sq[0, 1, :3] = 8.0                               # 8 samples of 1, 8 of 0: mean 0.5, variance 0.25 per channel
    acc[0, 2, :3] = np.nan
    acc[0, 3, :3] = 8.0; sq[0, 3, :3] = 3.0                               # squares below the mean's square: clamped to 0
    u = adaptive_ref.unconverged(acc, sq, n, 0.05, 0.01)
    assert u.tolist() == [[False, True, False, False]]
    # e2 = 0.75 / 16 = 0.046875; lim = t * 1.51: the threshold at which pixel 1 stops is sqrt(0.046875) / 1.51 = 0.14338
    assert adaptive_ref.unconverged(acc, sq, n, 0.1433, 0.01)[0, 1] and not adaptive_ref.unconverged(acc, sq, n, 0.1434, 0.01)[0, 1]
    u = np.zeros((4, 5), bool); u[1, 2] = True
    whole = adaptive_ref.dilate(u, np.arange(4))
    assert whole.sum() == 9 and whole[0:3, 1:4].all()
    shard = adaptive_ref.dilate(u, np.array([2, 3, 6, 7]))               # tile_rows 2, tile_index 1, tile_count 2: local rows 1 and 2 are not neighbours
    assert shard.sum() == 6 and shard[0:2, 1:4].all()
