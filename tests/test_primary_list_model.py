"""The strip lists' closed form (tools/primary_list_model.py, the float64 twin of k_primary_lists) against brute force, without a GPU: every sphere
that a random primary ray — made by start_path's law in float32, a third of them at the extremes of jitter and lens — passes sphere_root's
candidate rule for (float64, widened to disc > -1e-9 r^2) must be on the list of the ray's group of 64 pixels.  0 misses, and the list lengths
the design rests on."""
import os
import sys

import numpy as np
import pytest

from cases import ROOT, rt3

sys.path.insert(0, os.path.join(ROOT, "tools"))
import primary_list_model as M  # noqa: E402

RAYS = 200000


def check(cam, p, cr, seed):
    direct = M.direct_list(cr)
    lists = M.build_lists(cam, p, cr, direct)
    pix, o, d = M.primary_rays(cam, p, RAYS, np.random.default_rng(seed))
    hits, missed = M.misses(lists, pix, o, d, cr, direct)
    return lists, hits, missed


def test_bench_scene_lists_are_short_and_complete():
    cr, _ = rt3.scene_weekend(42)
    lists, hits, missed = check(rt3.weekend_camera(1920, 1080).c, M.params(1920, 1080, lens_radius=0.05), cr, 1)
    st = M.length_stats(lists)
    print(st, hits, missed)
    assert hits > 100000 and missed == 0
    assert st["groups"] == 32400 and st["median"] == 1 and st["p90"] == 6 and st["p99"] == 10 and st["max"] == 12
    assert 2.1 < st["mean"] < 2.25 and 0.24 < st["empty"] < 0.25


def test_small_frames_have_long_lists_and_stay_complete():
    cr, _ = rt3.scene_weekend(42)
    lists, hits, missed = check(rt3.weekend_camera(400, 225).c, M.params(400, 225, lens_radius=0.05), cr, 2)
    st = M.length_stats(lists)
    print(st, hits, missed)
    assert hits > 100000 and missed == 0 and st["max"] > 25            # some lists are long: the kernel needs its fallback


@pytest.mark.parametrize("k", range(12))
def test_random_cameras_and_scenes(k):
    rng = np.random.default_rng(100 + k)
    n = 300
    cr = np.zeros((n, 4), np.float32)
    cr[:, :3] = rng.uniform(-20.0, 20.0, (n, 3))
    cr[:, 3] = 10.0 ** rng.uniform(-1.0, 1.0, n)                        # two decades of radius
    look_from = rng.uniform(-15.0, 15.0, 3)
    if k % 4 == 0:                                                      # the camera inside a sphere
        cr[0] = (*look_from, 4.0)
    w, h = int(rng.integers(64, 321)), int(rng.integers(20, 90))       # most widths end a strip mid-row
    lens = (0.0, 0.05, 0.5)[k % 3]
    cam = rt3.Camera().look_at(w, h, tuple(look_from), tuple(rng.uniform(-5.0, 5.0, 3)), (0.0, 1.0, 0.0), float(rng.uniform(17.0, 88.0)),
                               float(rng.uniform(5.0, 30.0))).c
    tiles = dict(tile_rows=int(rng.integers(1, 6)), tile_index=int(rng.integers(0, 3)), tile_count=3) if k % 5 == 4 else {}
    lists, hits, missed = check(cam, M.params(w, h, lens_radius=lens, **tiles), cr, 200 + k)
    print(w, h, lens, M.length_stats(lists), hits, missed)
    assert hits > 0 and missed == 0
