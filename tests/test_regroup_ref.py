"""tests/regroup_ref.py, the numpy statement of rt3_regroup's order, against the properties that define it.  No GPU."""
import numpy as np
import pytest

import regroup_ref as G


def random_centres(n, seed, grid=None):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    if grid:                                                           # frequent ties
        c = np.round(c / grid).astype(np.float32) * np.float32(grid)
    return c * np.array([1.0, 0.3, 2.0], np.float32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 100, 513, 4097, 10000])
def test_permutation_and_part_sizes(n):
    c = random_centres(n, n)
    order = G.regroup_order(np.arange(n), c)
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
    parts = G.parts_of(n)
    leaves = [(b, e) for b, e in parts if e - b <= G.GROUP]
    assert sorted(leaves) == [(b, min(b + G.GROUP, n)) for b in range(0, n, G.GROUP)]       # only the very last group is short
    for b, e in parts:
        count = e - b
        if count <= G.GROUP:
            continue
        h = G.split_half(count)
        unit = 64 if count > 64 else 8
        assert 0 < h < count and h % unit == 0 and abs(h - count / 2) < unit


@pytest.mark.parametrize("n,grid", [(100, None), (1000, None), (1000, 10.0), (5000, 25.0)])
def test_left_is_not_larger_than_right_on_the_split_axis(n, grid):
    c = random_centres(n, 3 * n, grid)
    order = G.regroup_order(np.arange(n), c)
    # replay: the final order of a part is a permutation of what the part held when it was cut, so its box and axis can be recomputed
    for b, e in G.parts_of(n):
        if e - b <= G.GROUP:
            continue
        cc = c[order[b:e]]
        axis = G.split_axis(cc)
        h = G.split_half(e - b)
        assert cc[:h, axis].max() <= cc[h:, axis].min()


def test_ties_keep_index_order_and_zeros_are_equal():
    n = 64
    c = np.zeros((n, 3), np.float32)
    c[:, 0] = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-0.0))        # one key: nothing may move
    c[0, 0], c[n - 1, 0] = -1.0, 1.0                                   # (x is the longest axis)
    order = G.regroup_order(np.arange(n), c)
    assert np.array_equal(order, np.arange(n, dtype=np.uint32))
    # all coordinates equal on every axis: axis 0 (first maximum), and the order stays
    order = G.regroup_order(np.arange(200), np.ones((200, 3), np.float32))
    assert np.array_equal(order, np.arange(200, dtype=np.uint32))
    # ties inside a larger scene: equal keys appear in ascending index order within every sorted part of the top level
    c = random_centres(300, 5, grid=20.0)
    axis = G.split_axis(c)
    order = G.regroup_order(np.arange(300), c)
    h = G.split_half(300)
    left = set(order[:h].tolist())
    key = c[:, axis]
    cut = np.sort(key, kind="stable")[h - 1]
    tied = [i for i in range(300) if key[i] == cut]
    inside = [i in left for i in tied]
    assert inside == sorted(inside, reverse=True)                      # the tied ids that went left are the lowest ones


def test_first_maximum_picks_the_axis():
    c = np.zeros((16, 3), np.float32)
    c[:, 1] = np.arange(16)[::-1]
    c[:, 2] = np.arange(16)                                            # y and z have the same extent: y wins
    order = G.regroup_order(np.arange(16), c)
    assert set(order[:8].tolist()) == set(range(8, 16))


def test_pure_function_of_the_positions():
    n = 3000
    c = random_centres(n, 11, grid=5.0)
    first = G.regroup_order(np.arange(n), c)
    rng = np.random.default_rng(1)
    assert np.array_equal(G.regroup_order(rng.permutation(n), c), first)      # whatever order the ids come in
    assert np.array_equal(G.regroup_order(first, c), first)
    sub = np.arange(0, n, 3)                                           # a region that is not every primitive
    got = G.regroup_order(sub[::-1], c)
    assert np.array_equal(np.sort(got), sub.astype(np.uint32))


def test_unusable_records_take_the_filter_centre():
    cr = np.array([[1, 2, 3, 1], [np.nan, 0, 0, 1], [4, 5, 6, -1], [7, 8, 9, 1e30], [np.inf, 0, 0, 1]], np.float32)
    c = G.sphere_centres(cr, (10.0, 20.0, 30.0))
    assert np.array_equal(c, np.array([[1, 2, 3], [10, 20, 30], [10, 20, 30], [10, 20, 30], [10, 20, 30]], np.float32))


def test_faces_without_a_usable_bound_take_the_filter_centre():
    verts = np.array([[0, 0, 0, 0], [3, 0, 0, 0], [0, 3, 0, 0], [6, 6, 6, 0], [np.inf, 0, 0, 0]], np.float32)
    faces = np.zeros(4, [("v1", "<u4"), ("v2", "<u4"), ("v3", "<u4")])
    faces["v1"], faces["v2"], faces["v3"] = [0, 0, 0, 0], [1, 1, 3, 1], [2, 1, 3, 4]      # a triangle, two collapsed ones, a non-finite one
    centre = G.mesh_filter_centre(verts)
    assert np.array_equal(centre, np.array([3, 3, 3], np.float32))                          # (the infinite coordinate does not count)
    c = G.face_centres(faces, verts, centre)
    assert np.array_equal(c, np.array([[1, 1, 0], [3, 3, 3], [3, 3, 3], [3, 3, 3]], np.float32))


def test_padding_and_leaf_sets():
    p = G.padded(np.arange(70, dtype=np.uint32))
    assert len(p) == 128 and (p[70:] == G.PAD).all()
    sets = G.leaf_sets(p)
    assert len(sets) == 16 and sets[8] == frozenset(range(64, 70)) and sets[9] == frozenset()
