"""The filter centre and the direct list of a sphere upload without a GPU: the numpy restatement of tests/scene_build_ref.py
against the library's own host functions (rt3_debug_sphere_plan), on the scenes and the corner cases the device form is later held to."""
import numpy as np
import pytest

import scene_build_ref as B

F = np.float32


def cloud(n, seed, big=()):
    """n small spheres in a box of 10 units, then one sphere of radius r some 20 units out for every r of `big`."""
    rng = np.random.default_rng(seed)
    cr = np.empty((n + len(big), 4), F)
    cr[:n, :3] = rng.uniform(-5.0, 5.0, (n, 3)).astype(F)
    cr[:n, 3] = F(0.1)
    for k, r in enumerate(big):
        cr[n + k] = (20.0 + k, -3.0 * k, 2.0 * k, r)
    return cr


def hand_made():
    nan, inf = np.nan, np.inf
    out = {
        "n0": np.zeros((0, 4), F),
        "n1": np.array([[1.0, 2.0, 3.0, 0.5]], F),
        "n2": np.array([[1.0, 2.0, 3.0, 0.5], [-4.0, 0.0, 9.0, 0.25]], F),
        "odd": cloud(41, 1),
        "even": cloud(42, 1),
        "one_axis_nan": cloud(30, 2),
        "one_axis_inf": cloud(30, 3),
        "all_axes": cloud(30, 4),
        "no_finite_axis": np.array([[nan, 1.0, 2.0, 1.0], [inf, 3.0, -1.0, 1.0], [-inf, 0.0, 0.0, 1.0]], F),
        "equal_centres": np.tile(np.array([[2.0, -1.0, 7.0, 0.5]], F), (9, 1)),
        "four": cloud(40, 5, big=(50.0, 60.0, 70.0, 80.0)),
        "five": cloud(40, 6, big=(50.0, 60.0, 70.0, 80.0, 90.0)),
        "five_tied": cloud(40, 7, big=(50.0, 50.0, 50.0, 50.0, 50.0)),
        "nan_ratio": cloud(30, 8),
    }
    out["one_axis_nan"][3::7, 1] = nan
    out["one_axis_inf"][2::5, 2] = inf
    out["one_axis_inf"][3::5, 2] = -inf
    out["all_axes"][4::6, :3] = (nan, inf, -inf)
    out["five_tied"][40:, :3] = (20.0, 0.0, 0.0)                          # one centre, one radius: five equal ratios
    out["nan_ratio"][5, 0] = inf                                          # an infinite distance ...
    out["nan_ratio"][5, 3] = inf                                          # ... under an infinite radius: inf / inf
    out["nan_ratio"][6, 3] = inf                                          # (and an infinite radius at a finite distance IS a candidate)
    return out


def scenes(rt3):
    out = {"weekend": rt3.scene_weekend(42)[0], "stress700": rt3.scene_stress(700, 43)[0]}
    out.update(hand_made())
    return out


def check(rt3, name, cr):
    centre, direct = rt3.sphere_plan(cr)
    want_centre = B.filter_centre(cr)
    idx, r = B.candidates(cr)
    print("%s: n = %d, centre %s / %s, %d candidates, direct %s" % (name, len(cr), centre, want_centre, len(idx), direct))
    assert centre.dtype == F and np.array_equal(centre, want_centre), name
    if B.choice_is_unique(cr):
        assert np.array_equal(direct, B.direct_set(cr)), name
    assert B.is_valid_choice(cr, direct), name                             # ties among more than four: any four of the largest


@pytest.mark.parametrize("name", ["weekend", "stress700"] + sorted(hand_made()))
def test_the_restatement_is_the_hosts_plan(rt3, name):
    check(rt3, name, scenes(rt3)[name])


def test_the_cases_are_the_ones_they_are_named_for(rt3):
    S = scenes(rt3)
    count = {k: len(B.candidates(v)[0]) for k, v in S.items()}
    assert count["weekend"] == 1 and rt3.sphere_plan(S["weekend"])[1].tolist() == [0]      # the ground sphere
    assert count["four"] == 4 and count["five"] == 5 and B.choice_is_unique(S["five"])
    assert count["five_tied"] == 5 and not B.choice_is_unique(S["five_tied"])
    assert count["equal_centres"] == 9 and not B.choice_is_unique(S["equal_centres"])       # distance 0 everywhere: every ratio is +inf
    assert np.isnan(B.ratios(S["nan_ratio"], B.filter_centre(S["nan_ratio"]))[5]) and 5 not in rt3.sphere_plan(S["nan_ratio"])[1]
    assert 6 in rt3.sphere_plan(S["nan_ratio"])[1]
    assert np.array_equal(rt3.sphere_plan(S["no_finite_axis"])[0], np.array([0.0, 1.0, 0.0], F))
    assert rt3.sphere_plan(S["n0"])[1].size == 0 and not rt3.sphere_plan(S["n0"])[0].any()
    # the scenes the GPU tests assert set equality on have one answer
    for k in ("weekend", "stress700", "four", "five"):
        assert B.choice_is_unique(S[k]), k
