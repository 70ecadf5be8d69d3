"""What a full sphere upload decides before it builds anything, restated in numpy: sphere_filter_centre and
sphere_direct_list of the library, which rt3_debug_sphere_plan exposes and the device form of the upload has to reproduce.

centre     per axis the median at index m // 2 of the m finite coordinates; 0 on an axis without one
scene      the median at index n // 2 of the centres' distances from the centre, in double, a non-finite distance counted as 0
candidate  ratio = float32(double(r) / max(max(dist, scene), 1e-30)) >= 0.5 (a NaN is none)
direct     at most four candidates with the largest ratios; unique when there are at most four or the ratios are pairwise distinct"""
import numpy as np

F = np.float32


def as_records(center_radius):
    return np.ascontiguousarray(center_radius, F).reshape(-1, 4)


def filter_centre(center_radius):
    cr = as_records(center_radius)
    out = np.zeros(3, F)
    for a in range(3):
        c = cr[:, a][np.isfinite(cr[:, a])]
        if len(c):
            out[a] = np.sort(c)[len(c) // 2]
    return out


def distances(center_radius, centre):
    cr = as_records(center_radius)
    with np.errstate(invalid="ignore", over="ignore"):
        d = cr[:, :3].astype(np.float64) - np.asarray(centre, F).astype(np.float64)
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def scene_size(center_radius, centre):
    d = distances(center_radius, centre)
    if len(d) == 0:
        return 0.0
    d = np.where(np.isfinite(d), d, 0.0)
    return float(np.sort(d)[len(d) // 2])


def ratios(center_radius, centre):
    cr = as_records(center_radius)
    d = distances(cr, centre)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (cr[:, 3].astype(np.float64) / np.maximum(np.maximum(d, scene_size(cr, centre)), 1e-30)).astype(F)


def candidates(center_radius, centre=None):
    """(indices, ratios) of the candidates, in index order."""
    centre = filter_centre(center_radius) if centre is None else centre
    r = ratios(center_radius, centre)
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(r >= F(0.5))[0]
    return idx.astype(np.uint32), r[idx]


def choice_is_unique(center_radius):
    """At most four candidates, or pairwise distinct ratios: the direct list is then one set, whatever selects it."""
    idx, r = candidates(center_radius)
    return len(idx) <= 4 or len(np.unique(r)) == len(r)


def direct_set(center_radius):
    """The direct list as a sorted index array where the choice is unique (else: one valid choice, the lowest indices among equals)."""
    idx, r = candidates(center_radius)
    if len(idx) <= 4:
        return np.sort(idx)
    order = np.lexsort((idx, -r.astype(np.float64)))                   # ratio descending, then index ascending
    return np.sort(idx[order[:4]])


def is_valid_choice(center_radius, chosen):
    """Any four of the largest: every chosen sphere is a candidate and no sphere left out has a larger ratio than a chosen one."""
    idx, r = candidates(center_radius)
    chosen = np.asarray(chosen, np.uint32)
    if len(set(chosen.tolist())) != len(chosen) or len(chosen) != min(len(idx), 4) or not set(chosen.tolist()) <= set(idx.tolist()):
        return False
    if len(idx) <= 4:
        return True
    ratio_of = dict(zip(idx.tolist(), r.tolist()))
    weakest = min(ratio_of[i] for i in chosen.tolist())
    return all(ratio_of[i] <= weakest for i in idx.tolist() if i not in set(chosen.tolist()))


def usable_ids(center_radius, direct):
    """The spheres in the group order: not on the direct list, a finite centre and a finite r^2 (in f32)."""
    cr = as_records(center_radius)
    with np.errstate(over="ignore", invalid="ignore"):
        ok = np.isfinite(cr[:, :3]).all(axis=1) & np.isfinite(cr[:, 3] * cr[:, 3])
    ok[np.asarray(direct, np.int64)] = False
    return np.nonzero(ok)[0].astype(np.uint32)
