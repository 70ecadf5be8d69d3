#!/usr/bin/env python3
"""CPU model of the strip lists (k_primary_lists, raytracer-3_amd/csrc/rt3_primary_lists.hpp): the builder's closed form in
float64 against brute force on random primary rays made by start_path's law in float32.

For every aligned group of 64 owned pixels the builder lists the spheres a primary ray of the group may meet: central line from the camera
origin to the centre of the group's footprint on the focus plane, widened by the lens radius at the origin and by the footprint's half-extent
at the focus plane.  The model answers two questions: is the list a superset of the truth (it must be: 0 misses), and how long are the lists.

    python3 tools/primary_list_model.py [width height [rays]]      (default: the bench frame, 1920 1080, 400000 rays)

CPU only, numpy only (the scene and the camera come from the host half of librt3hip.so, which needs no GPU); not part of the product.
"""
import os
import sys

import numpy as np

f32 = np.float32
LIST_EPS, LIST_DELTA, LIST_SLACK = 4e-6, 2.0 ** -18, 1e-6      # kListEps, kListDelta, kListSlack


def cam_vectors(c):
    """The four vectors of an rt3_camera (or anything with these attributes) as float32 arrays."""
    return {k: np.array(list(getattr(c, k)), f32) for k in ("origin", "horizontal", "vertical", "lower_left_corner")}


def rows_owned(p):
    if p["tile_count"] <= 1:
        return p["height"]
    return sum(1 for y in range(p["height"]) if (y // p["tile_rows"]) % p["tile_count"] == p["tile_index"])


def frame_row(p, lrow):
    if p["tile_count"] <= 1:
        return lrow
    lb, within = divmod(lrow, p["tile_rows"])
    return (lb * p["tile_count"] + p["tile_index"]) * p["tile_rows"] + within


def params(width, height, lens_radius=0.0, tile_rows=8, tile_index=0, tile_count=1):
    return dict(width=width, height=height, lens_radius=lens_radius, tile_rows=tile_rows, tile_index=tile_index, tile_count=tile_count)


def direct_list(cr):
    """sphere_direct_list (rt3_sphere_plan.hpp): the at most four spheres with the largest r / max(|C - c0|, R) above 1/2."""
    cr = np.asarray(cr, np.float64)
    if len(cr) == 0:
        return []
    c0 = np.array([np.sort(cr[np.isfinite(cr[:, a]), a])[np.isfinite(cr[:, a]).sum() // 2] if np.isfinite(cr[:, a]).any() else 0.0 for a in range(3)])
    dist = np.sqrt(((cr[:, :3] - c0.astype(f32)) ** 2).sum(1))
    scene = np.sort(np.where(np.isfinite(dist), dist, 0.0))[len(dist) // 2]
    with np.errstate(all="ignore"):
        ratio = (cr[:, 3] / np.maximum(np.maximum(dist, scene), 1e-30)).astype(f32)
    order = [i for i in np.argsort(-ratio, kind="stable") if ratio[i] >= 0.5]
    return sorted(order[:4])


def pieces(p):
    """(group, x0, nx, frame row) of every piece of a frame row that a group of 64 owned pixels covers."""
    w, npix = p["width"], rows_owned(p) * p["width"]
    out = []
    for g in range(-(-npix // 64)):
        q, end = g * 64, min(g * 64 + 64, npix)
        while q < end:
            lrow, x0 = divmod(q, w)
            nx = min(w - x0, end - q)
            out.append((g, x0, nx, frame_row(p, lrow)))
            q += nx
    return np.array(out, np.int64).reshape(-1, 4), -(-npix // 64)


def build_lists(cam, p, cr, direct=()):
    """The builder's formula, float64: bool [groups, spheres].  A group with no list has every sphere set."""
    c = {k: v.astype(np.float64) for k, v in cam_vectors(cam).items()} if not isinstance(cam, dict) else {k: np.asarray(v, np.float64) for k, v in cam.items()}
    o0, h, v, ll = c["origin"], c["horizontal"], c["vertical"], c["lower_left_corner"]
    cr = np.asarray(cr, f32).astype(np.float64)
    C, r2 = cr[:, :3], (cr[:, 3].astype(f32) * cr[:, 3].astype(f32)).astype(np.float64)       # the device record holds r^2 in f32
    pc, n_groups = pieces(p)
    lists = np.zeros((n_groups, len(cr)), bool)
    with np.errstate(all="ignore"):
        lh, lv = np.sqrt((h * h).sum()), np.sqrt((v * v).sum())
        mag = max(np.abs(o0).max(), (np.abs(ll) + np.abs(h) + np.abs(v)).max())
        delta = LIST_DELTA * mag
        R = delta
        if p["lens_radius"] > 0.0:
            lu, lvn = (h.astype(f32) / f32(lh)).astype(np.float64), (v.astype(f32) / f32(lv)).astype(np.float64)
            R = R + float(f32(p["lens_radius"])) * np.sqrt(1.0 + abs((lu * lvn).sum())) * (1.0 + 1e-5)
        if not (mag < 1e300) or not (R < 1e300):
            lists[:] = True
            return lists
        wm1, hm1 = p["width"] - 1.0, p["height"] - 1.0
        no_list = np.zeros(n_groups, bool)
        w = C - o0
        ww = (w * w).sum(1)
        far = np.sqrt(ww) + R
        r_eff = np.sqrt(r2 + LIST_EPS * (r2 + far * far))
        for lo in range(0, len(pc), 4096):
            g, x0, nx, y = pc[lo:lo + 4096].T
            uc, du = (x0 + 0.5 * (nx - 1)) / wm1, 0.5 * nx / wm1
            vc, dv = (p["height"] - 1 - y) / hm1, 0.5 / hm1
            a = ll + uc[:, None] * h + vc[:, None] * v - o0
            L = np.sqrt((a * a).sum(1))
            rho = du * lh + dv * lv + delta
            k = (R + rho) / L
            bad = ~(L > 0.0) | ~(k < 1.0) | ~(L < 1e300)
            sc = (a @ w.T) / L[:, None]
            d2 = ww[None, :] - sc * sc
            lam = sc / L[:, None]
            reach = (r_eff[None, :] + np.abs(1.0 - lam) * R + np.abs(lam) * rho[:, None]) * (1.0 + LIST_SLACK)
            cand = ~(d2 * (1.0 - k * k)[:, None] > reach * reach)
            np.logical_or.at(lists, g, cand)
            np.logical_or.at(no_list, g, bad)
    lists[:, list(direct)] = False
    lists[no_list] = True
    return lists


def primary_rays(cam, p, n, rng, extreme=1.0 / 3.0):
    """n random primary rays by start_path's law, float32 operation by operation: (owned pixel index, origin, unit direction).
    A share `extreme` of them sits at the ends of the jitter interval and on the rim of the lens."""
    c = cam_vectors(cam) if not isinstance(cam, dict) else {k: np.asarray(v, f32) for k, v in cam.items()}
    o0, h, v, ll = c["origin"], c["horizontal"], c["vertical"], c["lower_left_corner"]
    w, hgt, npix = p["width"], p["height"], rows_owned(p) * p["width"]
    pix = rng.integers(0, npix, n)
    lrow, x = np.divmod(pix, w)
    y = np.array([frame_row(p, int(q)) for q in range(rows_owned(p))], np.int64)[lrow]
    ext = rng.random(n) < extreme
    top = np.nextafter(f32(0.5), f32(0.0))
    jx = np.where(ext, rng.choice([f32(-0.5), top], n), rng.random(n, f32) - f32(0.5)).astype(f32)
    jy = np.where(ext, rng.choice([f32(-0.5), top], n), rng.random(n, f32) - f32(0.5)).astype(f32)
    u = ((x.astype(f32) + jx) / (f32(w) - f32(1.0))).astype(f32)
    vv = (((hgt - 1 - y).astype(f32) + jy) / (f32(hgt) - f32(1.0))).astype(f32)
    with np.errstate(all="ignore"):
        r = (((ll[None, :] + u[:, None] * h[None, :]).astype(f32) + vv[:, None] * v[None, :]).astype(f32) - o0[None, :]).astype(f32)
        o = np.repeat(o0[None, :], n, 0)
        if p["lens_radius"] > 0.0:
            lu = (h / np.sqrt((h * h).sum(dtype=f32))).astype(f32)
            lv = (v / np.sqrt((v * v).sum(dtype=f32))).astype(f32)
            xi2 = np.where(ext, np.nextafter(f32(1.0), f32(0.0)), rng.random(n, f32)).astype(f32)
            xi3 = rng.random(n, f32)
            rad = (f32(p["lens_radius"]) * np.sqrt(xi2)).astype(f32)
            a, b = (rad * np.cos(2.0 * np.pi * xi3).astype(f32)).astype(f32), (rad * np.sin(2.0 * np.pi * xi3).astype(f32)).astype(f32)
            f = ((a[:, None] * lu[None, :]).astype(f32) + (b[:, None] * lv[None, :]).astype(f32)).astype(f32)
            o = (o + f).astype(f32)
            r = (r - f).astype(f32)
        inv = (f32(1.0) / np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]).astype(f32) + r[:, 2] * r[:, 2]).astype(f32))).astype(f32)
        d = (r * inv[:, None]).astype(f32)
    return pix, o, d


def misses(lists, pix, o, d, cr, direct=(), chunk=20000):
    """Counts (ray, sphere) pairs that pass sphere_root's candidate rule — float64, widened: c < 0 or (disc > -1e-9 r^2 and h > 0) — and,
    of those, the pairs whose sphere is not on the list of the ray's group.  Direct spheres are tested for every ray: not counted."""
    cr = np.asarray(cr, f32).astype(np.float64)
    C, r2 = cr[:, :3], cr[:, 3] ** 2
    keep = np.ones(len(cr), bool)
    keep[list(direct)] = False
    hits = missed = 0
    for lo in range(0, len(pix), chunk):
        oo, dd, gg = o[lo:lo + chunk].astype(np.float64), d[lo:lo + chunk].astype(np.float64), pix[lo:lo + chunk] >> 6
        with np.errstate(all="ignore"):
            cc = C[None, :, :] - oo[:, None, :]
            hh = (cc * dd[:, None, :]).sum(2)
            c = (cc * cc).sum(2) - r2[None, :]
            cand = ((c < 0.0) | ((hh * hh - c > -1e-9 * r2[None, :]) & (hh > 0.0))) & keep[None, :]
        hits += int(cand.sum())
        missed += int((cand & ~lists[gg]).sum())
    return hits, missed


def length_stats(lists):
    n = lists.sum(1)
    return dict(groups=len(n), mean=round(float(n.mean()), 2), median=int(np.median(n)), p90=int(np.percentile(n, 90)), p99=int(np.percentile(n, 99)),
                max=int(n.max()), empty=round(float((n == 0).mean()), 3))


def main(argv):
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rt3 = importlib.import_module("raytracer-3_amd")
    w, h = (int(argv[1]), int(argv[2])) if len(argv) > 2 else (1920, 1080)
    n = int(argv[3]) if len(argv) > 3 else 400000
    cr, _ = rt3.scene_weekend(42)
    cam = rt3.weekend_camera(w, h).c
    p = params(w, h, lens_radius=0.05)
    direct = direct_list(cr)
    lists = build_lists(cam, p, cr, direct)
    print("bench scene %dx%d, %d spheres, direct spheres %s: list lengths %s" % (w, h, len(cr), direct, length_stats(lists)))
    pix, o, d = primary_rays(cam, p, n, np.random.default_rng(1))
    hits, missed = misses(lists, pix, o, d, cr, direct)
    print("%d random primary rays (a third at the extremes of jitter and lens): %d sphere candidates beside the direct spheres, %d outside their "
          "group's list" % (n, hits, missed))
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
