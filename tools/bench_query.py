#!/usr/bin/env python3
"""Batched ray queries (rt3_intersect_device / rt3_occluded_device) on ONE MI355X: Mrays/s and the filter work per ray on the three
benchmark scenes — weekend (484 spheres, k_trace_mfma32), rt3_scene_stress(100000) (resident three-level form) and rt3_scene_cornell(64) at config 5's
grid (47 106 faces) — for two kinds of ray: the 1920x1080 primary rays of the config's camera, and 2^21 incoherent rays (origins on the surfaces,
random unit directions).  Beside each primary-ray query: the Mode-X render of the same camera at spp 1, depth 1 (the same filter on the same rays).
Kernel time from the C ABI's HIP events (rt3_stats.trace_ms) after a warm-up, best and median of REPS runs.  GPU only: fails without a device.
Usage: python tools/bench_query.py [reps]     (one JSON line per measurement)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
W, H = 1920, 1080


def unit(rng, n):
    v = rng.normal(0.0, 1.0, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def primary_rays(cam):
    c = cam.c
    o, hor, ver, llc = (np.array(getattr(c, f), np.float32) for f in ("origin", "horizontal", "vertical", "lower_left_corner"))
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    u = (x / np.float32(W - 1)).reshape(-1, 1)
    v = ((np.float32(H - 1) - y) / np.float32(H - 1)).reshape(-1, 1)
    d = llc + u * hor + v * ver - o
    return rt3.make_rays(np.broadcast_to(o, d.shape), d)


def surface_rays(rng, n, spheres=None, faces=None, verts=None):
    if spheres is not None:
        s = spheres[rng.integers(0, len(spheres), n)]
        o = s[:, :3] + unit(rng, n) * s[:, 3:4] * np.float32(1.0001)
    else:
        f = faces[rng.integers(0, len(faces), n)]
        p = [verts[f[k], :3] for k in ("v1", "v2", "v3")]
        a, b = rng.random((n, 1)), rng.random((n, 1))
        flip = (a + b) > 1.0
        a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
        o = p[0] + a * (p[1] - p[0]) + b * (p[2] - p[0])
    return rt3.make_rays(o.astype(np.float32), unit(rng, n))


def timed(r, fn):
    fn()                                                              # warm-up: code objects, buffers, occupancy queries
    torch.cuda.synchronize()
    ms, st = [], None
    for _ in range(REPS):
        fn()
        st = r.stats()                                                # waits for the launch; HIP events around the trace kernel
        ms.append(st.trace_ms)
    return sorted(ms), st


def report(scene, what, n, ms, st):
    row = dict(scene=scene, what=what, rays=n, valid_rays=st.ray_casts, best_ms=round(ms[0], 3), median_ms=round(ms[len(ms) // 2], 3),
               mrays_per_s=round(n / ms[0] / 1e3, 1), filter_tests_per_ray=round(st.filter_tests / max(1, st.ray_casts), 2),
               exact_tests_per_ray=round(st.exact_tests / max(1, st.ray_casts), 2), bound_tests_per_ray=round(st.bound_tests / max(1, st.ray_casts), 2),
               launches=st.launches)
    print(json.dumps(row), flush=True)
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_query.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    rng = np.random.default_rng(2026)
    empty_sph = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    scenes = []
    cr, m = rt3.scene_weekend(42)
    scenes.append(("weekend 484 spheres", dict(spheres=(cr, m)), rt3.weekend_camera(W, H), dict(spheres=cr)))
    cr, m = rt3.scene_stress(100000, 43)
    scenes.append(("stress 100000 spheres", dict(spheres=(cr, m)),
                   rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0), dict(spheres=cr)))
    f, v, fm = rt3.scene_cornell(64)
    scenes.append(("cornell 47106 faces", dict(mesh=(f, v, fm)), rt3.Camera().update(W, H, 2.0, 2.0, 2.0), dict(faces=f, verts=v)))
    ratios = {}
    for name, up, cam, prims in scenes:
        r.set_mesh(*(up["mesh"] if "mesh" in up else empty_mesh))
        r.set_spheres(*(up["spheres"] if "spheres" in up else empty_sph))
        p = rt3.make_params(W, H, spp=1, max_depth=1, seed=1, flags=1)
        ms_r, st_r = timed(r, lambda: r.render_path(cam.c, p))
        rend = report(name, "mode-X render spp 1 depth 1", W * H, ms_r, st_r)
        for kind, rays in (("primary", primary_rays(cam)), ("incoherent", surface_rays(rng, 1 << 21, **prims))):
            dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
            for q in ("nearest", "occluded"):
                fn = (lambda: r.intersect(dev)) if q == "nearest" else (lambda: r.occluded(dev))
                ms, st = timed(r, fn)
                row = report(name, "%s %s" % (q, kind), len(rays), ms, st)
                if kind == "primary":
                    ratios["%s / %s" % (name, q)] = round(row["best_ms"] / rend["best_ms"], 3)
    print(json.dumps(dict(query_over_render_trace_ms=ratios)), flush=True)


if __name__ == "__main__":
    main()
