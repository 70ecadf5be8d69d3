#!/usr/bin/env python3
"""Radiance along caller-supplied rays (rt3_radiance_device) on ONE MI355X, on the three benchmark scenes — weekend (484 spheres,
k_trace_mfma32), rt3_scene_stress(100000) (resident three-level form) and rt3_scene_cornell(64) (47 106 faces):
  (a) the 1920x1080 camera rays of the scene's camera (sample 0 of rt3_camera_rays_device) at SPP samples per ray, depth DEPTH, beside the Mode-X render of
      the same camera, spp and depth in the same process, alternated: trace_ms of each and the ratio.  Same number of paths, the same materials and
      depth; what differs is the ray source (a 32-byte load instead of start_path) and, on the <= 512-sphere scene, the render's strip lists and ray stock.
  (b) 2^21 incoherent rays (origins on the surfaces, random unit directions), one sample, depth 8: Mrays/s and Mcasts/s.
Kernel time from the C ABI's HIP events (rt3_stats.trace_ms, summed over the call's batches) after a warm-up: median, min and max of REPS runs.
GPU only: fails without a device.
Usage: python tools/bench_radiance.py [reps] [spp] [depth]     (one JSON line per measurement)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SPP = int(sys.argv[2]) if len(sys.argv) > 2 else 4
DEPTH = int(sys.argv[3]) if len(sys.argv) > 3 else 8
W, H = 1920, 1080


def unit(rng, n):
    v = rng.normal(0.0, 1.0, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


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


def alternated(r, fns):
    """Every function once as a warm-up, then REPS rounds of all of them in turn: sorted trace_ms and the last stats of each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms, st = [[] for _ in fns], [None] * len(fns)
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            fn()
            st[k] = r.stats()                                         # waits for the call; HIP events around its trace launches
            ms[k].append(st[k].trace_ms)
    return [sorted(m) for m in ms], st


def report(scene, what, paths, ms, st):
    med = ms[len(ms) // 2]
    row = dict(scene=scene, what=what, paths=paths, ray_casts=st.ray_casts, median_ms=round(med, 3), min_ms=round(ms[0], 3), max_ms=round(ms[-1], 3),
               mpaths_per_s=round(paths / med / 1e3, 1), mcasts_per_s=round(st.ray_casts / med / 1e3, 1),
               filter_tests_per_cast=round(st.filter_tests / max(1, st.ray_casts), 2), launches=st.launches)
    print(json.dumps(row), flush=True)
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_radiance.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    rng = np.random.default_rng(2026)
    empty_sph = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    scenes = []
    cr, m = rt3.scene_weekend(42)
    scenes.append(("weekend 484 spheres", dict(spheres=(cr, m)), rt3.weekend_camera(W, H), dict(spheres=cr), 0.05, 1))
    cr, m = rt3.scene_stress(100000, 43)
    scenes.append(("stress 100000 spheres", dict(spheres=(cr, m)),
                   rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0), dict(spheres=cr), 0.0, 1))
    f, v, fm = rt3.scene_cornell(64)
    scenes.append(("cornell 47106 faces", dict(mesh=(f, v, fm)), rt3.Camera().update(W, H, 2.0, 2.0, 2.0), dict(faces=f, verts=v), 0.0, 3))
    ratios = {}
    for name, up, cam, prims, lens, flags in scenes:
        r.set_mesh(*(up["mesh"] if "mesh" in up else empty_mesh))
        r.set_spheres(*(up["spheres"] if "spheres" in up else empty_sph))
        p = rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1, flags=flags, lens_radius=lens)
        rays = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
        r.camera_rays_device(cam.c, p, 0, 1, rays.data_ptr(), torch.cuda.current_stream().cuda_stream)
        frame = torch.empty(W * H, dtype=torch.int32, device="cuda")
        render = lambda: r.render_path_device(cam.c, p, frame.data_ptr(), torch.cuda.current_stream().cuda_stream)   # noqa: E731
        rad = lambda: r.radiance(rays, samples=SPP, max_depth=DEPTH, seed=1, flags=flags & 2)                            # noqa: E731
        (ms_r, ms_q), (st_r, st_q) = alternated(r, [render, rad])
        a = report(name, "mode-X render, %d spp, depth %d" % (SPP, DEPTH), W * H * SPP, ms_r, st_r)
        b = report(name, "radiance of the camera rays, %d samples, depth %d" % (SPP, DEPTH), W * H * SPP, ms_q, st_q)
        ratios[name] = round(b["median_ms"] / a["median_ms"], 3)
        inc = surface_rays(rng, 1 << 21, **prims)
        dev = torch.from_numpy(inc.view(np.float32).reshape(-1, 8).copy()).cuda()
        (ms_i,), (st_i,) = alternated(r, [lambda: r.radiance(dev, samples=1, max_depth=8, seed=1, flags=flags & 2)])
        report(name, "radiance of 2^21 incoherent rays, 1 sample, depth 8", len(inc), ms_i, st_i)
    print(json.dumps(dict(radiance_over_render_trace_ms=ratios)), flush=True)


if __name__ == "__main__":
    main()
