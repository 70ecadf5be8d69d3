#!/usr/bin/env python3
"""First-hit AOVs (rt3_render_aov_device) on ONE MI355X: the AOV call's device time beside the Mode-X render of the same
params at depth 1 (rt3_render_path_device, max_depth 1: the same primary rays through the same filter), at 1920x1080, spp 1 and 16, on the three
benchmark scenes — weekend (484 spheres, k_trace_mfma32), rt3_scene_stress(100000) (resident three-level form) and rt3_scene_cornell(64).
Per call: total_ms (first to last launch of the call, HIP events: for the AOV pass camera rays + query + accumulation per batch, then the resolve)
and trace_ms (the trace / query launches alone), best and median of REPS runs after a warm-up.  GPU only: fails without a device.
Usage: python tools/bench_aov.py [reps]     (one JSON line per measurement, then the ratios)"""
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


def timed(r, fn):
    fn()                                                              # warm-up: code objects, buffers, occupancy queries
    torch.cuda.synchronize()
    tot, tr, st = [], [], None
    for _ in range(REPS):
        fn()
        st = r.stats()                                                # waits for the call; HIP events on its stream
        tot.append(st.total_ms)
        tr.append(st.trace_ms)
    return sorted(tot), sorted(tr), st


def report(scene, what, spp, tot, tr, st):
    row = dict(scene=scene, what=what, spp=spp, best_total_ms=round(tot[0], 3), median_total_ms=round(tot[len(tot) // 2], 3),
               best_trace_ms=round(tr[0], 3), ray_casts=st.ray_casts, samples=st.samples, launches=st.launches,
               msamples_per_s=round(W * H * spp / tot[0] / 1e3, 1))
    print(json.dumps(row), flush=True)
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_aov.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    empty_sph = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    scenes = []
    cr, m = rt3.scene_weekend(42)
    scenes.append(("weekend 484 spheres", None, (cr, m), rt3.weekend_camera(W, H), 0.05))
    cr, m = rt3.scene_stress(100000, 43)
    scenes.append(("stress 100000 spheres", None, (cr, m),
                   rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0), 0.0))
    f, v, fm = rt3.scene_cornell(64)
    scenes.append(("cornell 47106 faces", (f, v, fm), None, rt3.Camera().update(W, H, 2.0, 2.0, 2.0), 0.0))
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")
    aov = torch.empty(W * H * 12, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ratios = {}
    for name, mesh, sph, cam, lens in scenes:
        r.set_mesh(*(mesh if mesh is not None else empty_mesh))
        r.set_spheres(*(sph if sph is not None else empty_sph))
        for spp in (1, 16):
            p = rt3.make_params(W, H, spp=spp, max_depth=1, seed=1, lens_radius=lens)
            a = report(name, "render depth 1", spp, *timed(r, lambda: r.render_path_device(cam.c, p, frame.data_ptr(), stream)))
            b = report(name, "aov", spp, *timed(r, lambda: r.render_aov_device(cam.c, p, aov.data_ptr(), stream)))
            ratios["%s / spp %d" % (name, spp)] = dict(total=round(b["best_total_ms"] / a["best_total_ms"], 3),
                                                       trace=round(b["best_trace_ms"] / a["best_trace_ms"], 3))
    print(json.dumps(dict(aov_over_depth1_render=ratios)), flush=True)


if __name__ == "__main__":
    main()
