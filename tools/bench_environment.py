#!/usr/bin/env python3
"""Environment-map lighting (rt3_set_environment*) on ONE MI355X: what the map's lookup costs a Mode-X render.  The three benchmark
scenes — weekend (484 spheres, k_trace_mfma32 with strip lists), rt3_scene_stress(100000) (the resident three-level form) and rt3_scene_cornell(64)
(47 106 faces) — at 1920x1080, SPP samples, depth DEPTH, rendered with a random N = 512 map (25 MB, four 16-byte loads per miss) and, the same scene, camera
and parameters, with no map (the sky), alternated in one process: trace_ms of each and the ratio.  The paths are the same in both — a map changes no ray —
so the ratio is the miss branch alone.  Kernel time from the C ABI's HIP events (rt3_stats.trace_ms) after a warm-up: median, min and max of REPS rounds.
GPU only: fails without a device.
Usage: python tools/bench_environment.py [reps] [spp] [depth] [n_face]     (one JSON line per measurement)"""
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
SPP = int(sys.argv[2]) if len(sys.argv) > 2 else 16
DEPTH = int(sys.argv[3]) if len(sys.argv) > 3 else 8
N_FACE = int(sys.argv[4]) if len(sys.argv) > 4 else 512
W, H = 1920, 1080


def report(scene, what, ms, st):
    med = ms[len(ms) // 2]
    row = dict(scene=scene, what=what, paths=W * H * SPP, ray_casts=st.ray_casts, median_ms=round(med, 3), min_ms=round(ms[0], 3), max_ms=round(ms[-1], 3),
               mcasts_per_s=round(st.ray_casts / med / 1e3, 1), launches=st.launches)
    print(json.dumps(row), flush=True)
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_environment.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    cube = torch.from_numpy(np.random.default_rng(2026).uniform(0.0, 2.0, (6, N_FACE, N_FACE, 4)).astype(np.float32)).cuda()
    empty_sph = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    scenes = []
    cr, m = rt3.scene_weekend(42)
    scenes.append(("weekend 484 spheres", dict(spheres=(cr, m)), rt3.weekend_camera(W, H), 0.05))
    cr, m = rt3.scene_stress(100000, 43)
    scenes.append(("stress 100000 spheres", dict(spheres=(cr, m)), rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0), 0.0))
    f, v, fm = rt3.scene_cornell(64)
    scenes.append(("cornell 47106 faces", dict(mesh=(f, v, fm)), rt3.Camera().update(W, H, 2.0, 2.0, 2.0), 0.0))
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ratios = {}
    for name, up, cam, lens in scenes:
        r.set_mesh(*(up["mesh"] if "mesh" in up else empty_mesh))
        r.set_spheres(*(up["spheres"] if "spheres" in up else empty_sph))
        p = rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1, flags=rt3.FLAG_GAMMA2, lens_radius=lens)
        ms, st = {"sky": [], "map": []}, {}

        def render(which):
            if which == "map":
                r.set_environment(cube)
            else:
                r.clear_environment()
            r.render_path_device(cam.c, p, frame.data_ptr(), stream)
            return r.stats()                                          # waits for the call; HIP events around its trace launches
        for which in ("sky", "map"):                                  # warm-up
            render(which)
        for _ in range(REPS):
            for which in ("sky", "map"):
                st[which] = render(which)
                ms[which].append(st[which].trace_ms)
        assert st["sky"].ray_casts == st["map"].ray_casts             # a map changes no path
        a = report(name, "mode-X render, sky, %d spp, depth %d" % (SPP, DEPTH), sorted(ms["sky"]), st["sky"])
        b = report(name, "mode-X render, N = %d map, %d spp, depth %d" % (N_FACE, SPP, DEPTH), sorted(ms["map"]), st["map"])
        ratios[name] = round(b["median_ms"] / a["median_ms"], 4)
    r.clear_environment()
    print(json.dumps(dict(map_over_sky_trace_ms=ratios)), flush=True)


if __name__ == "__main__":
    main()
