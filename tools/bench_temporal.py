#!/usr/bin/env python3
"""The temporal denoiser (rt3_denoise_temporal_device) on ONE MI355X at 1920x1080, 5 passes, on weekend and
cornell(64), beside rt3_denoise of the same frame: device events around each call on the current torch stream, WARMUP untimed calls, then
REPS timed ones; median, min and max in ms.  The temporal call is timed with a history (the previous frame of a 1-degree orbit for weekend, the
same camera for cornell).  The quality lines run the 8-frame weekend orbit of
tests/test_gpu_temporal.py (320x240, 1 spp per frame) and the same at 1920x1080: MSE of the raw frame, rt3_denoise and the temporal output of
the last frame against a REF_SPP frame of its camera.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats` in a separate run.
GPU only: fails without a device.
Usage: python tools/bench_temporal.py [reps] [warmup] [--no-quality]     (one JSON line per measurement)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(ARGS[0]) if len(ARGS) > 0 else 20
WARMUP = int(ARGS[1]) if len(ARGS) > 1 else 5
QUALITY = "--no-quality" not in sys.argv
W, H, SPP, PASSES, REF_SPP = 1920, 1080, 4, 5, 1024


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=REPS, warmup=WARMUP)


def orbit_camera(w, h, deg):
    a = np.radians(deg)
    return rt3.Camera().look_at(w, h, (13.0 * np.cos(a) + 3.0 * np.sin(a), 2.0, 3.0 * np.cos(a) - 13.0 * np.sin(a)), (0.0, 0.0, 0.0),
                                vfov=20.0, focus_dist=10.0)


def mse(a, b):
    return float(np.mean((a[..., :3].astype(np.float64) - b[..., :3]) ** 2))


def quality(r, w, h, frames=8):
    """The last frame of a `frames`-frame weekend orbit (1 degree per frame, 1 spp, seed 100 + k) against a REF_SPP frame (seed 7)."""
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    r.set_spheres(*rt3.scene_weekend(42))
    prev = None
    for k in range(frames):
        cam = orbit_camera(w, h, float(k))
        p = rt3.make_params(w, h, spp=1, max_depth=50, seed=100 + k, lens_radius=0.05)
        r.render_path(cam.c, p)
        lin, aov = r.accum_resolve(p), r.render_aov(cam.c, p)
        out, prev = r.denoise_temporal(lin, aov, cam.c, prev)
    spatial = r.denoise(lin, aov)
    q = rt3.make_params(w, h, spp=REF_SPP, max_depth=50, seed=7, lens_radius=0.05)
    r.render_path(cam.c, q)
    ref = r.accum_resolve(q)
    m = dict(raw=mse(lin, ref), spatial=mse(spatial, ref), temporal=mse(out, ref))
    return dict(what="quality weekend orbit %dx%d, frame %d, 1 spp, vs %d spp" % (w, h, frames, REF_SPP), mse_raw=m["raw"],
                mse_spatial=m["spatial"], mse_temporal=m["temporal"], ratio_spatial_over_temporal=round(m["spatial"] / m["temporal"], 3),
                ratio_raw_over_temporal=round(m["raw"] / m["temporal"], 3))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_temporal.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    empty_sph = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    scenes = [("weekend", None, rt3.scene_weekend(42), [orbit_camera(W, H, 0.0), orbit_camera(W, H, 1.0)], 0.05, 0),
              ("cornell(64)", rt3.scene_cornell(64), None, [rt3.main_camera(W, H)] * 2, 0.0, rt3.FLAG_BLACK_BACKGROUND)]
    stream = torch.cuda.current_stream().cuda_stream
    lin = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    aov = torch.empty((H, W, 12), dtype=torch.float32, device="cuda")
    for name, mesh, sph, cams, lens, flags in scenes:
        r.set_mesh(*(mesh if mesh is not None else empty_mesh))
        r.set_spheres(*(sph if sph is not None else empty_sph))
        prev = None
        for k, cam in enumerate(cams):
            p = rt3.make_params(W, H, spp=SPP, max_depth=50, seed=1 + k, flags=flags, lens_radius=lens)
            r.render_path_device(cam.c, p, torch.empty(W * H, dtype=torch.int32, device="cuda").data_ptr(), stream)
            r.accum_resolve_device(lin.data_ptr(), stream)
            r.render_aov_device(cam.c, p, aov.data_ptr(), stream)
            if k == 0:
                _, prev = r.denoise_temporal(lin, aov, cam.c, None, iterations=PASSES)
        print(json.dumps(dict(scene=name, what="denoise %d passes" % PASSES, **timed(lambda: r.denoise(lin, aov, iterations=PASSES)))),
              flush=True)
        print(json.dumps(dict(scene=name, what="denoise_temporal %d passes, no history" % PASSES,
                              **timed(lambda: r.denoise_temporal(lin, aov, cam.c, None, iterations=PASSES)))), flush=True)
        out, nxt = r.denoise_temporal(lin, aov, cam.c, prev, iterations=PASSES)
        share = float((nxt[0][..., 3] == 2).float().mean().item())
        print(json.dumps(dict(scene=name, what="denoise_temporal %d passes, with history" % PASSES, history_share=round(share, 4),
                              **timed(lambda: r.denoise_temporal(lin, aov, cam.c, prev, iterations=PASSES)))), flush=True)
    if QUALITY:
        for w, h in ((320, 240), (1920, 1080)):
            print(json.dumps(quality(r, w, h)), flush=True)


if __name__ == "__main__":
    main()
