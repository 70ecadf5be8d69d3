#!/usr/bin/env python3
"""The display transform (rt3_display_device) on ONE MI355X: the device form without auto-exposure (one launch: 16 bytes in
and 4 out per pixel) and with it (the state's memset and three launches: 16 more bytes in), beside rt3_accum_resolve_device on the same frame (an
existing pass with the same input traffic: 16 bytes in, 16 out), at 1920x1080 and 3840x2160.  The frame is the linear frame of a three-sphere
render.  Timing: HIP events on the calls' stream around BATCH back-to-back calls (a single call is a few microseconds: the window has to be longer
than the clock's grain), the three passes alternating inside every repetition, best and median per call of REPS repetitions after a warm-up of
every shape.  Bytes per second are the bytes the pass has to move (computed here from the shape) over that time.  GPU only: fails without a device.
Usage: python tools/bench_display.py [reps [batch]]     (one JSON line per measurement, then the ratios)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
BATCH = int(sys.argv[2]) if len(sys.argv) > 2 else 50


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_display.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    r.set_spheres(*rt3.scene_three_spheres())
    s = torch.cuda.Stream()
    ratios = {}
    for w, h in ((1920, 1080), (3840, 2160)):
        npix = w * h
        cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
        p = rt3.make_params(w, h, spp=2, max_depth=4, seed=1)
        words = torch.empty(npix, dtype=torch.int32, device="cuda")
        lin = torch.empty(npix * 4, dtype=torch.float32, device="cuda")
        scratch = torch.empty(npix * 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render_path_device(cam.c, p, words.data_ptr(), s.cuda_stream)              # the accumulation the resolve reads
        r.accum_resolve_device(lin.data_ptr(), s.cuda_stream)
        plain = rt3.display_params("filmic", "srgb")
        auto = rt3.display_params("filmic", "srgb", auto=True)
        passes = [
            ("accum_resolve", 32, lambda: r.accum_resolve_device(scratch.data_ptr(), s.cuda_stream)),
            ("display filmic,srgb", 20, lambda: r.display_device(w, h, lin.data_ptr(), plain, words.data_ptr(), s.cuda_stream)),
            ("display filmic,srgb,auto", 36, lambda: r.display_device(w, h, lin.data_ptr(), auto, words.data_ptr(), s.cuda_stream)),
        ]
        for _, _, fn in passes:                                                      # warm-up: code objects, the state's allocation
            for _ in range(3):
                fn()
        s.synchronize()
        times = {name: [] for name, _, _ in passes}
        for _ in range(REPS):
            for name, _, fn in passes:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(BATCH):
                    fn()
                b.record(s)
                b.synchronize()
                times[name].append(a.elapsed_time(b) / BATCH)
        rows = {}
        for name, bytes_per_pixel, _ in passes:
            t = sorted(times[name])
            rows[name] = dict(frame="%dx%d" % (w, h), what=name, best_us=round(t[0] * 1e3, 2), median_us=round(t[len(t) // 2] * 1e3, 2),
                              worst_us=round(t[-1] * 1e3, 2), bytes_per_pixel=bytes_per_pixel,
                              tb_per_s_at_best=round(npix * bytes_per_pixel / (t[0] * 1e-3) / 1e12, 3), reps=REPS, batch=BATCH)
            print(json.dumps(rows[name]), flush=True)
        hist, dark, gain = r.display_state()
        print(json.dumps(dict(frame="%dx%d" % (w, h), counted=int(hist.sum()), dark=dark, gain=float(gain))), flush=True)
        base = rows["accum_resolve"]["median_us"]
        ratios["%dx%d" % (w, h)] = dict(plain_over_resolve=round(rows["display filmic,srgb"]["median_us"] / base, 3),
                                        auto_over_resolve=round(rows["display filmic,srgb,auto"]["median_us"] / base, 3))
    print(json.dumps(dict(median_ratios=ratios)), flush=True)
    r.close()


if __name__ == "__main__":
    main()
