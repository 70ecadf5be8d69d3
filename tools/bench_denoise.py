#!/usr/bin/env python3
"""The denoiser (rt3_denoise_device) on ONE MI355X, at 1920x1080, 4 spp, 5 passes, on cornell(64) (the command line's
cornell view) and weekend.  In the same run and the same way it times the 4-spp render (rt3_render_path_device), the linear resolve
(rt3_accum_resolve_device) and the AOV pass (rt3_render_aov_device) that feed it: device events around each call on the current torch stream,
WARMUP untimed calls, then REPS timed ones; median, min and max in ms.  Bytes per pass come from the shapes (below), and the quality line gives
the MSE of the raw and the denoised frame against a REF_SPP frame of the same camera.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a separate run.  GPU only: fails without a device.
Usage: python tools/bench_denoise.py [reps] [warmup]     (one JSON line per measurement)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H, SPP, PASSES, REF_SPP = 1920, 1080, 4, 5, 1024
HBM_PEAK, FP32_PEAK = 8.0e12, 157.3e12          # MI355X spec peaks (bytes/s, FLOP/s)

# Bytes each kernel must move at least (every plane read and written once), per pixel.
#   prepare: colour 16 + the first 32 bytes of the AOV record + il 16 + guide 16 + gz 4
#   moments / a pass: (I, v) 16 + guide 16 + gz 4 in, 16 out; the last pass also reads the albedo (16)
# And what the taps of one pass load (mostly from L1 / L2): 3x3 blur and 5x5 taps, 32 bytes each (guide + (I, v)), + gz.
COMPULSORY = dict(prepare=84, moments=52, atrous=52, atrous_last=68)
TAP_BYTES_PER_PASS = (9 + 25) * 32 + 4
# FLOPs counted from the source (one per add / mul / div / sqrt / max; dn_exp as its 20 operations), per pixel at P = 128 (7 squarings):
# w_g of a pair 36 (w_n 12, e_z 5, exp 20 with the product); a pass: 8 blur taps of 39, 24 taps of 64 (w_g's parts, e_l 8, weight 2, sums 11),
# centre and finish 19; the moments: 48 taps of 41 (w_g + 5 sums), finish 5; prepare: 20.
FLOPS_PER_PASS = 8 * 39 + 24 * 64 + 19
FLOPS_MOMENTS, FLOPS_PREPARE = 48 * 41 + 5, 20


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    empty_sph = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    scenes = [("cornell(64)", rt3.scene_cornell(64), None, rt3.main_camera(W, H), 0.0, rt3.FLAG_BLACK_BACKGROUND),
              ("weekend", None, rt3.scene_weekend(42), rt3.weekend_camera(W, H), 0.05, 0)]
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")
    lin = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    aov = torch.empty((H, W, 12), dtype=torch.float32, device="cuda")
    npix = W * H
    for name, mesh, sph, cam, lens, flags in scenes:
        r.set_mesh(*(mesh if mesh is not None else empty_mesh))
        r.set_spheres(*(sph if sph is not None else empty_sph))
        p = rt3.make_params(W, H, spp=SPP, max_depth=50, seed=1, flags=flags, lens_radius=lens)
        rows = [("render %d spp" % SPP, lambda: r.render_path_device(cam.c, p, frame.data_ptr(), stream)),
                ("accum_resolve", lambda: r.accum_resolve_device(lin.data_ptr(), stream)),
                ("render_aov %d spp" % SPP, lambda: r.render_aov_device(cam.c, p, aov.data_ptr(), stream))]
        for what, fn in rows:
            print(json.dumps(dict(scene=name, what=what, **timed(fn))), flush=True)
        r.render_path_device(cam.c, p, frame.data_ptr(), stream)
        r.accum_resolve_device(lin.data_ptr(), stream)
        r.render_aov_device(cam.c, p, aov.data_ptr(), stream)
        t = timed(lambda: r.denoise(lin, aov, iterations=PASSES))
        per_pass_ms = t["median_ms"] / PASSES
        compulsory = npix * (COMPULSORY["prepare"] + COMPULSORY["moments"] + (PASSES - 1) * COMPULSORY["atrous"] + COMPULSORY["atrous_last"])
        flops = npix * (FLOPS_PREPARE + FLOPS_MOMENTS + PASSES * FLOPS_PER_PASS)
        floor_s = max(compulsory / HBM_PEAK, flops / FP32_PEAK)
        print(json.dumps(dict(scene=name, what="denoise %d passes" % PASSES, **t, per_pass_ms=round(per_pass_ms, 4),
                              compulsory_bytes_per_pass=npix * COMPULSORY["atrous"], tap_bytes_per_pass=npix * TAP_BYTES_PER_PASS,
                              compulsory_bytes_call=compulsory, counted_flops_call=flops,
                              bound="bandwidth" if compulsory / HBM_PEAK >= flops / FP32_PEAK else "compute",
                              share_of_peak=round(floor_s / (t["median_ms"] * 1e-3), 4),
                              tap_bytes_per_s=round(npix * TAP_BYTES_PER_PASS * PASSES / (t["median_ms"] * 1e-3) / 1e12, 2))), flush=True)
        # quality: raw and denoised against a REF_SPP frame (another seed) of the same camera
        raw = lin.cpu().numpy()
        den = r.denoise(lin, aov, iterations=PASSES).cpu().numpy()
        q = rt3.make_params(W, H, spp=REF_SPP, max_depth=50, seed=2, flags=flags, lens_radius=lens)
        r.render_path(cam.c, q)
        ref = r.accum_resolve(q)
        mse_raw = float(np.mean((raw[..., :3].astype(np.float64) - ref[..., :3]) ** 2))
        mse_den = float(np.mean((den[..., :3].astype(np.float64) - ref[..., :3]) ** 2))
        print(json.dumps(dict(scene=name, what="quality vs %d spp" % REF_SPP, mse_raw=mse_raw, mse_denoised=mse_den,
                              mse_ratio=round(mse_raw / mse_den, 2))), flush=True)


if __name__ == "__main__":
    main()
