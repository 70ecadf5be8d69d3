#!/usr/bin/env python3
"""Display sequences (rt3_display_sequence_device) on ONE MI355X, filmic + sRGB at 1920x1080 and 3840x2160, beside
rt3_display_device on the same frame (the linear frame of a three-sphere render):
  display            rt3_display_device with a given gain (one launch: 16 bytes in and 4 out per pixel)
  display auto       ... with auto-exposure (the state's memset and three launches: 16 more bytes in)
  sequence adapt     rt3_display_sequence_device with auto-exposure, a device record as prev and out, no bloom: the same launches with
                     k_display_gain_step in k_display_gain's place — the adaptation should cost nothing
  sequence bloom 5   ... with a given gain and a bloom pyramid of five levels (2 * 5 launches)
  launch             rt3_display_device on a 1 x 1 frame: what one more launch in a call costs, back to back on a stream
Timing as tools/bench_display.py: HIP events on the calls' stream around BATCH back-to-back calls, the passes alternating inside every repetition,
best and median per call of REPS repetitions after a warm-up of every shape.  The bytes a pass must move are computed here from the shapes; for
the bloom the time's ratio over `display` is set beside the bytes' ratio, and the excess beside launches x the measured per-launch time.
GPU only: fails without a device.
Usage: python tools/bench_display_sequence.py [reps [batch]]     (one JSON line per measurement, then the comparison)"""
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
LEVELS = 5


def bloom_bytes(w, h, levels):
    """The bytes a call with a given gain and `levels` levels must move, and its launches: planes of 16 bytes a texel.
    k_bloom_down_first reads the frame and writes D_1; k_bloom_down reads D_{l-1} and writes D_l; k_bloom_up reads U_{l+1} and D_l and writes U_l;
    k_display_map_bloom reads the frame and U_1 and writes the words."""
    n = [w * h]
    for _ in range(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        n.append(w * h)
    total = 16 * n[0] + 16 * n[1]
    total += sum(16 * n[l - 1] + 16 * n[l] for l in range(2, levels + 1))
    total += sum(16 * n[l + 1] + 32 * n[l] for l in range(1, levels))
    total += 16 * n[0] + 16 * n[1] + 4 * n[0]
    return total, 2 * levels


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_display_sequence.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    r.set_spheres(*rt3.scene_three_spheres())
    s = torch.cuda.Stream()
    summary = {}
    for w, h in ((1920, 1080), (3840, 2160)):
        npix = w * h
        cam = rt3.Camera().update(w, h, 1.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0)
        p = rt3.make_params(w, h, spp=2, max_depth=4, seed=1)
        words = torch.empty(npix, dtype=torch.int32, device="cuda")
        lin = torch.empty(npix * 4, dtype=torch.float32, device="cuda")
        record = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.render_path_device(cam.c, p, words.data_ptr(), s.cuda_stream)              # the accumulation the resolve reads
        r.accum_resolve_device(lin.data_ptr(), s.cuda_stream)
        plain = rt3.display_params("filmic", "srgb")
        auto = rt3.display_params("filmic", "srgb", auto=True)
        adapt = rt3.display_sequence_params("filmic", "srgb", auto=True, adapt=(256, 64))
        bloom = rt3.display_sequence_params("filmic", "srgb", bloom=(LEVELS, 1.0, 0.25))
        b_bytes, b_launches = bloom_bytes(w, h, LEVELS)
        passes = [
            ("display", 20 * npix, 1, lambda: r.display_device(w, h, lin.data_ptr(), plain, words.data_ptr(), s.cuda_stream)),
            ("display auto", 36 * npix, 3, lambda: r.display_device(w, h, lin.data_ptr(), auto, words.data_ptr(), s.cuda_stream)),
            ("sequence adapt", 36 * npix, 3, lambda: r.display_sequence_device(w, h, lin.data_ptr(), adapt, record.data_ptr(), record.data_ptr(),
                                                                              words.data_ptr(), s.cuda_stream)),
            ("sequence bloom %d" % LEVELS, b_bytes, b_launches, lambda: r.display_sequence_device(w, h, lin.data_ptr(), bloom, 0, 0, words.data_ptr(),
                                                                                                 s.cuda_stream)),
            ("launch", 20, 1, lambda: r.display_device(1, 1, lin.data_ptr(), plain, words.data_ptr(), s.cuda_stream)),
        ]
        for _, _, _, fn in passes:                                                   # warm-up: code objects, the state's and the pyramid's allocation
            for _ in range(3):
                fn()
        s.synchronize()
        times = {name: [] for name, _, _, _ in passes}
        for _ in range(REPS):
            for name, _, _, fn in passes:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(BATCH):
                    fn()
                b.record(s)
                b.synchronize()
                times[name].append(a.elapsed_time(b) / BATCH)
        rows = {}
        for name, nbytes, launches, _ in passes:
            t = sorted(times[name])
            rows[name] = dict(frame="%dx%d" % (w, h), what=name, best_us=round(t[0] * 1e3, 2), median_us=round(t[len(t) // 2] * 1e3, 2),
                              worst_us=round(t[-1] * 1e3, 2), bytes=nbytes, launches=launches,
                              tb_per_s_at_best=round(nbytes / (t[0] * 1e-3) / 1e12, 3), reps=REPS, batch=BATCH)
            print(json.dumps(rows[name]), flush=True)
        level, frames = (int(v) for v in record.cpu().numpy().view(np.uint32)[:2])
        print(json.dumps(dict(frame="%dx%d" % (w, h), adapted_level=level, frames=frames)), flush=True)
        d, a, q, b, one = (rows[k] for k in ("display", "display auto", "sequence adapt", "sequence bloom %d" % LEVELS, "launch"))
        time_ratio, byte_ratio = b["median_us"] / d["median_us"], b_bytes / (20 * npix)
        summary["%dx%d" % (w, h)] = dict(
            adapt_minus_auto_us=round(q["median_us"] - a["median_us"], 2), auto_spread_us=round(a["worst_us"] - a["best_us"], 2),
            bloom_time_over_display=round(time_ratio, 3), bloom_bytes_over_display=round(byte_ratio, 3),
            bloom_excess_us=round(b["median_us"] - byte_ratio * d["median_us"], 2),
            launches_times_launch_us=round((b_launches - 1) * one["median_us"], 2))
    print(json.dumps(dict(comparison=summary)), flush=True)
    r.close()


if __name__ == "__main__":
    main()
