#!/usr/bin/env python3
"""Adaptive sampling on the MI355X (rt3_render_path_adaptive): what the list form costs and what the rule saves.

    python tools/bench_adaptive.py [--width 1920 --height 1080 --budget 256 --reference-spp 4096 --reps 5] > profiles/adaptive_bench_mi355x.log

Two scenes at the given frame size: the weekend scene (484 spheres, k_trace_mfma32, strip lists in round 0) and 100 000 spheres (the resident
three-level kernel).  Times are device times of the whole call (rt3_stats::total_ms: HIP events around the first and the last launch, so the
waits for the per-round read-back are inside), after a warm-up, variants alternated in one process, medians of --reps.

  overhead   adaptive with threshold 1e-30 (no pixel with any variance ever leaves) against rt3_render_path of the same spp: the price of the
             rounds, the read-backs, the list indirection and — weekend scene — of primary rays that miss the strip lists after round 0
  benefit    thresholds 0.1 / 0.05 / 0.02: share of the uniform sample count, time against the uniform render of the budget, and the MSE of the
             linear frame against a --reference-spp frame of rt3_render_path, beside a uniform render of the same total sample count (rounded up)
"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime per process, see raytracer-3_amd/__init__.py)

rt3 = importlib.import_module("raytracer-3_amd")


def scenes(w, h):
    cr, mats = rt3.scene_weekend(42)
    yield "weekend (484 spheres, k_trace_mfma32)", cr, mats, rt3.weekend_camera(w, h).c, dict(max_depth=50, seed=1, flags=1, lens_radius=0.05)
    cr, mats = rt3.scene_stress(100000, 43)
    cam = rt3.Camera().look_at(w, h, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)
    yield "stress100k (100 000 spheres, resident three-level kernel)", cr, mats, cam.c, dict(max_depth=50, seed=1, flags=1)


def mse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float((d * d).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step-spp", type=int, default=16)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    w, h = a.width, a.height
    r = rt3.initialize_renderer(0)
    print("adaptive sampling, %dx%d, budget %d spp, min %d, step %d, dark 0.01; device %s; times: rt3_stats.total_ms, median of %d after a warm-up"
          % (w, h, a.budget, a.min_spp, a.step_spp, torch.cuda.get_device_name(0), a.reps))
    for name, cr, mats, cam, kw in scenes(w, h):
        r.set_spheres(cr, mats)
        p = rt3.make_params(w, h, spp=a.budget, **kw)
        print("\n== %s" % name)

        def uniform(params):
            r.render_path(cam, params)
            return r.stats()

        def adaptive(threshold):
            _, counts = r.render_adaptive(cam, p, threshold=threshold, min_spp=a.min_spp, step_spp=a.step_spp, dark=0.01)
            return r.stats(), counts

        # -- overhead of the list form: nothing leaves
        uniform(p); adaptive(1e-30)                                    # warm-up of both
        tu, ta = [], []
        for _ in range(a.reps):
            tu.append(uniform(p).total_ms)
            st, counts = adaptive(1e-30)
            ta.append(st.total_ms)
        mu, ma = statistics.median(tu), statistics.median(ta)
        print("overhead: uniform %d spp %.2f ms (min %.2f max %.2f) | adaptive, threshold 1e-30: %.2f ms (min %.2f max %.2f), %d launches, "
              "share of samples %.4f | ratio adaptive / uniform %.3f"
              % (a.budget, mu, min(tu), max(tu), ma, min(ta), max(ta), st.launches, counts.sum(dtype=np.uint64) / (float(w) * h * a.budget), ma / mu))

        # -- benefit
        r.render_path(cam, rt3.make_params(w, h, spp=a.reference_spp, **kw))
        reference = r.accum_resolve(p)
        r.render_path(cam, p)
        print("benefit: uniform %d spp: %.2f ms, MSE against %d spp %.3e" % (a.budget, mu, a.reference_spp, mse(r.accum_resolve(p), reference)))
        for threshold in (0.1, 0.05, 0.02):
            st, counts = adaptive(threshold)
            frame = r.accum_resolve(p)
            total = int(counts.sum(dtype=np.uint64))
            equal = max(1, -(-total // (w * h)))                       # the uniform render of the same sample count, rounded up
            pe = rt3.make_params(w, h, spp=equal, **kw)
            uniform(pe)
            frame_e = r.accum_resolve(pe)
            t_a, t_e = [], []
            for _ in range(a.reps):
                t_a.append(adaptive(threshold)[0].total_ms)
                t_e.append(uniform(pe).total_ms)
            levels, per_level = np.unique(counts, return_counts=True)
            print("threshold %-5g share of samples %.3f | %.2f ms = %.3f of uniform %d spp | MSE %.3e | uniform %d spp (same samples): %.2f ms, MSE %.3e | "
                  "launches %d | pixels at min %.3f, at budget %.3f"
                  % (threshold, total / (float(w) * h * a.budget), statistics.median(t_a), statistics.median(t_a) / mu, a.budget, mse(frame, reference),
                     equal, statistics.median(t_e), mse(frame_e, reference), st.launches,
                     per_level[levels == a.min_spp].sum() / float(w * h), per_level[levels == a.budget].sum() / float(w * h)))
    r.close()


if __name__ == "__main__":
    main()
