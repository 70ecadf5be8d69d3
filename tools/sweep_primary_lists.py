#!/usr/bin/env python3
"""Sweep of RT3_PRIMARY_LIST_MAX (the longest strip list a restock of k_trace_mfma32 still traces itself) on the bench scene, in ONE
process, the settings interleaved round by round: kernel time by HIP events, frames compared with lists off.
    python tools/sweep_primary_lists.py [width height spp [rounds]]      (default 1920 1080 64 5; lists are long at 400 225)"""
import importlib, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
rt3 = importlib.import_module("raytracer-3_amd")
W, H, spp = (int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1920, 1080, 64)
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
SETTINGS = ["off", "0", "4", "8", "16", "24", "32", "64", "512", "default"]
r = rt3.HipRenderer()
cr, mats = rt3.scene_weekend(42)
cam = rt3.weekend_camera(W, H)
r.set_spheres(cr, mats)
p = rt3.make_params(W, H, spp=spp, max_depth=50, seed=1, flags=1, lens_radius=0.05)
times, frames, stats = {s: [] for s in SETTINGS}, {}, {}
for i in range(rounds + 1):
    for s in SETTINGS:
        os.environ.pop("RT3_PRIMARY_LISTS", None)
        os.environ.pop("RT3_PRIMARY_LIST_MAX", None)
        if s == "off":
            os.environ["RT3_PRIMARY_LISTS"] = "0"
        elif s != "default":
            os.environ["RT3_PRIMARY_LIST_MAX"] = s
        frames[s] = r.render_path(cam.c, p)
        st = r.stats()
        stats[s] = (st.ray_casts, st.filter_tests // len(cr), st.mfma_instructions, st.exact_tests)
        if i:
            times[s].append(st.trace_ms)
base = statistics.median(times["off"])
print("%dx%d, %d spp, %d rounds; lists off: %.3f ms" % (W, H, spp, rounds, base))
for s in SETTINGS:
    t = times[s]
    print("RT3_PRIMARY_LIST_MAX %-7s median %8.3f ms  x%.4f  (min %.3f max %.3f)  identical %s  casts %d, through the filter %d, mfma %d, exact tests %d"
          % (s, statistics.median(t), statistics.median(t) / base, min(t), max(t), np.array_equal(frames[s], frames["off"]), *stats[s]))
