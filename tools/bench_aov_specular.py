#!/usr/bin/env python3
"""Specular-chain AOVs (rt3_render_aov_specular_device) on ONE MI355X, at 1920x1080, 4 spp.

1. Device time of the chain call with max_bounces 4 and 8 beside rt3_render_aov_device, on weekend, rt3_scene_stress(100000) and
   rt3_scene_cornell(64), for both forms of the bounce loop: the early exit through a one-word read-back per bounce (the default) and every round
   queued without a host wait (RT3_AOV_CHAIN_NO_WAIT=1).  total_ms: first to last launch of the call (HIP events on its stream, rt3_get_stats), so
   the host's round trips of the first form are inside it; best and median of REPS calls after WARMUP untimed ones.
2. Per bounce, without the early exit: the time max_bounces = k adds over k - 1, and the share of the items still running after k bounces
   (the valid rays query k + 1 traces: ray_casts(k) - ray_casts(k - 1)).
3. What the guides are for: rt3_denoise of a 4-spp frame guided by first-hit AOVs and by chain AOVs (max_bounces 8; max_fuzz 0 and 1), MSE against a
   REF_SPP frame of another seed (tools/bench_denoise.py's protocol), over the whole frame and over the pixels whose first hit is a followed
   material; on weekend and on a Cornell box whose two blocks are a mirror and a block of glass.
GPU only: fails without a device.  Usage: python tools/bench_aov_specular.py [reps] [warmup] [ref_spp]     (one JSON line per measurement)"""
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
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
REF_SPP = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
W, H, SPP, PASSES = 1920, 1080, 4, 5
EMPTY_SPH = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
EMPTY_MESH = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))


def timed(r, fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    tot, tr, st = [], [], None
    for _ in range(REPS):
        fn()
        st = r.stats()                                                # waits for the call; HIP events on its stream
        tot.append(st.total_ms)
        tr.append(st.trace_ms)
    tot.sort(); tr.sort()
    return dict(best_total_ms=round(tot[0], 3), median_total_ms=round(tot[len(tot) // 2], 3), max_total_ms=round(tot[-1], 3),
                median_trace_ms=round(tr[len(tr) // 2], 3), ray_casts=st.ray_casts, launches=st.launches, reps=REPS, warmup=WARMUP)


def set_scene(r, mesh, sph):
    r.set_mesh(*(mesh if mesh is not None else EMPTY_MESH))
    r.set_spheres(*(sph if sph is not None else EMPTY_SPH))


def cornell_mirror_glass(grid=64):
    """rt3_scene_cornell with its first block a fuzz-0 mirror and its second a block of glass (the blocks: the Lambert faces behind the five walls)."""
    f, v, fm = rt3.scene_cornell(grid)
    fm = fm.copy()
    blocks = np.nonzero((np.arange(len(fm)) >= 10 * grid * grid) & (fm["kind"] == rt3.MAT_LAMBERT))[0]
    a, b = blocks[:len(blocks) // 2], blocks[len(blocks) // 2:]
    fm["kind"][a], fm["rgb"][a], fm["param"][a] = rt3.MAT_METAL, (0.9, 0.9, 0.9), 0.0
    fm["kind"][b], fm["param"][b] = rt3.MAT_DIELECTRIC, 1.5
    return f, v, fm


def timing(r):
    aov = torch.empty(W * H * 12, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    scenes = [("weekend 484 spheres", None, rt3.scene_weekend(42), rt3.weekend_camera(W, H), 0.05),
              ("stress 100000 spheres", None, rt3.scene_stress(100000, 43),
               rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0), 0.0),
              ("cornell 47106 faces", rt3.scene_cornell(64), None, rt3.Camera().update(W, H, 2.0, 2.0, 2.0), 0.0)]
    items = W * H * SPP
    for name, mesh, sph, cam, lens in scenes:
        set_scene(r, mesh, sph)
        p = rt3.make_params(W, H, spp=SPP, max_depth=1, seed=1, lens_radius=lens)
        print(json.dumps(dict(scene=name, what="render_aov", **timed(r, lambda: r.render_aov_device(cam.c, p, aov.data_ptr(), stream)))), flush=True)
        for wait in (True, False):
            os.environ["RT3_AOV_CHAIN_NO_WAIT"] = "0" if wait else "1"
            for mb in (4, 8):
                t = timed(r, lambda: r.render_aov_specular_device(cam.c, p, aov.data_ptr(), stream, max_bounces=mb, max_fuzz=0.0))
                print(json.dumps(dict(scene=name, what="render_aov_specular", loop="early exit" if wait else "no host wait", max_bounces=mb, **t)),
                      flush=True)
        os.environ["RT3_AOV_CHAIN_NO_WAIT"] = "1"                     # per bounce: every round runs, so round k's cost is a difference
        prev = None
        for mb in range(0, 9):
            t = timed(r, lambda: r.render_aov_specular_device(cam.c, p, aov.data_ptr(), stream, max_bounces=mb, max_fuzz=0.0))
            row = dict(scene=name, what="per bounce", max_bounces=mb, median_total_ms=t["median_total_ms"], ray_casts=t["ray_casts"])
            if prev is not None:
                row.update(added_ms=round(t["median_total_ms"] - prev["median_total_ms"], 3),
                           alive_share=round((t["ray_casts"] - prev["ray_casts"]) / items, 5))
            print(json.dumps(row), flush=True)
            prev = t
        os.environ["RT3_AOV_CHAIN_NO_WAIT"] = "0"


def quality(r):
    scenes = [("weekend", None, rt3.scene_weekend(42), rt3.weekend_camera(W, H), 0.05, 0),
              ("cornell(64), mirror and glass blocks", cornell_mirror_glass(64), None, rt3.main_camera(W, H), 0.0, rt3.FLAG_BLACK_BACKGROUND)]
    for name, mesh, sph, cam, lens, flags in scenes:
        set_scene(r, mesh, sph)
        mats = (sph[1] if sph is not None else mesh[2])
        p = rt3.make_params(W, H, spp=SPP, max_depth=50, seed=1, flags=flags, lens_radius=lens)
        r.render_path(cam.c, p)
        lin = r.accum_resolve(p)
        first = r.render_aov(cam.c, p)
        q = rt3.make_params(W, H, spp=REF_SPP, max_depth=50, seed=2, flags=flags, lens_radius=lens)
        r.render_path(cam.c, q)
        ref = r.accum_resolve(q)[..., :3].astype(np.float64)
        lin_t = torch.from_numpy(lin).cuda()

        def mse(frame, mask=None):
            e = ((frame[..., :3].astype(np.float64) - ref) ** 2).mean(axis=-1)
            return float(e.mean() if mask is None else e[mask].mean())

        def denoised(guides):
            g = torch.from_numpy(np.ascontiguousarray(guides).view(np.float32).reshape(H, W, 12)).cuda()
            return r.denoise(lin_t, g, iterations=PASSES).cpu().numpy()

        hit = (first["kind"] == rt3.HIT_SPHERE) | (first["kind"] == rt3.HIT_FACE)
        idx = np.where(hit, first["index"], 0)
        for max_fuzz in (0.0, 1.0):
            followed = hit & ((mats["kind"][idx] == rt3.MAT_DIELECTRIC) | ((mats["kind"][idx] == rt3.MAT_METAL) & (mats["param"][idx] <= max_fuzz)))
            chain = r.render_aov_specular(cam.c, p, max_bounces=8, max_fuzz=max_fuzz)
            d_first, d_chain = denoised(first), denoised(chain)
            row = dict(scene=name, what="denoise %d spp vs %d spp" % (SPP, REF_SPP), max_bounces=8, max_fuzz=max_fuzz,
                       specular_first_hit_share=round(float(followed.mean()), 4),
                       mse_raw=mse(lin), mse_first_hit_guides=mse(d_first), mse_chain_guides=mse(d_chain),
                       specular_mse_raw=mse(lin, followed), specular_mse_first_hit_guides=mse(d_first, followed),
                       specular_mse_chain_guides=mse(d_chain, followed),
                       rest_mse_first_hit_guides=mse(d_first, ~followed), rest_mse_chain_guides=mse(d_chain, ~followed))
            print(json.dumps(row), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_aov_specular.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    timing(r)
    quality(r)


if __name__ == "__main__":
    main()
