#!/usr/bin/env python3
"""The motion plane and the denoiser that reads it (rt3_motion_device, rt3_denoise_temporal_motion_device) on ONE
MI355X at 1920x1080, 5 passes: device events around each call on the current torch stream, WARMUP untimed calls, then REPS timed ones; median,
min and max in ms.  Weekend with every sphere of odd index moved between the two frames, cornell(64) with a third of its vertices displaced:
rt3_motion alone, then the motion-aware call and rt3_denoise_temporal of the same frame alternated in one process (two rounds each).  Then
what re-uploading a moved scene costs per frame on the host (rt3_set_spheres: the filter rows are rebuilt; wall clock, weekend and 100 000
spheres), as a number.  The quality lines run the 8-frame sequence of tests/test_gpu_motion.py (two Lambert spheres moving 0.1 units per
frame, 320x240, 1 spp per frame): MSE of rt3_denoise, the camera-only temporal call and the motion-aware call of the last frame against a
REF_SPP frame, over the pixels that show a mover and over the frame.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`
in a separate run.  GPU only: fails without a device.
Usage: python tools/bench_motion.py [reps] [warmup] [--no-quality]     (one JSON line per measurement)"""
import importlib
import json
import os
import sys
import time

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
F = np.float32


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


def slid(cr, k, step=(0.1, 0.02, -0.05)):
    out = cr.copy()
    out[1::2, :3] += (F(k) * np.array(step, F)).astype(F)
    return out


# the scene of tests/test_gpu_motion.py's quality floor
Q_SPHERES = np.array([[0.0, -1000.5, -4.0, 1000.0], [-1.2, 0.0, -4.0, 0.5], [0.0, 0.0, -4.5, 0.5], [1.2, 0.0, -4.0, 0.5],
                      [-0.6, -0.2, -3.0, 0.3], [0.9, -0.2, -3.0, 0.3]], F)
Q_RGB = [(0.5, 0.5, 0.5), (0.8, 0.2, 0.2), (0.2, 0.7, 0.3), (0.2, 0.3, 0.8), (0.8, 0.7, 0.2), (0.7, 0.3, 0.7)]
Q_STEPS = {4: (0.1, 0.0, 0.0), 5: (-0.04, 0.09, 0.0)}


def q_spheres(k):
    cr = Q_SPHERES.copy()
    for i, step in Q_STEPS.items():
        cr[i, :3] += (F(k) * np.array(step, F)).astype(F)
    return cr


def quality(r, w, h, frames=8):
    mats = np.zeros(len(Q_RGB), rt3.MATERIAL)
    mats["rgb"], mats["kind"] = Q_RGB, rt3.MAT_LAMBERT
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    cam = rt3.main_camera(w, h)
    prev_m = prev_c = None
    for k in range(frames):
        r.set_spheres(q_spheres(k), mats)
        p = rt3.make_params(w, h, spp=1, max_depth=50, seed=200 + k)
        r.render_path(cam.c, p)
        lin, aov = r.accum_resolve(p), r.render_aov(cam.c, p)
        plane = r.motion(aov, cam.c, prev_center_radius=q_spheres(k - 1)) if k else None
        out_m, prev_m = r.denoise_temporal(lin, aov, cam.c, prev_m, motion=plane)
        out_c, prev_c = r.denoise_temporal(lin, aov, cam.c, prev_c)
    spatial = r.denoise(lin, aov)
    q = rt3.make_params(w, h, spp=REF_SPP, max_depth=50, seed=7)
    r.render_path(cam.c, q)
    ref = r.accum_resolve(q)
    mask = plane[..., 3] != 0
    res = dict(what="quality, two Lambert spheres moving 0.1 per frame, %dx%d, frame %d, 1 spp, vs %d spp" % (w, h, frames, REF_SPP),
               mover_pixels=int(mask.sum()),
               history_share_movers_motion=round(float((prev_m[0]["length"][mask] >= frames).mean()), 4),
               history_share_movers_camera_only=round(float((prev_c[0]["length"][mask] >= frames).mean()), 4))
    for name, img in (("spatial", spatial), ("camera_only", out_c), ("motion", out_m)):
        res["mse_movers_" + name], res["mse_frame_" + name] = mse(img[mask], ref[mask]), mse(img, ref)
    res["ratio_movers_camera_only_over_motion"] = round(res["mse_movers_camera_only"] / res["mse_movers_motion"], 3)
    res["ratio_frame_camera_only_over_motion"] = round(res["mse_frame_camera_only"] / res["mse_frame_motion"], 3)
    return res


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    empty_sph = (np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    cr, mats = rt3.scene_weekend(42)
    faces, verts, fmats = rt3.scene_cornell(64)
    moved_verts = verts.copy()
    third = len(verts) // 3 // 3 * 3
    moved_verts[third:2 * third, :3] += np.random.default_rng(1).normal(0.0, 0.02, (third, 3)).astype(F)
    # (name, the two frames' (mesh, spheres), the cameras, lens, flags, the previous arrays of frame 1)
    scenes = [("weekend, odd spheres moved", [(None, (cr, mats)), (None, (slid(cr, 1), mats))], [orbit_camera(W, H, 0.0), orbit_camera(W, H, 1.0)],
               0.05, 0, dict(prev_center_radius=torch.from_numpy(cr).cuda())),
              ("cornell(64), a third of the vertices moved", [((faces, verts, fmats), None), ((faces, moved_verts, fmats), None)],
               [rt3.main_camera(W, H)] * 2, 0.0, rt3.FLAG_BLACK_BACKGROUND, dict(prev_vertices=torch.from_numpy(verts).cuda()))]
    stream = torch.cuda.current_stream().cuda_stream
    lin = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    aov = torch.empty((H, W, 12), dtype=torch.float32, device="cuda")
    for name, frames, cams, lens, flags, prev_arrays in scenes:
        prev = None
        for k, ((mesh, sph), cam) in enumerate(zip(frames, cams)):
            r.set_mesh(*(mesh if mesh is not None else empty_mesh))
            r.set_spheres(*(sph if sph is not None else empty_sph))
            p = rt3.make_params(W, H, spp=SPP, max_depth=50, seed=1 + k, flags=flags, lens_radius=lens)
            r.render_path_device(cam.c, p, torch.empty(W * H, dtype=torch.int32, device="cuda").data_ptr(), stream)
            r.accum_resolve_device(lin.data_ptr(), stream)
            r.render_aov_device(cam.c, p, aov.data_ptr(), stream)
            if k == 0:
                _, prev = r.denoise_temporal(lin, aov, cam.c, None, iterations=PASSES)
        plane = r.motion(aov, cam.c, **prev_arrays)
        moved = plane[..., 3] != 0
        _, with_m = r.denoise_temporal(lin, aov, cam.c, prev, iterations=PASSES, motion=plane)
        _, without = r.denoise_temporal(lin, aov, cam.c, prev, iterations=PASSES)
        shares = dict(moved_share=round(float(moved.float().mean().item()), 4),
                      history_share_moved_motion=round(float((with_m[0][..., 3][moved] == 2).float().mean().item()), 4),
                      history_share_moved_camera_only=round(float((without[0][..., 3][moved] == 2).float().mean().item()), 4))
        print(json.dumps(dict(scene=name, what="motion", **shares, **timed(lambda: r.motion(aov, cam.c, **prev_arrays)))), flush=True)
        for rnd in (1, 2):                                             # alternated in one process
            print(json.dumps(dict(scene=name, what="denoise_temporal %d passes, motion plane, round %d" % (PASSES, rnd),
                                  **timed(lambda: r.denoise_temporal(lin, aov, cam.c, prev, iterations=PASSES, motion=plane)))), flush=True)
            print(json.dumps(dict(scene=name, what="denoise_temporal %d passes, camera only, round %d" % (PASSES, rnd),
                                  **timed(lambda: r.denoise_temporal(lin, aov, cam.c, prev, iterations=PASSES)))), flush=True)
    # what moving the spheres costs on the host per frame: rt3_set_spheres rebuilds the filter rows (wall clock, median of 5)
    r.set_mesh(*empty_mesh)
    for name, (c, m) in (("weekend (%d spheres)" % len(cr), (cr, mats)), ("stress (100000 spheres)", rt3.scene_stress(100000, 43))):
        ts = []
        for k in range(5):
            moved_c = slid(c, k + 1)
            t0 = time.perf_counter()
            r.set_spheres(moved_c, m)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        print(json.dumps(dict(scene=name, what="rt3_set_spheres of the moved scene, host wall clock", median_ms=round(ts[2], 3),
                              min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3), reps=5)), flush=True)
    if QUALITY:
        print(json.dumps(quality(r, 320, 240)), flush=True)


if __name__ == "__main__":
    main()
