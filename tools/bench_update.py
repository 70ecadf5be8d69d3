#!/usr/bin/env python3
"""Scene updates (rt3_update_spheres*, rt3_update_mesh*) on ONE MI355X against the full upload they replace.

  update vs set      per scene (weekend 484 spheres, 100 000 and 10^6 spheres, cornell(64) = 47 106 faces): the host wall clock of a full
                     upload (rt3_set_spheres / rt3_set_mesh) of the moved scene, the host wall clock of the update of the same arrays followed
                     by a synchronise (host form), the device time of the device-form update alone (events on the torch stream), and the
                     device time of one 1-spp 1920x1080 frame of that scene for scale.  Full uploads and updates alternate in one process.
  rows               the device-form update with the fused lane-parallel row kernel (k_refit_rows, three launches) and with the five
                     k_group_bounds / k_group_frags launches the full upload uses (RT3_REFIT_SIMPLE=1), alternated.  Per-kernel times:
                     run this under `rocprofv3 --kernel-trace --stats`, in a run of its own, with --rows-only.
  cost of the order  100 000 spheres, the odd ones sliding: the 1-spp frame time after k updates against the frame time after a fresh full
                     upload of the same frame, k = 1, 8, 64 (when to re-upload).
GPU only: fails without a device.
Usage: python tools/bench_update.py [reps] [warmup] [--rows-only] [--no-million]     (one JSON line per measurement)"""
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
WARMUP = int(ARGS[1]) if len(ARGS) > 1 else 3
W, H = 1920, 1080
F = np.float32


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=len(ms))


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def device(fn, reps=None):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps or REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def slid(cr, k, step=(0.1, 0.02, -0.05)):
    out = cr.copy()
    out[1::2, :3] += (F(k) * np.array(step, F)).astype(F)
    return out


def frame_ms(r, cam, flags, seed=1):
    """Device time of one 1-spp frame (rt3_stats.total_ms), median of five."""
    out = torch.empty(W * H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for k in range(6):
        r.render_path_device(cam.c, rt3.make_params(W, H, spp=1, max_depth=50, seed=seed + k, flags=flags), out.data_ptr(), stream)
        ms.append(r.stats().total_ms)
    return round(sorted(ms[1:])[2], 4)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_update.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    empty_sph = (np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    stress_cam = rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)
    sphere_scenes = [("weekend 484 spheres", rt3.scene_weekend(42), rt3.weekend_camera(W, H), 20),
                     ("stress 100000 spheres", rt3.scene_stress(100000, 43), stress_cam, 8)]
    if "--no-million" not in sys.argv:
        sphere_scenes.append(("stress 1000000 spheres", rt3.scene_stress(1000000, 45), stress_cam, 3))
    rows_only = "--rows-only" in sys.argv

    def ab_rows(name, fn):
        for rnd in (1, 2):                                             # alternated in one process
            os.environ.pop("RT3_REFIT_SIMPLE", None)
            print(json.dumps(dict(scene=name, what="device update, k_refit_rows (3 launches), round %d" % rnd, **device(fn))), flush=True)
            os.environ["RT3_REFIT_SIMPLE"] = "1"
            print(json.dumps(dict(scene=name, what="device update, k_group_bounds / k_group_frags (5 launches), round %d" % rnd, **device(fn))),
                  flush=True)
            os.environ.pop("RT3_REFIT_SIMPLE", None)

    r.set_mesh(*empty_mesh)
    for name, (cr, mats), cam, reps in sphere_scenes:
        moved = [slid(cr, k) for k in (1, 2)]
        dev = [torch.from_numpy(m).cuda() for m in moved]
        r.set_spheres(cr, mats)
        flip = [0]

        def dev_update():
            flip[0] ^= 1
            r.update_spheres(dev[flip[0]])
        if not rows_only:
            res = dict(scene=name)
            for rnd in (1, 2):                                         # full upload and update alternated
                res["set_spheres_wall_round%d" % rnd] = wall(lambda: r.set_spheres(moved[rnd - 1], mats), reps)
                res["update_spheres_wall_round%d" % rnd] = wall(lambda: r.update_spheres(moved[rnd % 2]), reps)
            res["update_spheres_device"] = device(dev_update)
            res["frame_1spp_ms"] = frame_ms(r, cam, 0)
            res["set_over_update_wall"] = round(res["set_spheres_wall_round2"]["median_ms"] / res["update_spheres_wall_round2"]["median_ms"], 2)
            res["frame_over_update_device"] = round(res["frame_1spp_ms"] / res["update_spheres_device"]["median_ms"], 2)
            print(json.dumps(res), flush=True)
        ab_rows(name, dev_update)

    faces, verts, fmats = rt3.scene_cornell(64)
    name = "cornell(64) %d faces" % len(faces)
    moved = []
    for seed in (1, 2):
        v = verts.copy()
        third = len(v) // 3 // 3 * 3
        v[third:2 * third, :3] += np.random.default_rng(seed).normal(0.0, 0.02, (third, 3)).astype(F)
        moved.append(v)
    dev = [torch.from_numpy(m).cuda() for m in moved]
    r.set_spheres(*empty_sph)
    r.set_mesh(faces, verts, fmats)
    flip = [0]

    def dev_update_mesh():
        flip[0] ^= 1
        r.update_mesh(dev[flip[0]])
    if not rows_only:
        res = dict(scene=name)
        for rnd in (1, 2):
            res["set_mesh_wall_round%d" % rnd] = wall(lambda: r.set_mesh(faces, moved[rnd - 1], fmats), 8)
            res["update_mesh_wall_round%d" % rnd] = wall(lambda: r.update_mesh(moved[rnd % 2]), 8)
        res["update_mesh_device"] = device(dev_update_mesh)
        res["frame_1spp_ms"] = frame_ms(r, rt3.Camera().update(W, H, 2.0, 2.0, 2.0), rt3.FLAG_BLACK_BACKGROUND)
        res["set_over_update_wall"] = round(res["set_mesh_wall_round2"]["median_ms"] / res["update_mesh_wall_round2"]["median_ms"], 2)
        res["frame_over_update_device"] = round(res["frame_1spp_ms"] / res["update_mesh_device"]["median_ms"], 2)
        print(json.dumps(res), flush=True)
    ab_rows(name, dev_update_mesh)
    if rows_only:
        return

    # the cost of keeping the order: frame k after k updates against frame k after a fresh full upload
    r.set_mesh(*empty_mesh)
    cr, mats = rt3.scene_stress(100000, 43)
    fresh = rt3.initialize_renderer(0)
    fresh.set_mesh(*empty_mesh)
    r.set_spheres(cr, mats)
    done = 0
    for k in (1, 8, 64):
        while done < k:
            done += 1
            r.update_spheres(slid(cr, done))
        fresh.set_spheres(slid(cr, k), mats)
        a, b = frame_ms(r, stress_cam, 0, seed=100), frame_ms(fresh, stress_cam, 0, seed=100)
        print(json.dumps(dict(scene="stress 100000 spheres, odd spheres slid k x (0.1, 0.02, -0.05)", what="1-spp frame after k updates vs after a full upload",
                              k=k, frame_ms_after_updates=a, frame_ms_after_full_upload=b, ratio=round(a / b, 3))), flush=True)
    fresh.close()


if __name__ == "__main__":
    main()
