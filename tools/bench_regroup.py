#!/usr/bin/env python3
"""rt3_regroup*  on ONE MI355X against the full upload it replaces.

  regroup vs set     per scene (weekend 484 spheres, 100 000 and 10^6 spheres, cornell(64) = 47 106 faces): the host wall clock of a full
                     upload (rt3_set_spheres / rt3_set_mesh) of the moved scene, the host wall clock of a refit of the same arrays, the
                     host wall clock of rt3_regroup (queue + synchronise), and the device time of rt3_regroup_device alone (events on the
                     torch stream).  Full uploads, refits and regroups alternate in one process; medians.
  per kernel         run this under `rocprofv3 --kernel-trace --stats`, in a run of its own, with --kernels-only: device-form refits and
                     regroups of the 100 000-sphere scene only.
  the drift          100 000 spheres, the odd ones sliding by (0.1, 0.02, -0.05) per frame: the 1-spp 1920x1080 frame time and the three
                     filter counters per ray cast after k = 8 and k = 64 refits, in three states: as is, after rt3_regroup, and after a
                     full upload of the same positions.
GPU only: fails without a device.
Usage: python tools/bench_regroup.py [reps] [warmup] [--kernels-only] [--no-million]     (one JSON line per measurement)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_update as BU  # noqa: E402   (stats / wall / device / slid / frame_ms: the same instruments)

rt3 = BU.rt3
F = np.float32
W, H = BU.W, BU.H


def frame_and_counters(r, cam, flags, seed=100):
    ms = BU.frame_ms(r, cam, flags, seed=seed)
    st = r.stats()
    casts = max(st.ray_casts, 1)
    return dict(frame_ms=ms, filter_tests_per_cast=round(st.filter_tests / casts, 3), bound_tests_per_cast=round(st.bound_tests / casts, 3),
                exact_tests_per_cast=round(st.exact_tests / casts, 3))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_regroup.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    L = rt3.lib()
    empty_sph = (np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    stress_cam = rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)
    kernels_only = "--kernels-only" in sys.argv
    sphere_scenes = [("stress 100000 spheres", rt3.scene_stress(100000, 43), 8)]
    if not kernels_only:
        sphere_scenes.insert(0, ("weekend 484 spheres", rt3.scene_weekend(42), 20))
        if "--no-million" not in sys.argv:
            sphere_scenes.append(("stress 1000000 spheres", rt3.scene_stress(1000000, 45), 3))

    def regroup_device(what):
        import ctypes as C
        stream = torch.cuda.current_stream().cuda_stream
        r._check(L.rt3_regroup_device(r._ctx, what, C.c_void_p(stream)))

    r.set_mesh(*empty_mesh)
    for name, (cr, mats), reps in sphere_scenes:
        moved = [BU.slid(cr, k) for k in (8, 16)]
        dev = [torch.from_numpy(m).cuda() for m in moved]
        r.set_spheres(cr, mats)
        flip = [0]

        def refit_then_regroup():
            flip[0] ^= 1
            r.update_spheres(dev[flip[0]])
            regroup_device(rt3.REGROUP_SPHERES)

        def refit_only():
            flip[0] ^= 1
            r.update_spheres(dev[flip[0]])
        if kernels_only:
            BU.device(refit_then_regroup)
            continue
        res = dict(scene=name)
        for rnd in (1, 2):                                             # full upload, refit and regroup alternated
            res["set_spheres_wall_round%d" % rnd] = BU.wall(lambda: r.set_spheres(moved[rnd - 1], mats), reps)
            ts = []
            for _ in range(reps):
                r.update_spheres(moved[rnd % 2])                       # (host form: the regroup has something to do every time)
                ts.append(BU.wall(lambda: L.rt3_regroup(r._ctx, rt3.REGROUP_SPHERES), 1)["median_ms"])
            res["regroup_wall_round%d" % rnd] = BU.stats(ts)
            res["update_spheres_wall_round%d" % rnd] = BU.wall(lambda: r.update_spheres(moved[rnd % 2]), reps)
        both, alone = BU.device(refit_then_regroup), BU.device(refit_only)
        res["refit_and_regroup_device"] = both
        res["refit_device"] = alone
        res["regroup_device_ms"] = round(both["median_ms"] - alone["median_ms"], 4)
        res["set_over_regroup_wall"] = round(res["set_spheres_wall_round2"]["median_ms"] / res["regroup_wall_round2"]["median_ms"], 2)
        print(json.dumps(res), flush=True)
    if kernels_only:
        torch.cuda.synchronize()
        return

    faces, verts, fmats = rt3.scene_cornell(64)
    name = "cornell(64) %d faces" % len(faces)
    moved = []
    for seed in (1, 2):
        v = verts.copy()
        v[:, :3] += np.random.default_rng(seed).normal(0.0, 0.02, (len(v), 3)).astype(F)
        moved.append(v)
    dev = [torch.from_numpy(m).cuda() for m in moved]
    r.set_spheres(*empty_sph)
    r.set_mesh(faces, verts, fmats)
    flip = [0]

    def mesh_refit_then_regroup():
        flip[0] ^= 1
        r.update_mesh(dev[flip[0]])
        regroup_device(rt3.REGROUP_MESH)

    def mesh_refit_only():
        flip[0] ^= 1
        r.update_mesh(dev[flip[0]])
    res = dict(scene=name)
    for rnd in (1, 2):
        res["set_mesh_wall_round%d" % rnd] = BU.wall(lambda: r.set_mesh(faces, moved[rnd - 1], fmats), 8)
        ts = []
        for _ in range(8):
            r.update_mesh(moved[rnd % 2])
            ts.append(BU.wall(lambda: L.rt3_regroup(r._ctx, rt3.REGROUP_MESH), 1)["median_ms"])
        res["regroup_wall_round%d" % rnd] = BU.stats(ts)
        res["update_mesh_wall_round%d" % rnd] = BU.wall(lambda: r.update_mesh(moved[rnd % 2]), 8)
    both, alone = BU.device(mesh_refit_then_regroup), BU.device(mesh_refit_only)
    res["refit_and_regroup_device"] = both
    res["refit_device"] = alone
    res["regroup_device_ms"] = round(both["median_ms"] - alone["median_ms"], 4)
    res["set_over_regroup_wall"] = round(res["set_mesh_wall_round2"]["median_ms"] / res["regroup_wall_round2"]["median_ms"], 2)
    print(json.dumps(res), flush=True)

    # the drift: frame k after k refits as is, after a regroup, and after a fresh full upload of the same positions
    r.set_mesh(*empty_mesh)
    cr, mats = rt3.scene_stress(100000, 43)
    fresh = rt3.initialize_renderer(0)
    fresh.set_mesh(*empty_mesh)
    r.set_spheres(cr, mats)
    done = 0
    for k in (8, 64):
        while done < k:
            done += 1
            r.update_spheres(BU.slid(cr, done))
        as_is = frame_and_counters(r, stress_cam, 0)
        r._check(L.rt3_regroup(r._ctx, rt3.REGROUP_SPHERES))
        regrouped = frame_and_counters(r, stress_cam, 0)
        fresh.set_spheres(BU.slid(cr, k), mats)
        full = frame_and_counters(fresh, stress_cam, 0)
        print(json.dumps(dict(scene="stress 100000 spheres, odd spheres slid k x (0.1, 0.02, -0.05)", what="1-spp frame after k refits: as is / after rt3_regroup / after a full upload",
                              k=k, as_is=as_is, after_regroup=regrouped, after_full_upload=full,
                              as_is_over_full=round(as_is["frame_ms"] / full["frame_ms"], 3),
                              regroup_over_full=round(regrouped["frame_ms"] / full["frame_ms"], 3))), flush=True)
        r.set_spheres(cr, mats)                                        # (k = 64 starts from the sorted order again, as the first measurement did)
        done = 0
    fresh.close()


if __name__ == "__main__":
    main()
