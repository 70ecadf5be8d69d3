#!/usr/bin/env python3
"""rt3_set_spheres_device / rt3_set_mesh_device on ONE MI355X against the host upload they replace.

  per scene          weekend 484 spheres, stress 100 000 and 10^6 spheres (--no-million skips it), cornell(64) = 47 106 faces.  Alternated
                     in one process, medians:
                       host_form_wall      the host wall clock of the host form from numpy arrays (rt3_set_spheres / rt3_set_mesh)
                       device_form_wall    the host wall clock of the device form plus a synchronise, from tensors already on the device
                       cpu_then_host_wall  the host wall clock of .cpu() plus the host form: what a caller who has tensors pays today
                       device_form_device  the device time of the device form alone, by events on the torch stream (it includes the
                                           call's one wait)
                     and the ratios host form / device form, cpu + host form / device form.
  the frame          the 1-spp 1920x1080 frame time and the three filter counters per ray cast after each form (the device form leaves the
                     order of a regroup, the host form the host's split).
GPU only: fails without a device.
Usage: python tools/bench_set_device.py [reps] [warmup] [--no-million]     (one JSON line per scene)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_update as BU  # noqa: E402   (stats / wall / device / frame_ms: the same instruments)
from bench_regroup import frame_and_counters  # noqa: E402

rt3 = BU.rt3
F = np.float32
W, H = BU.W, BU.H


def records(a):
    """A numpy array of records as a tensor on the device (structured records as bytes)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def host_copy(t, dtype):
    """The tensor back on the host, as the numpy array the host form takes."""
    a = t.cpu().numpy()
    return a.view(dtype).reshape(-1) if dtype is not None else a


def measure(name, reps, host_form, device_form, cpu_then_host, r, cam, flags):
    res = dict(scene=name)
    sync = torch.cuda.synchronize

    def device_and_sync():
        device_form()
        sync()
    for fn in (host_form, device_and_sync, cpu_then_host):                # warm-up: the scratch, the regroup plan, the allocator
        fn()
    for rnd in (1, 2):                                                    # the three forms alternated
        res["host_form_wall_round%d" % rnd] = BU.wall(host_form, reps)
        res["device_form_wall_round%d" % rnd] = BU.wall(device_and_sync, reps)
        res["cpu_then_host_wall_round%d" % rnd] = BU.wall(cpu_then_host, reps)
    res["device_form_device"] = BU.device(device_form, reps)
    dev_ms = res["device_form_wall_round2"]["median_ms"]
    res["host_over_device_wall"] = round(res["host_form_wall_round2"]["median_ms"] / dev_ms, 2)
    res["cpu_then_host_over_device_wall"] = round(res["cpu_then_host_wall_round2"]["median_ms"] / dev_ms, 2)
    host_form()
    res["frame_after_host_form"] = frame_and_counters(r, cam, flags)
    device_and_sync()
    res["frame_after_device_form"] = frame_and_counters(r, cam, flags)
    res["frame_device_over_host"] = round(res["frame_after_device_form"]["frame_ms"] / res["frame_after_host_form"]["frame_ms"], 3)
    print(json.dumps(res), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_set_device.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    empty_sph = (np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    stress_cam = rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)
    sphere_scenes = [("weekend 484 spheres", rt3.scene_weekend(42), 20, rt3.weekend_camera(W, H)),
                     ("stress 100000 spheres", rt3.scene_stress(100000, 43), 8, stress_cam)]
    if "--no-million" not in sys.argv:
        sphere_scenes.append(("stress 1000000 spheres", rt3.scene_stress(1000000, 45), 3, stress_cam))
    r.set_mesh(*empty_mesh)
    for name, (cr, mats), reps, cam in sphere_scenes:
        t_cr, t_mats = records(cr), records(mats)
        measure(name, reps, lambda: r.set_spheres(cr, mats), lambda: r.set_spheres(t_cr, t_mats),
                lambda: r.set_spheres(host_copy(t_cr, None), host_copy(t_mats, rt3.MATERIAL)), r, cam, 0)

    faces, verts, fmats = rt3.scene_cornell(64)
    t_f, t_v, t_m = records(faces), records(verts), records(fmats)
    r.set_spheres(*empty_sph)
    measure("cornell(64) %d faces" % len(faces), 8, lambda: r.set_mesh(faces, verts, fmats), lambda: r.set_mesh(t_f, t_v, t_m),
            lambda: r.set_mesh(host_copy(t_f, rt3.GFACE), host_copy(t_v, None), host_copy(t_m, rt3.MATERIAL)), r, rt3.main_camera(W, H),
            rt3.FLAG_BLACK_BACKGROUND)
    r.close()


if __name__ == "__main__":
    main()
