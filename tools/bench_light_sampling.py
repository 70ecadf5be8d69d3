#!/usr/bin/env python3
"""Importance sampling of the emissive primitives (RT3_FLAG_LIGHT_SAMPLING) on ONE MI355X: what the shadow rays cost and what they buy.
Time: weekend with every seventh small sphere made a lamp (484 spheres, k_trace_mfma32), rt3_scene_cornell(64) (47 106 faces, its own light; black
background) and rt3_scene_stress(100000) with every thousandth sphere made a lamp (the resident three-level form), at 1920x1080, SPP samples, depth
DEPTH, rendered with and without the flag, alternated in one process: trace_ms and ray_casts of each, the ratio, and the time of the table build (the
first flagged call after a scene upload against the second, whole-call wall time with a device synchronisation).
Noise: the same three scenes at 480x270: the mean squared error of the linear frame against a plain REF_SPP-spp frame, at equal samples and at (about)
equal time — the plain render gets time_ratio times the samples.  One scene has ONE LARGE emitter (the box's light, a quad the bounces find by
themselves): where the flag loses there, the figures say so.  Also the variance ratio of the test suite's small-lamp scene.
GPU only: fails without a device.
Usage: python tools/bench_light_sampling.py [reps] [spp] [depth]     (one JSON line per measurement)"""
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
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SPP = int(sys.argv[2]) if len(sys.argv) > 2 else 16
DEPTH = int(sys.argv[3]) if len(sys.argv) > 3 else 8
REF_SPP = 4096
NEE = rt3.FLAG_LIGHT_SAMPLING
BLACK = rt3.FLAG_BLACK_BACKGROUND


def out(**row):
    print(json.dumps(row), flush=True)


def scenes(w, h):
    """(name, upload, camera, lens radius, flags of the plain render)."""
    res = []
    cr, m = rt3.scene_weekend(42)
    m = m.copy()
    lamps = np.nonzero(cr[:, 3] < 0.5)[0][::7]
    m["kind"][lamps], m["rgb"][lamps] = rt3.MAT_FLAT, 12.0
    res.append(("weekend, %d of 484 spheres emit" % len(lamps), dict(spheres=(cr, m)), rt3.weekend_camera(w, h), 0.05, BLACK))
    f, v, fm = rt3.scene_cornell(64)
    res.append(("cornell 47106 faces, one large emitter", dict(mesh=(f, v, fm)), rt3.Camera().update(w, h, 2.0, np.float32(w) / np.float32(h) * np.float32(2.0), 2.0),
                0.0, BLACK))
    cr, m = rt3.scene_stress(100000, 43)
    m = m.copy()
    m["kind"][::1000], m["rgb"][::1000] = rt3.MAT_FLAT, 20.0
    res.append(("stress 100000 spheres, 100 emit", dict(spheres=(cr, m)),
                rt3.Camera().look_at(w, h, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0), 0.0, 0))
    return res


def upload(r, up):
    r.set_mesh(*(up["mesh"] if "mesh" in up else (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))))
    r.set_spheres(*(up["spheres"] if "spheres" in up else (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))))


def time_part(r):
    W, H = 1920, 1080
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ratios = {}
    for name, up, cam, lens, base in scenes(W, H):
        upload(r, up)
        torch.cuda.synchronize()
        par = {w: rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1, flags=rt3.FLAG_GAMMA2 | base | fl, lens_radius=lens) for w, fl in (("plain", 0), ("flag", NEE))}
        ms, st = {"plain": [], "flag": []}, {}

        def render(which):
            r.render_path_device(cam.c, par[which], frame.data_ptr(), stream)
            return r.stats()                                          # waits for the call; HIP events around its trace launches
        for which in ("plain", "flag"):                               # warm-up (the flagged one builds the table)
            render(which)
        for _ in range(REPS):
            for which in ("plain", "flag"):
                st[which] = render(which)
                ms[which].append(st[which].trace_ms)
        med = {w: sorted(ms[w])[len(ms[w]) // 2] for w in ms}
        for w in ("plain", "flag"):
            out(scene=name, what="%s, %d spp, depth %d" % (w, SPP, DEPTH), ray_casts=st[w].ray_casts, median_ms=round(med[w], 3),
                min_ms=round(min(ms[w]), 3), max_ms=round(max(ms[w]), 3), mcasts_per_s=round(st[w].ray_casts / med[w] / 1e3, 1))
        ratios[name] = dict(time=round(med["flag"] / med["plain"], 4), casts=round(st["flag"].ray_casts / st["plain"].ray_casts, 4))
        # the table build: a small flagged call right after an upload (builds) against the same call again (does not)
        small = rt3.make_params(64, 36, spp=1, max_depth=2, seed=1, flags=NEE | base)
        scam = rt3.main_camera(64, 36)
        walls = []
        for _ in range(REPS):
            if "spheres" in up:
                r.set_spheres(*up["spheres"])
            else:
                r.set_mesh(*up["mesh"])
            torch.cuda.synchronize()
            t = []
            for _ in range(2):
                t0 = time.perf_counter()
                r.render_path(scam.c, small)
                t.append((time.perf_counter() - t0) * 1e3)
            walls.append(t[0] - t[1])
        out(scene=name, table_build_ms=dict(entries=len(r.light_table()[0]), median=round(sorted(walls)[len(walls) // 2], 3), min=round(min(walls), 3),
                                            max=round(max(walls), 3)))
    out(flag_over_plain=ratios)


def noise_part(r):
    w, h, spp = 480, 270, 64
    for name, up, cam, lens, base in scenes(w, h):
        upload(r, up)

        def linear(spp_, flag, seed):
            p = rt3.make_params(w, h, spp=spp_, max_depth=DEPTH, seed=seed, flags=base | flag, lens_radius=lens)
            r.render_path(cam.c, p)
            ms = r.stats().trace_ms
            return r.accum_resolve(p)[..., :3].astype(np.float64), ms
        ref, _ = linear(REF_SPP, 0, 99)
        plain, t_plain = linear(spp, 0, 1)
        flag, t_flag = linear(spp, NEE, 1)
        more = max(spp, int(round(spp * t_flag / t_plain)))
        plain_eq, t_eq = linear(more, 0, 1)
        mse = lambda a: float(((a - ref) ** 2).mean())               # noqa: E731
        out(scene=name, frame="%dx%d, depth %d, reference %d spp plain" % (w, h, DEPTH, REF_SPP), spp=spp, mse_plain=mse(plain), mse_flag=mse(flag),
            ms_plain=round(t_plain, 3), ms_flag=round(t_flag, 3), equal_time_spp_plain=more, ms_plain_equal_time=round(t_eq, 3), mse_plain_equal_time=mse(plain_eq),
            ref_mean=float(ref.mean()), flag_mean=float(flag.mean()), plain_mean=float(plain.mean()))
    # the small-lamp scene of tests/test_gpu_light_sampling.py: summed per-pixel sample variance over the floor, 64 spp
    w, h = 64, 48
    cr = np.array([[0.0, -1000.5, -3.0, 1000.0], [0.0, 0.5, -3.0, 0.05]], np.float32)
    sm = np.array([((0.6, 0.6, 0.6), 0.0, rt3.MAT_LAMBERT), ((400.0, 400.0, 400.0), 0.0, rt3.MAT_FLAT)], rt3.MATERIAL)
    upload(r, dict(spheres=(cr, sm)))
    cam = rt3.Camera().look_at(w, h, (0.0, 1.0, 1.0), (0.0, -0.5, -3.0), (0.0, 1.0, 0.0), 50.0, 4.0)
    first = r.intersect(r.camera_rays(cam.c, rt3.make_params(w, h, spp=64, max_depth=4, seed=2, flags=rt3.FLAG_VARIANCE | BLACK)), 0.001)
    floor = ((first["kind"] == rt3.HIT_SPHERE) & (first["index"] == 0)).reshape(64, h, w).all(axis=0)      # every sample's primary ray meets the floor
    var = {}
    for fl in (0, NEE):
        p = rt3.make_params(w, h, spp=64, max_depth=4, seed=2, flags=rt3.FLAG_VARIANCE | BLACK | fl)
        r.render_path(cam.c, p)
        acc, sq, done = r.accum_download(p, want_sq=True)
        mean = acc[..., :3].astype(np.float64) / done
        var[fl] = float(np.maximum(sq[..., :3].astype(np.float64) / done - mean * mean, 0.0)[floor].sum())
    out(small_lamp_variance=dict(plain=var[0], flag=var[NEE], ratio=round(var[0] / var[NEE], 1), floor_pixels=int(floor.sum())))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_light_sampling.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    time_part(r)
    noise_part(r)


if __name__ == "__main__":
    main()
