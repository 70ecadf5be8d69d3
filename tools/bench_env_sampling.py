#!/usr/bin/env python3
"""Importance sampling of the environment map (RT3_FLAG_ENV_SAMPLING) on ONE MI355X: what the shadow rays cost and what they buy.
Time: the three benchmark scenes — weekend (484 spheres, k_trace_mfma32), rt3_scene_stress(100000) (the resident three-level form) and
rt3_scene_cornell(64) (47 106 faces) — at 1920x1080, SPP samples, depth DEPTH under a random N = N_FACE map, rendered with and without the flag, alternated
in one process: trace_ms and ray_casts of each, the ratio, and the time of the table build (the first flagged call after set_environment against the
second, whole-call wall time with a device synchronisation).
Noise: the weekend scene at 480x270 under a sky with a small sun (a smooth gradient plus a 3 x 3-texel block of radiance 20 000 on face +Y) and under the
smooth gradient alone: the mean squared error of the linear frame against a plain 4096-spp frame, at equal samples and at (about) equal time — the plain
render gets time_ratio times the samples.  Also the variance ratio of the test suite's bright-block scene.
GPU only: fails without a device.
Usage: python tools/bench_env_sampling.py [reps] [spp] [depth] [n_face]     (one JSON line per measurement)"""
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
N_FACE = int(sys.argv[4]) if len(sys.argv) > 4 else 512
W, H = 1920, 1080
NEE = rt3.FLAG_ENV_SAMPLING


def out(**row):
    print(json.dumps(row), flush=True)


def gradient_cube(n, sun):
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    s, t = np.meshgrid(c, c)
    cube = np.zeros((6, n, n, 4), np.float32)
    dirs = [(1 + 0 * s, -t, -s), (-1 + 0 * s, -t, s), (s, 1 + 0 * s, t), (s, -1 + 0 * s, -t), (s, -t, 1 + 0 * s), (-s, -t, -1 + 0 * s)]
    for f, (x, y, z) in enumerate(dirs):
        up = y / np.sqrt(x * x + y * y + z * z)
        a = 0.5 * (up + 1.0)
        cube[f, ..., 0], cube[f, ..., 1], cube[f, ..., 2] = 1.0 - 0.5 * a, 1.0 - 0.3 * a, 1.0
    if sun:
        cube[2, n // 3:n // 3 + 3, n // 2:n // 2 + 3, :3] = 20000.0
    return cube


def time_part(r):
    cube = torch.from_numpy(np.random.default_rng(2026).uniform(0.0, 2.0, (6, N_FACE, N_FACE, 4)).astype(np.float32)).cuda()
    empty_sph = (np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))
    empty_mesh = (np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    scenes = []
    cr, m = rt3.scene_weekend(42)
    scenes.append(("weekend 484 spheres", dict(spheres=(cr, m)), rt3.weekend_camera(W, H), 0.05))
    cr, m = rt3.scene_stress(100000, 43)
    scenes.append(("stress 100000 spheres", dict(spheres=(cr, m)), rt3.Camera().look_at(W, H, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0), 0.0))
    f, v, fm = rt3.scene_cornell(64)
    scenes.append(("cornell 47106 faces", dict(mesh=(f, v, fm)), rt3.Camera().update(W, H, 2.0, 2.0, 2.0), 0.0))
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ratios = {}
    for name, up, cam, lens in scenes:
        r.set_mesh(*(up["mesh"] if "mesh" in up else empty_mesh))
        r.set_spheres(*(up["spheres"] if "spheres" in up else empty_sph))
        r.set_environment(cube)
        torch.cuda.synchronize()
        par = {w: rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1, flags=rt3.FLAG_GAMMA2 | fl, lens_radius=lens) for w, fl in (("plain", 0), ("flag", NEE))}
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
            out(scene=name, what="%s, N = %d map, %d spp, depth %d" % (w, N_FACE, SPP, DEPTH), ray_casts=st[w].ray_casts, median_ms=round(med[w], 3),
                min_ms=round(min(ms[w]), 3), max_ms=round(max(ms[w]), 3), mcasts_per_s=round(st[w].ray_casts / med[w] / 1e3, 1))
        ratios[name] = dict(time=round(med["flag"] / med["plain"], 4), casts=round(st["flag"].ray_casts / st["plain"].ray_casts, 4))
    out(flag_over_plain=ratios)
    # the table build: a small flagged call right after set_environment (builds) against the same call again (does not)
    small = rt3.make_params(64, 36, spp=1, max_depth=2, seed=1, flags=NEE)
    cam = rt3.main_camera(64, 36)
    walls = []
    for _ in range(REPS):
        r.set_environment(cube)
        torch.cuda.synchronize()
        t = []
        for _ in range(2):
            t0 = time.perf_counter()
            r.render_path(cam.c, small)
            t.append((time.perf_counter() - t0) * 1e3)
        walls.append(t[0] - t[1])
    out(table_build_ms=dict(n_face=N_FACE, cells=6 * min(N_FACE, 256) ** 2, median=round(sorted(walls)[len(walls) // 2], 3), min=round(min(walls), 3), max=round(max(walls), 3)))


def noise_part(r):
    w, h, depth, ref_spp, spp = 480, 270, 8, 4096, 64
    cr, m = rt3.scene_weekend(42)
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    r.set_spheres(cr, m)
    cam = rt3.weekend_camera(w, h)

    def linear(spp_, flag, seed):
        p = rt3.make_params(w, h, spp=spp_, max_depth=depth, seed=seed, flags=flag, lens_radius=0.05)
        r.render_path(cam.c, p)
        ms = r.stats().trace_ms
        return r.accum_resolve(p)[..., :3].astype(np.float64), ms
    for name, sun in (("sky + small sun", True), ("smooth sky", False)):
        r.set_environment(gradient_cube(64, sun))
        ref, _ = linear(ref_spp, 0, 99)
        plain, t_plain = linear(spp, 0, 1)
        flag, t_flag = linear(spp, NEE, 1)
        more = max(spp, int(round(spp * t_flag / t_plain)))
        plain_eq, t_eq = linear(more, 0, 1)
        mse = lambda a: float(((a - ref) ** 2).mean())               # noqa: E731
        out(map=name, frame="%dx%d weekend, depth %d, reference %d spp plain" % (w, h, depth, ref_spp), spp=spp, mse_plain=mse(plain), mse_flag=mse(flag),
            ms_plain=round(t_plain, 3), ms_flag=round(t_flag, 3), equal_time_spp_plain=more, ms_plain_equal_time=round(t_eq, 3), mse_plain_equal_time=mse(plain_eq),
            ref_mean=float(ref.mean()), flag_mean=float(flag.mean()), plain_mean=float(plain.mean()))
    # the bright-block scene of tests/test_gpu_env_sampling.py: summed per-pixel sample variance over the ground, 64 spp
    w, h = 64, 48
    r.set_spheres(np.array([[0.0, -1000.5, -3.0, 1000.0]], np.float32), np.array([((0.6, 0.6, 0.6), 0.0, rt3.MAT_LAMBERT)], rt3.MATERIAL))
    cube = np.zeros((6, 32, 32, 4), np.float32)
    cube[2, 20:22, 9:11, :3] = 400.0
    r.set_environment(cube)
    cam = rt3.Camera().look_at(w, h, (0.0, 1.0, 1.0), (0.0, -0.5, -3.0), (0.0, 1.0, 0.0), 50.0, 4.0)
    ground = r.render_aov(cam.c, rt3.make_params(w, h, spp=4, max_depth=4, seed=2))["coverage"] == 1.0
    var = {}
    for fl in (0, NEE):
        p = rt3.make_params(w, h, spp=64, max_depth=4, seed=2, flags=rt3.FLAG_VARIANCE | fl)
        r.render_path(cam.c, p)
        acc, sq, done = r.accum_download(p, want_sq=True)
        mean = acc[..., :3].astype(np.float64) / done
        var[fl] = float(np.maximum(sq[..., :3].astype(np.float64) / done - mean * mean, 0.0)[ground].sum())
    out(bright_block_variance=dict(plain=var[0], flag=var[NEE], ratio=round(var[0] / var[NEE], 1), ground_pixels=int(ground.sum())))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_env_sampling.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    time_part(r)
    noise_part(r)
    r.clear_environment()


if __name__ == "__main__":
    main()
