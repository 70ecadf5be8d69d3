#!/usr/bin/env python3
"""Lens sequences (rt3_denoise_temporal_optic_device, rt3_motion_optic_device) on ONE MI355X, 5 passes: device events
around each call on the current torch stream, WARMUP untimed calls, then REPS timed ones; median, min and max in ms.  Weekend, two frames one
degree of orbit apart with every sphere of odd index moved between them: per lens model at 2048x1024 (the cube at 1024x6144) the temporal call
with the motion plane and rt3_motion_optic, beside rt3_denoise_temporal_motion_device and rt3_motion_device on a pinhole frame of 2048x1024,
alternated in one process (two rounds each).  The quality line runs an 8-frame, 1-spp equirectangular weekend orbit (one degree per frame,
512x256): MSE of the last frame against a REF_SPP frame for the raw frame, rt3_denoise alone and the temporal call.  With --bench PARENT_ROOT
(a built checkout of the parent commit) the headline of bench.py (--gpus 1) is run in this tree and in that one alternately, ROUNDS times each,
in fresh processes.
The log goes to profiles/optic_bench_mi355x.log as well as to stdout.  GPU only: fails without a device.
Usage: python tools/bench_optic.py [reps] [warmup] [--no-quality] [--bench PARENT_ROOT]     (one JSON line per measurement)"""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
ARGS, PARENT_ROOT, skip = [], None, False
for i, a in enumerate(sys.argv[1:], 1):
    if skip:
        skip = False
    elif a == "--bench":
        PARENT_ROOT, skip = sys.argv[i + 1], True
    elif not a.startswith("--"):
        ARGS.append(a)
REPS = int(ARGS[0]) if len(ARGS) > 0 else 20
WARMUP = int(ARGS[1]) if len(ARGS) > 1 else 5
QUALITY = "--no-quality" not in sys.argv
W, H, PASSES, REF_SPP, ROUNDS = 2048, 1024, 5, 1024, 3
F = np.float32
LOG = os.path.join(ROOT, "profiles", "optic_bench_mi355x.log")
log_file = None


def emit(record):
    line = json.dumps(record)
    print(line, flush=True)
    log_file.write(line + "\n")
    log_file.flush()


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


def orbit_from(deg):
    a = np.radians(deg)
    return (13.0 * np.cos(a) + 3.0 * np.sin(a), 2.0, 3.0 * np.cos(a) - 13.0 * np.sin(a))


def orbit_lens(model, deg):
    return rt3.make_lens(model, orbit_from(deg), (0.0, 0.0, 0.0), fov_deg=180.0, extent=(8.0, 4.0))


def orbit_camera(w, h, deg):
    return rt3.Camera().look_at(w, h, orbit_from(deg), (0.0, 0.0, 0.0), vfov=20.0, focus_dist=10.0)


def mse(a, b):
    return float(np.mean((a[..., :3].astype(np.float64) - b[..., :3]) ** 2))


def slid(cr, k, step=(0.1, 0.02, -0.05)):
    out = cr.copy()
    out[1::2, :3] += (F(k) * np.array(step, F)).astype(F)
    return out


def two_frames(r, cr, mats, view, w, h):
    """Frame 0 (the scene as it is) and frame 1 (odd spheres moved) of `view` = ("camera", None) or ("lens", model), on the device: (colour,
    aov, view of frame 1, the history of frame 0, the motion plane of frame 1)."""
    kind, model = view
    stream = torch.cuda.current_stream().cuda_stream
    lin = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    aov = torch.empty((h, w, 12), dtype=torch.float32, device="cuda")
    prev = None
    for k in range(2):
        r.set_spheres(slid(cr, k), mats)
        p = rt3.make_params(w, h, spp=1, max_depth=8, seed=1 + k)
        if kind == "lens":
            v = orbit_lens(model, float(k))
            r.render_lens_device(v, p, 0, 1, lin.data_ptr(), stream)
            r.render_lens_aov_device(v, p, aov.data_ptr(), stream)
            if k == 0:
                _, prev = r.denoise_temporal_lens(lin, aov, v, None, iterations=PASSES)
        else:
            v = orbit_camera(w, h, float(k)).c
            r.render_path_device(v, p, torch.empty(w * h, dtype=torch.int32, device="cuda").data_ptr(), stream)
            r.accum_resolve_device(lin.data_ptr(), stream)
            r.render_aov_device(v, p, aov.data_ptr(), stream)
            if k == 0:
                _, prev = r.denoise_temporal(lin, aov, v, None, iterations=PASSES)
    prev_cr = torch.from_numpy(cr).cuda()
    plane = r.motion_lens(aov, v, prev_center_radius=prev_cr) if kind == "lens" else r.motion(aov, v, prev_center_radius=prev_cr)
    return lin, aov, v, prev, plane, prev_cr


def device_times(r):
    cr, mats = rt3.scene_weekend(42)
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    views = [(("camera", None), W, H)] + [(("lens", m), *((1024, 6144) if m == "cube" else (W, H))) for m in ("equirect", "fisheye", "ortho", "cube")]
    state = {v: two_frames(r, cr, mats, v, w, h) for v, w, h in views}
    calls = {}
    for v, w, h in views:
        lin, aov, view, prev, plane, prev_cr = state[v]
        name = "pinhole" if v[0] == "camera" else v[1]
        if v[0] == "camera":
            temporal = lambda a=state[v]: r.denoise_temporal(a[0], a[1], a[2], a[3], iterations=PASSES, motion=a[4])      # noqa: E731
            motion = lambda a=state[v]: r.motion(a[1], a[2], prev_center_radius=a[5])                                    # noqa: E731
            _, hist = temporal()
        else:
            temporal = lambda a=state[v]: r.denoise_temporal_lens(a[0], a[1], a[2], a[3], iterations=PASSES, motion=a[4])  # noqa: E731
            motion = lambda a=state[v]: r.motion_lens(a[1], a[2], prev_center_radius=a[5])                                 # noqa: E731
            _, hist = temporal()
        calls[name] = (w, h, temporal, motion, dict(moved_share=round(float((plane[..., 3] != 0).float().mean().item()), 4),
                                                    history_share=round(float((hist[0][..., 3] == 2).float().mean().item()), 4)))
    for rnd in (1, 2):                                                 # alternated in one process
        for name, (w, h, temporal, motion, shares) in calls.items():
            emit(dict(scene="weekend, odd spheres moved", view=name, frame="%dx%d" % (w, h), what="temporal denoiser, %d passes, motion plane" % PASSES,
                      round=rnd, **shares, **timed(temporal)))
            emit(dict(scene="weekend, odd spheres moved", view=name, frame="%dx%d" % (w, h), what="motion plane", round=rnd, **timed(motion)))


def quality(r, w=512, h=256, frames=8):
    r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    r.set_spheres(*rt3.scene_weekend(42))
    prev = None
    for k in range(frames):
        lens = orbit_lens("equirect", float(k))
        p = rt3.make_params(w, h, spp=1, max_depth=50, seed=100 + k)
        lin, aov = r.render_lens(lens, p), r.render_lens_aov(lens, p)
        out, prev = r.denoise_temporal_lens(lin, aov, lens, prev)
    spatial = r.denoise(lin, aov)
    ref = r.render_lens(lens, rt3.make_params(w, h, spp=REF_SPP, max_depth=50, seed=7))
    m_raw, m_sp, m_t = mse(lin, ref), mse(spatial, ref), mse(out, ref)
    emit(dict(what="quality, equirect weekend orbit, 1 degree per frame, %dx%d, frame %d, 1 spp, vs %d spp" % (w, h, frames, REF_SPP),
              mse_raw=m_raw, mse_rt3_denoise=m_sp, mse_temporal=m_t, ratio_spatial_over_temporal=round(m_sp / m_t, 3),
              history_share_full=round(float((prev[0]["length"] >= frames).mean()), 4)))


def headline(parent_root):
    """bench.py's JSON line of this tree and of the parent's checkout, alternated, a fresh process each."""
    for rnd in range(1, ROUNDS + 1):
        for name, root in (("tree", ROOT), ("parent", os.path.abspath(parent_root))):
            env = {k: v for k, v in os.environ.items() if k != "RT3_LIB_PATH"}
            done = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env, cwd=root,
                                  capture_output=True, text=True, timeout=600)
            if done.returncode != 0:
                raise SystemExit("bench.py failed in the %s checkout:\n%s" % (name, done.stderr[-2000:]))
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("{")][-1]
            emit(dict(what="bench.py --gpus 1 --steps 3 --warmup 1", checkout=name, round=rnd, result=json.loads(line)))


def main():
    global log_file
    if not torch.cuda.is_available():
        raise SystemExit("bench_optic.py needs an MI355X (no CPU fallback)")
    log_file = open(LOG, "w")
    if PARENT_ROOT:                                                    # first: no context of this process is open yet
        headline(PARENT_ROOT)
    r = rt3.initialize_renderer(0)
    device_times(r)
    if QUALITY:
        quality(r)
    r.close()
    log_file.close()


if __name__ == "__main__":
    main()
