#!/usr/bin/env python3
"""Image textures (rt3_set_texture*, rt3_bind_*_textures*) on ONE MI355X: what an albedo map costs a Mode-X render.  The three
benchmark scenes — weekend (484 spheres, k_trace_mfma32 with strip lists), rt3_scene_stress(100000) (the resident three-level form) and
rt3_scene_cornell(64) (47 106 faces) — at 1920x1080, SPP samples, depth DEPTH, the same scene, camera and parameters rendered three ways, alternated in
one process:
    plain     no binding: the Render form, the sky
    white     a 1 x 1 texel of (1, 1, 1) on every Lambert and metal primitive: the texture form, every fetch the same 16 bytes — the same paths and the
              same image as `plain`, so white / plain is the cost of the FORM (the descriptor, the (u, v), the four loads that hit one line)
    image     a random SIDE x SIDE texture on the same primitives (spheres: their own (u, v); faces: a planar projection of the vertices on the two
              longest axes of the scene's box, SIDE / 64 tiles across it): other albedos but the same paths — an albedo changes no ray — so
              image / white is the cost of the FETCHES (four 16-byte loads per hit from 16 MB) and image / plain what a user sees
Kernel time from the C ABI's HIP events (rt3_stats.trace_ms) after a warm-up: median, min and max of REPS rounds.  GPU only: fails without a device.
Usage: python tools/bench_textures.py [reps] [spp] [depth] [side]     (one JSON line per measurement)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SPP = int(sys.argv[2]) if len(sys.argv) > 2 else 16
DEPTH = int(sys.argv[3]) if len(sys.argv) > 3 else 8
SIDE = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
W, H = 1920, 1080
WHITE, IMAGE = 0, 1


def report(scene, what, ms, st):
    med = ms[len(ms) // 2]
    row = dict(scene=scene, what=what, paths=W * H * SPP, ray_casts=st.ray_casts, median_ms=round(med, 3), min_ms=round(ms[0], 3), max_ms=round(ms[-1], 3),
               mcasts_per_s=round(st.ray_casts / med / 1e3, 1), launches=st.launches)
    print(json.dumps(row), flush=True)
    return row


def slots_of(mats, slot):
    """`slot` for every Lambert and metal primitive, none for the rest."""
    return np.where((mats["kind"] == rt3.MAT_LAMBERT) | (mats["kind"] == rt3.MAT_METAL), slot, rt3.TEX_NONE).astype(np.uint32)


def planar_uv(faces, verts):
    """(n_faces, 6): every vertex projected on the two longest axes of the vertices' box, SIDE / 64 repeats of the texture across the box."""
    v = np.asarray(verts, np.float32)[:, :3]
    lo, hi = v.min(axis=0), v.max(axis=0)
    a, b = np.argsort(hi - lo)[::-1][:2]
    t = (v[:, [a, b]] - lo[[a, b]]) / np.maximum(hi - lo, 1e-6)[[a, b]] * np.float32(SIDE / 64.0)
    return np.ascontiguousarray(np.concatenate([t[faces["v1"]], t[faces["v2"]], t[faces["v3"]]], axis=1), np.float32)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_textures.py needs an MI355X (no CPU fallback)")
    r = rt3.initialize_renderer(0)
    r.set_texture(WHITE, np.ones((1, 1, 3), np.float32))
    r.set_texture(IMAGE, torch.from_numpy(np.random.default_rng(2026).uniform(0.1, 1.0, (SIDE, SIDE, 4)).astype(np.float32)).cuda())
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
        p = rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=1, flags=rt3.FLAG_GAMMA2, lens_radius=lens)
        uv = planar_uv(up["mesh"][0], up["mesh"][1]) if "mesh" in up else None

        def render(which):
            slot = {"plain": None, "white": WHITE, "image": IMAGE}[which]
            if "spheres" in up:
                r.bind_sphere_textures(None if slot is None else slots_of(up["spheres"][1], slot))
            else:
                r.bind_mesh_textures(None if slot is None else slots_of(up["mesh"][2], slot), uv)
            r.render_path_device(cam.c, p, frame.data_ptr(), stream)
            return r.stats(), frame.clone()                             # stats() waits for the call; HIP events around its trace launches
        order = ("plain", "white", "image")
        ms, st, img = {k: [] for k in order}, {}, {}
        for which in order:                                             # warm-up
            render(which)
        for _ in range(REPS):
            for which in order:
                st[which], img[which] = render(which)
                ms[which].append(st[which].trace_ms)
        assert st["plain"].ray_casts == st["white"].ray_casts == st["image"].ray_casts                        # an albedo changes no path
        assert torch.equal(img["plain"], img["white"]) and not torch.equal(img["plain"], img["image"])        # a white texture is no texture
        rows = {k: report(name, "mode-X render, %s, %d spp, depth %d" % (k if k != "image" else "%d x %d image" % (SIDE, SIDE), SPP, DEPTH), sorted(ms[k]), st[k])
                for k in order}
        ratios[name] = dict(white_over_plain=round(rows["white"]["median_ms"] / rows["plain"]["median_ms"], 4),
                            image_over_plain=round(rows["image"]["median_ms"] / rows["plain"]["median_ms"], 4),
                            image_over_white=round(rows["image"]["median_ms"] / rows["white"]["median_ms"], 4))
    r.clear_textures()
    print(json.dumps(dict(texture_trace_ms_ratios=ratios)), flush=True)


if __name__ == "__main__":
    main()
