"""Shared scene/case definitions for the parity tests and the golden generator."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as O  # noqa: E402

rt3 = importlib.import_module("raytracer-3_amd")
TEDDY = os.path.join(GOLDEN, "teddy.obj")             # the reference's bin/objects/teddy.obj, as data


def load_builtin_scene():
    """Flattened built-in scene of src/Main.cpp:280-283 from the committed fixture (works without /root/reference)."""
    z = np.load(os.path.join(GOLDEN, "builtin_scene.npz"))
    return z["faces"].view(O.GFACE).reshape(-1), z["verts"]


def mode_x_cases():
    """name -> dict(scene arrays, camera, params)."""
    cases = {}
    cr, mats = rt3.scene_three_spheres()
    cam = rt3.Camera().update(64, 36, 1.0, np.float32(64) / np.float32(36) * np.float32(2.0), 2.0)
    cases["three_spheres_64x36x16_d8"] = dict(spheres=cr, smats=mats, cam=cam.c,
                                              params=dict(width=64, height=36, spp=16, max_depth=8, seed=1, flags=1))
    cr, mats = rt3.scene_weekend(42)
    cam = rt3.weekend_camera(96, 54)
    cases["weekend_96x54x4_d50_lens"] = dict(spheres=cr, smats=mats, cam=cam.c,
                                             params=dict(width=96, height=54, spp=4, max_depth=50, seed=1, flags=1, lens_radius=0.05))
    cases["weekend_96x54x9_d12_tile1of3"] = dict(spheres=cr, smats=mats, cam=cam.c,
                                                 params=dict(width=96, height=54, spp=9, max_depth=12, seed=5, flags=1,
                                                             tile_rows=4, tile_index=1, tile_count=3))
    faces, verts, fmats = rt3.scene_cornell(4)
    cam = rt3.Camera().update(48, 48, 2.0, 2.0, 2.0)
    cases["cornell_g4_48x48x8_d6_black"] = dict(faces=faces, verts=verts, fmats=fmats, cam=cam.c,
                                                params=dict(width=48, height=48, spp=8, max_depth=6, seed=3, flags=1 | 2))
    return cases


def oracle_render(case, threads=8, **override):
    """Renders a case with the CPU oracle; returns (pixels, ray_casts)."""
    params = dict(case["params"])
    params.update(override)
    p = O.make_params(**params)
    kw = {}
    if case.get("spheres") is not None:
        kw.update(spheres=case["spheres"], smats=np.ascontiguousarray(case["smats"]).view(O.MATERIAL))
    if case.get("faces") is not None:
        fm = case.get("fmats")
        kw.update(faces=np.ascontiguousarray(case["faces"]).view(O.GFACE), verts=case["verts"],
                  fmats=None if fm is None else np.ascontiguousarray(fm).view(O.MATERIAL))
    return O.render_path(O.copy_camera(case["cam"]), p, threads=threads, **kw)


def hip_upload(r, case):
    """Uploads a case's scene to a HipRenderer through the C ABI."""
    if case.get("faces") is not None:
        r.set_mesh(case["faces"], case["verts"], case.get("fmats"))
    else:
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), np.float32))
    if case.get("spheres") is not None:
        r.set_spheres(case["spheres"], case["smats"])
    else:
        r.set_spheres(np.zeros((0, 4), np.float32), np.zeros(0, rt3.MATERIAL))


def hip_render(r, case, upload=True, **override):
    """Renders a case with the HIP path (rt3_render_path); returns the compact pixel array."""
    if upload:
        hip_upload(r, case)
    params = dict(case["params"])
    params.update(override)
    return r.render_path(case["cam"], rt3.make_params(**params))
