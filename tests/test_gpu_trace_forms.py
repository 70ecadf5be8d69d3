"""The table plan_trace picks a trace kernel from, walked in one place: every form (Render, RenderRef, Query, List, Rays) under
every switch that selects a kernel family, on three tiny scenes, against the same form of the unfiltered kernel (rt3_debug_force_brute).  The
comparisons are those of the form's own tests — pixels and counts by equality (test_gpu_brute, test_gpu_adaptive), hits by test_gpu_ray_query's
same(), radiance by test_gpu_radiance's same(): bit for bit.  A family that has no such form (rt3.h: queries and rt3_radiance* ignore RT3_NO_MFMA
and RT3_MFMA_K64) must ignore the switch and still equal the unfiltered result."""
import contextlib
import os

import numpy as np
import pytest

from test_gpu_radiance import same as same_radiance
from test_gpu_ray_query import query, same as same_hits

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, SEED = 32, 8, 4, 4, 9                               # four waves of pixels; 4 spp: the stratified path
FAMILIES = {                                                          # the switches are read per call
    "default": {}, "force_tiled": {"RT3_FORCE_TILED": "1"}, "no_resident": {"RT3_NO_RESIDENT": "1"},
    "levels3": {"RT3_LEVELS": "3"}, "levels4": {"RT3_LEVELS": "4"}, "levels4_tiled": {"RT3_LEVELS": "4", "RT3_NO_RESIDENT": "1"},
    "no_mfma": {"RT3_NO_MFMA": "1"}, "k64": {"RT3_MFMA_K64": "1"},
}
SCENES = ["spheres", "mesh", "both"]


@contextlib.contextmanager
def family(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@contextlib.contextmanager
def unfiltered(r):
    r.force_brute(True)
    try:
        yield
    finally:
        r.force_brute(False)


def families_of(scene):
    """A sphere-only scene of <= 512 spheres takes the single-block kernel unless RT3_FORCE_TILED sends it on: every family once more with it."""
    out = dict(FAMILIES)
    if scene == "spheres":
        out.update({"tiled_" + k: dict(v, RT3_FORCE_TILED="1") for k, v in FAMILIES.items() if k != "force_tiled"})
    return out


def upload(rt3, r, scene):
    """40 spheres (one of them the ground: the direct list), a device-tessellated sphere of a few dozen faces (rt3_mesh_sphere), or both."""
    ents = []
    if scene != "spheres":
        ents.append(rt3.create_sphere((0.3, 0.0, -3.5), 0.8, 6, 5, (0.7, 0.4, 0.3), material=rt3.lambertian((0.7, 0.4, 0.3))))
    r.prerender(ents, gpu_prerender=True)
    if scene != "spheres":
        assert 24 <= r.n_faces <= 100
    if scene != "mesh":
        rng = np.random.default_rng(40)
        cr = np.zeros((40, 4), np.float32)
        cr[:, :3] = rng.uniform([-6.0, -0.6, -6.0], [6.0, 1.2, -2.5], (40, 3))
        cr[:, 3] = rng.uniform(0.1, 0.5, 40)
        cr[0] = (0.0, -100.6, -4.0, 100.0)
        sm = np.zeros(40, rt3.MATERIAL)
        sm["kind"] = np.arange(40) % 4                                # flat, Lambert, metal, dielectric
        sm["rgb"] = rng.uniform(0.2, 1.0, (40, 3))
        sm["param"] = np.where(sm["kind"] == 3, 1.5, rng.uniform(0.0, 0.5, 40)).astype(np.float32)
        r.set_spheres(cr, sm)
        assert len(r.sphere_build()[1]) >= 1                          # the ground is tested directly, not through the filter
    cam = rt3.Camera().update(W, H, 1.0, 4.0, 1.0)                    # at the origin, looking down -z, no lens
    return cam, rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=SEED, flags=1)


def walk(r, scene, call, same, check=None, unfiltered_call=None):
    """call() under every family equals call() of the unfiltered kernel; check(name, env, stats) says which kernel must have run."""
    with unfiltered(r):
        ref = (unfiltered_call or call)()
        assert r.stats().mfma_instructions == 0
    for name, env in families_of(scene).items():
        with family(env):
            got = call()
        same(got, ref, "%s / %s" % (scene, name))
        if check:
            check(name, env, r.stats())
    return ref


def equal(a, b, what):
    for x, y in zip(a, b) if isinstance(a, tuple) else [(a, b)]:
        assert np.array_equal(x, y), "%s: %d values differ" % (what, int((x != y).sum()))


@pytest.mark.parametrize("scene", SCENES)
def test_render(rt3, renderer, scene):
    cam, p = upload(rt3, renderer, scene)

    def check(name, env, st):
        valu = "RT3_NO_MFMA" in env
        assert (st.mfma_instructions == 0) == valu, name             # the vector-ALU scan | a matrix-filter kernel
        if not valu:
            single = scene == "spheres" and "RT3_FORCE_TILED" not in env
            assert st.mfma_flop_per_instruction == (32768 if single and "RT3_MFMA_K64" in env else 16384), name
    ref = walk(renderer, scene, lambda: renderer.render_path(cam.c, p), equal, check)
    assert len(np.unique(ref)) > 16                                   # not a frame of sky


@pytest.mark.parametrize("scene", SCENES)
def test_query(rt3, renderer, scene):
    cam, p = upload(rt3, renderer, scene)
    rays = renderer.camera_rays(cam.c, p)
    assert len(rays) == W * H * SPP

    def check(name, env, st):                                         # no VALU and no K = 64 form: the switches are ignored
        assert st.mfma_instructions > 0 and st.mfma_flop_per_instruction == 16384, name
    ref = walk(renderer, scene, lambda: query(renderer, rays, np.float32(0.001)), same_hits, check,
               unfiltered_call=lambda: query(renderer, rays, np.float32(0.001), brute=True))       # (query() sets the debug switch itself)
    kinds = np.bincount(ref["kind"], minlength=4)
    assert kinds[0] > 0 and kinds[3] == 0 and (scene == "spheres" or kinds[1] > 0) and (scene == "mesh" or kinds[2] > 0), kinds


@pytest.mark.parametrize("scene", SCENES)
def test_rays(rt3, renderer, scene):
    cam, p = upload(rt3, renderer, scene)
    rays = renderer.camera_rays(cam.c, p, 0, 1)
    assert len(rays) == W * H

    def check(name, env, st):
        assert st.mfma_instructions > 0 and st.mfma_flop_per_instruction == 16384 and st.samples == W * H * SPP, name
    ref = walk(renderer, scene, lambda: renderer.radiance(rays, samples=SPP, max_depth=DEPTH, seed=SEED), same_radiance, check)
    assert not np.isnan(ref).any() and (ref[:, :3] != 0).any(axis=1).mean() > 0.2


@pytest.mark.parametrize("scene", SCENES)
def test_list(rt3, renderer, scene):
    """An adaptive render whose threshold nothing reaches: every pixel with any variance goes on after the first round, through the list form."""
    cam, p = upload(rt3, renderer, scene)

    def check(name, env, st):
        assert (st.mfma_instructions == 0) == ("RT3_NO_MFMA" in env) and st.launches == 3, name       # rounds of 2, 1 and 1 samples
    _, counts = walk(renderer, scene, lambda: renderer.render_adaptive(cam.c, p, threshold=1e-30, min_spp=2, step_spp=1), equal, check)
    assert (counts == SPP).mean() > 0.2                               # rounds 2 and 3 had their lists


def test_render_ref(rt3, renderer):
    """RT3_FLAG_REFERENCE_PRIMARY: the face-only scene, camera at the origin, no lens (anything else takes the unfiltered kernel)."""
    cam, _ = upload(rt3, renderer, "mesh")
    p = rt3.make_params(W, H, spp=SPP, max_depth=DEPTH, seed=SEED, flags=1 | rt3.FLAG_REFERENCE_PRIMARY)
    with unfiltered(renderer):
        ref = renderer.render_path(cam.c, p)
    assert len(np.unique(ref)) > 16
    for name in ("default", "levels3", "levels4", "no_mfma"):
        with family(FAMILIES[name]):
            equal(renderer.render_path(cam.c, p), ref, name)
        assert (renderer.stats().mfma_instructions == 0) == (name == "no_mfma"), name
