"""The specular-chain law (include/rt3.h "Specular-chain AOVs") without a GPU: rt3_debug_aov_bounce against the numpy restatement
bit for bit, the restatement itself against a mirrored camera, the wire struct, the header and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aov_chain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt3.h")
F = np.float32
E_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def bounce_inputs():
    """Some thousand hits: metal and dielectric (and the kinds a chain ends on), front and back, grazing, total internal reflection, cosv clamped."""
    rng = np.random.default_rng(2027)
    blocks = []

    def block(k, d, n, kinds, fuzz=None, ior=None):
        mk = rng.choice(kinds, k).astype(np.uint32)
        m = np.zeros((k, 4), F)
        m[:, :3] = rng.uniform(0.05, 1.0, (k, 3))
        m[:, 3] = rng.choice([0.0, 0.0, 0.25, 1.0], k) if fuzz is None else fuzz
        g = mk == R.MAT_DIELECTRIC
        iors = (rng.uniform(1.05, 2.4, k) if ior is None else np.full(k, ior)).astype(F)
        m[g, 0] = (F(1.0) / iors)[g]
        m[g, 3] = iors[g]
        blocks.append(dict(d=d, n=n, mk=mk, m=m, p=rng.uniform(-50.0, 50.0, (k, 3)).astype(F), T=rng.uniform(0.0, 1.0, (k, 3)).astype(F),
                           b=rng.integers(0, 5, k).astype(np.uint32)))

    k = 1500
    block(k, unit(rng.normal(size=(k, 3))), unit(rng.normal(size=(k, 3))), [0, 1, 2, 2, 3, 3])           # front and back, every kind
    n = unit(rng.normal(size=(k, 3)))
    t = unit(np.cross(n, rng.normal(size=(k, 3))))
    block(k, unit(t.astype(np.float64) + rng.choice([-1, 1], (k, 1)) * 10.0 ** rng.uniform(-9, -2, (k, 1)) * n), n, [2, 3])     # grazing
    n = unit(rng.normal(size=(k, 3)))
    t = unit(np.cross(n, rng.normal(size=(k, 3))))
    s = rng.uniform(0.55, 0.999, (k, 1))                              # sin of the angle inside the glass: beyond 1 / 1.5 mostly
    block(k, unit(s * t + np.sqrt(1.0 - s * s) * n), n, [3], ior=1.5)                                       # back side: total internal reflection
    n = unit(rng.normal(size=(k, 3)))
    block(k, (-n * F(1.0 + 2.0 ** -22)).astype(F), n, [2, 3])                                               # -(d.n) > 1 for many: cosv clamped
    ins = {key: np.concatenate([b[key] for b in blocks]) for key in blocks[0]}
    ins["p"][::97, 1] = np.inf                                        # a next ray the query engine would refuse: the chain ends
    return ins


def host_step(rt3, ins, max_bounces, max_fuzz):
    L = rt3.lib()
    k = len(ins["d"])
    chain = rt3.rt3_aov_chain_params(max_bounces, max_fuzz, 0, 0)
    follow = np.zeros(k, np.uint32)
    rgb, nor, dr = (np.zeros((k, 3), F) for _ in range(3))
    arrs = [np.ascontiguousarray(ins[key]) for key in ("d", "p", "n", "m", "T")]
    ptr = lambda a, i, stride: C.c_void_p(a.ctypes.data + stride * i)     # noqa: E731
    for i in range(k):
        rc = L.rt3_debug_aov_bounce(ptr(arrs[0], i, 12), ptr(arrs[1], i, 12), ptr(arrs[2], i, 12), int(ins["mk"][i]), ptr(arrs[3], i, 16),
                                    ptr(arrs[4], i, 12), int(ins["b"][i]), C.byref(chain), ptr(rgb, i, 12), ptr(nor, i, 12), ptr(dr, i, 12),
                                    ptr(follow, i, 4))
        assert rc == 0
    return follow, rgb, nor, dr


@pytest.mark.parametrize("max_bounces,max_fuzz", [(4, 0.0), (2, 0.25), (16, 1.0)])
def test_debug_bounce_equals_the_restatement(rt3, max_bounces, max_fuzz):
    ins = bounce_inputs()
    follow, rgb, nor, dr = host_step(rt3, ins, max_bounces, max_fuzz)
    f2, rgb2, nor2, dr2 = R.step(ins["d"], ins["p"], ins["n"], ins["mk"], ins["m"], ins["T"], ins["b"], max_bounces, max_fuzz)
    assert np.array_equal(follow != 0, f2)
    for a, b in ((rgb, rgb2), (nor, nor2), (dr, dr2)):
        assert np.array_equal(bits(a), bits(b))
    # the inputs reach every branch: followed mirrors and glass, refusals by kind, fuzz and bounce count, absorption, total internal reflection, the clamp
    glass, metal = ins["mk"] == 3, ins["mk"] == 2
    assert (f2 & glass).sum() > 500 and (f2 & metal).sum() > 100 and (~f2 & metal).sum() > 50 and not f2[ins["mk"] < 2].any()
    dn = -np.abs(R.dot(ins["d"], ins["n"]))
    assert (-dn > F(1.0)).sum() > 100                                 # cosv clamped
    back = glass & (R.dot(ins["d"], ins["n"]) >= 0)
    sin2 = 1.0 - dn.astype(np.float64) ** 2
    assert (back & (ins["m"][:, 3].astype(np.float64) ** 2 * sin2 > 1.0)).sum() > 500       # total internal reflection
    assert (np.abs(dn) < 1e-4).sum() > 500                            # grazing
    if max_bounces <= 4:
        assert ((ins["b"] >= max_bounces) & (glass | metal)).sum() > 100      # out of bounces


def test_followed_directions_are_valid_rays(rt3):
    ins = bounce_inputs()
    follow, _, nor, dr = R.step(ins["d"], ins["p"], ins["n"], ins["mk"], ins["m"], ins["T"], ins["b"], 16, 1.0)
    assert R.ray_valid(ins["p"][follow], dr[follow]).all()
    assert (R.dot(ins["d"], nor) <= 0).all()                          # flipped normals face the ray
    assert not follow[::97].any()                                     # the non-finite hit points end their chains


# ---------------------------------------------------------------------------------------------- a plane mirror against the mirrored camera
MW, MH, MZ = 32, 24, -4.0


def mirror_scene(rt3):
    """A plane mirror z = MZ (two fuzz-0 metal faces, rgb 1, normal +z) in front of a camera at the origin that looks down -z, and FLAT-coloured
    spheres behind the camera: every primary ray hits the mirror, every sphere is seen through it only."""
    verts = np.array([[-40, -40, MZ, 1], [40, -40, MZ, 1], [40, 40, MZ, 1], [-40, 40, MZ, 1]], F)
    faces = np.zeros(2, rt3.GFACE)
    faces["v1"], faces["v2"], faces["v3"] = [0, 0], [2, 3], [1, 2]          # (the face test's winding: clockwise about the normal)
    faces["normal"] = [0.0, 0.0, 1.0]
    faces["color"] = 1.0
    fmats = np.zeros(2, rt3.MATERIAL)
    fmats["rgb"], fmats["param"], fmats["kind"] = 1.0, 0.0, R.MAT_METAL
    rng = np.random.default_rng(5)
    n = 40
    cr = np.zeros((n, 4), F)
    cr[:, 0], cr[:, 1] = rng.uniform(-4.5, 4.5, n), rng.uniform(-3.2, 3.2, n)
    cr[:, 2], cr[:, 3] = rng.uniform(1.5, 5.0, n), rng.uniform(0.8, 1.6, n)
    smats = np.zeros(n, rt3.MATERIAL)
    smats["rgb"], smats["kind"] = rng.uniform(0.1, 0.9, (n, 3)), R.MAT_FLAT
    return dict(faces=faces, verts=verts, fmats=fmats, spheres=cr, smats=smats)


def pinhole_rays(rt3):
    """One ray per pixel of a MW x MH frame from the origin down -z, and its mirror image about z = MZ (exact: a sign and one subtraction)."""
    x = (np.arange(MW) + 0.5) / MW * 2.0 - 1.0
    y = 1.0 - (np.arange(MH) + 0.5) / MH * 2.0
    d = unit(np.stack(np.broadcast_arrays(x[None, :] * 0.8, y[:, None] * 0.6, -1.0), axis=-1).reshape(-1, 3))
    rays = np.zeros(MW * MH, rt3.RAY)
    rays["direction"], rays["t_max"] = d, np.inf
    mirrored = rays.copy()
    mirrored["origin"][:, 2] = F(2.0 * MZ)
    mirrored["direction"][:, 2] = -d[:, 2]
    return rays, mirrored


def oracle_tracer(rt3, oracle, scene, with_faces):
    def trace(rays):
        hits = np.zeros(len(rays), rt3.HIT)
        for i, r in enumerate(rays):
            kind, t, idx = oracle.nearest(r["origin"], r["direction"], spheres=scene["spheres"], faces=scene["faces"] if with_faces else None,
                                          verts=scene["verts"] if with_faces else None)
            hits[i] = (t, kind, idx, 0) if kind else (np.inf, 0, 0xFFFFFFFF, 0)
        return hits
    return trace


def test_plane_mirror_equals_the_mirrored_camera(rt3, oracle):
    scene = mirror_scene(rt3)
    rays, mirrored = pinhole_rays(rt3)
    through, info = R.chain_aov(rays, oracle_tracer(rt3, oracle, scene, True), scene, 8, 0.0, 1, rt3.AOV, rt3.RAY)
    direct, dinfo = R.chain_aov(mirrored, oracle_tracer(rt3, oracle, scene, False), scene, 0, 0.0, 1, rt3.AOV, rt3.RAY)
    on_mirror = through["kind"] == R.HIT_FACE
    assert on_mirror.all()                                            # the mirror fills the frame; kind / index name it, not what it shows
    assert (through["index"] < 2).all() and (through["coverage"] == 1.0).all()
    same = (info["end_hit"] == dinfo["end_hit"]) & (info["end_index"] == dinfo["end_index"])
    left_out = int((on_mirror & ~same).sum())
    assert left_out <= 0.02 * on_mirror.sum(), left_out
    on_prim = same & (info["end_hit"] == R.HIT_SPHERE)
    assert on_prim.sum() > 200 and (same & (info["end_hit"] == R.HIT_NONE)).sum() > 20       # spheres and sky both show in the mirror
    assert (info["bounces"][on_prim] == 1).all()
    assert np.array_equal(bits(through["albedo"][on_prim]), bits(direct["albedo"][on_prim]))
    assert np.array_equal(bits(through["albedo"][on_prim]), bits(scene["smats"]["rgb"][info["end_index"][on_prim]]))
    # the path length through the mirror is the mirrored camera's distance, up to the rounding of the two legs
    assert np.allclose(through["depth"][on_prim], direct["depth"][on_prim], rtol=1e-5)
    assert info["casts"] == MW * MH + int(on_mirror.sum())


def test_zero_bounces_is_the_first_hit(rt3, oracle):
    scene = mirror_scene(rt3)
    rays, _ = pinhole_rays(rt3)
    aov, info = R.chain_aov(rays, oracle_tracer(rt3, oracle, scene, True), scene, 0, 0.0, 1, rt3.AOV, rt3.RAY)
    assert info["casts"] == MW * MH and (info["bounces"] == 0).all()
    assert np.array_equal(aov["albedo"], np.ones((MW * MH, 3), F)) and np.array_equal(aov["normal"], np.tile(F([0, 0, 1]), (MW * MH, 1)))


# ---------------------------------------------------------------------------------------------- wire struct, header, bindings, refusals
def test_struct_size(rt3):
    assert C.sizeof(rt3.rt3_aov_chain_params) == 16
    assert [f[0] for f in rt3.rt3_aov_chain_params._fields_] == ["max_bounces", "max_fuzz", "flags", "_pad"]


def test_header_and_bindings(rt3):
    text = open(HEADER).read()
    assert re.search(r"#define RT3_ABI_VERSION 3u\b", text) and rt3.ABI_VERSION == 3 and rt3.lib().rt3_abi_version() == 3
    assert re.search(r"typedef struct rt3_aov_chain_params \{\s*/\* 16 bytes \*/", text)
    names = ["rt3_render_aov_specular", "rt3_render_aov_specular_device", "rt3_render_lens_aov_specular", "rt3_render_lens_aov_specular_device",
             "rt3_debug_aov_bounce"]
    for name in names:
        assert re.search(r"^int\s+%s\(" % name, text, re.M), name
        assert name in rt3.EXPORTS and hasattr(rt3.lib(), name)
        assert getattr(rt3.lib(), name).argtypes is not None
    for method in ("render_aov_specular", "render_aov_specular_device", "render_lens_aov_specular"):
        assert callable(getattr(rt3.HipRenderer, method))
    stubs = open(os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")).read()
    for name in names[:4]:
        assert re.search(r"^int %s\(" % name, stubs, re.M), name


def test_refusals_without_a_device(rt3):
    L = rt3.lib()
    v = (C.c_float * 4)(0.0, 0.0, -1.0, 0.0)
    n = (C.c_float * 3)(0.0, 0.0, 1.0)
    out = [(C.c_float * 3)() for _ in range(3)]
    fw = C.c_uint32(7)

    def call(chain, d=v, follow=fw):
        return L.rt3_debug_aov_bounce(d, v, n, 2, v, v, 0, C.byref(chain) if chain is not None else None, out[0], out[1], out[2],
                                      C.byref(follow) if follow is not None else None)
    P = rt3.rt3_aov_chain_params
    assert call(P(16, 0.0, 0, 0)) == 0 and fw.value in (0, 1)
    for bad in (None, P(17, 0.0, 0, 0), P(1, float("nan"), 0, 0), P(1, -0.5, 0, 0), P(1, float("inf"), 0, 0), P(1, 0.0, 1, 0), P(1, 0.0, 0, 1)):
        fw.value = 7
        assert call(bad) == E_ARG and fw.value == 7
    assert call(P(1, 0.0, 0, 0), d=None) == E_ARG and call(P(1, 0.0, 0, 0), follow=None) == E_ARG
    # the entry points without a context
    chain = P(1, 0.0, 0, 0)
    assert L.rt3_render_aov_specular(None, None, None, C.byref(chain), None) == E_ARG
    assert L.rt3_render_aov_specular_device(None, None, None, C.byref(chain), None, None) == E_ARG
    assert L.rt3_render_lens_aov_specular(None, None, None, C.byref(chain), None) == E_ARG
    assert L.rt3_render_lens_aov_specular_device(None, None, None, C.byref(chain), None, None) == E_ARG


# ---------------------------------------------------------------------------------------------- the command line's refusals (no device needed)
@pytest.mark.parametrize("args,message", [
    (("--spp", "4", "--aov-specular", "4", "--frames", "2", "o.ppm"), "--aov-specular is not available with --frames or --lens-frames"),
    (("--spp", "4", "--lens", "equirect", "--lens-frames", "2", "--aov-specular", "4", "o.ppm"), "--aov-specular is not available with --frames"),
    (("--aov-specular", "4", "o.ppm"), "--aov-specular needs the path tracer"),
    (("--spp", "4", "--aov-specular", "17", "o.ppm"), "at most 16 bounces"),
    (("--spp", "4", "--aov-specular", "4,-1", "o.ppm"), "Invalid aov-specular fuzz"),
    (("--spp", "4", "--aov-specular", "4,nan", "o.ppm"), "Invalid aov-specular fuzz"),
    (("--spp", "4", "--aov-specular"), "--aov-specular has no value."),
])
def test_cli_refusals(args, message):
    import subprocess
    exe = os.path.join(ROOT, "raytracer-3_amd", "rt3")
    p = subprocess.run([exe, *args], capture_output=True, text=True)
    assert p.returncode == 255 and message in p.stderr, (p.returncode, p.stderr)


def test_cli_help_lists_the_option():
    import subprocess
    p = subprocess.run([os.path.join(ROOT, "raytracer-3_amd", "rt3"), "-h"], capture_output=True, text=True)
    assert p.returncode == 0 and "--aov-specular" in p.stdout and "BOUNCES[,MAX_FUZZ]" in p.stdout
