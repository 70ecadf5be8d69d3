"""Header, binding, library and command line cover the emitters' sampling (RT3_FLAG_LIGHT_SAMPLING): the two test-only functions with the
declared signatures, the flag constant, the NULL-context and "no device" returns, the usage errors of --light-sampling, and an ABI version that stayed 3."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
SIGNATURES = {
    "rt3_debug_light_sample": [VP, U32, VP, U32, VP, VP, VP, U32, U32, U32, VP, VP, VP, VP, VP],
    "rt3_debug_light_table": [VP, VP, VP, U64, VP],
}


def p(a):
    return a.ctypes.data_as(VP)


def test_header_binding_and_library_cover_the_new_symbols(rt3):
    from test_abi import header_symbols
    names = header_symbols()
    L = rt3.lib()
    header = open(os.path.join(ROOT, "include", "rt3.h")).read()
    for s, args in SIGNATURES.items():
        assert s in names and s in rt3.EXPORTS and hasattr(L, s), s
        fn = getattr(L, s)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert "environment" not in s
    flat = re.sub(r"\s+", " ", header)
    assert ("int rt3_debug_light_sample(const rt3_gface* faces, uint32_t n_faces, const float* vertices_xyzw, uint32_t n_vertices, "
            "const rt3_material* face_materials, const float* center_radius, const rt3_material* sphere_materials, uint32_t n_spheres, "
            "uint32_t base, uint32_t depth, uint32_t* light, float point[3], float light_normal[3], float* area, float* pl);") in flat
    assert "int rt3_debug_light_table(rt3_ctx* ctx, uint32_t* q_out, uint64_t* cdf_out, uint64_t capacity, uint32_t* n_entries);" in flat
    assert "#define RT3_FLAG_LIGHT_SAMPLING    32u" in header and rt3.FLAG_LIGHT_SAMPLING == 32
    assert "#define RT3_FLAG_ENV_SAMPLING      16u" in header                       # the older flag is where it was
    assert L.rt3_abi_version() == 3 and rt3.ABI_VERSION == 3 and "RT3_ABI_VERSION 3u" in header     # a flag bit and functions: nothing else
    assert C.sizeof(rt3.rt3_params) == 44 and C.sizeof(rt3.RADIANCE_PARAMS) == 24
    assert "Emitters: sampling" in header and header.index("Emitters: sampling") > header.index("Environment map: sampling")


def test_python_surface(rt3):
    assert list(inspect.signature(rt3.light_sample).parameters) == ["faces", "verts", "face_materials", "center_radius", "sphere_materials", "base", "depth"]
    assert list(inspect.signature(rt3.HipRenderer.light_table).parameters) == ["self"]
    assert "FLAG_LIGHT_SAMPLING" in rt3.HipRenderer.radiance.__doc__
    with pytest.raises(rt3.Fatal):                                                 # one material per sphere
        rt3.light_sample(None, None, None, np.zeros((2, 4), np.float32), np.zeros(1, rt3.MATERIAL), 1, 0)


def test_refusals_that_need_no_device(rt3, tmp_path):
    L = rt3.lib()
    faces = np.zeros(1, rt3.GFACE)
    faces["v2"], faces["v3"] = 1, 2
    verts = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32)
    fm = np.zeros(1, rt3.MATERIAL)
    fm["rgb"] = 1.0
    cr = np.array([[0, 0, 3, 1]], np.float32)
    sm = np.zeros(1, rt3.MATERIAL)
    sm["rgb"] = 1.0
    light, point, normal = np.full(1, 9, np.uint32), np.full(3, 9.0, np.float32), np.full(3, 9.0, np.float32)
    area, pl = np.full(1, 9.0, np.float32), np.full(1, 9.0, np.float32)
    outs = (p(light), p(point), p(normal), p(area), p(pl))
    fn = L.rt3_debug_light_sample
    assert fn(p(faces), 1, p(verts), 3, p(fm), p(cr), p(sm), 1, 1, 0, *outs) == 0 and light[0] < 2 and pl[0] > 0 and area[0] > 0
    assert fn(None, 0, None, 0, None, p(cr), p(sm), 1, 1, 0, *outs) == 0 and light[0] == 0        # a class that is absent may be NULL
    assert fn(p(faces), 1, p(verts), 3, p(fm), None, None, 0, 1, 0, *outs) == 0 and light[0] == 0
    assert fn(None, 0, None, 0, None, None, None, 0, 1, 0, *outs) == 0 and light[0] == 0xFFFFFFFF and pl[0] == 0     # the empty table
    light[:], point[:], normal[:], area[:], pl[:] = 9, 9.0, 9.0, 9.0, 9.0
    bad = faces.copy()
    bad["v3"] = 3
    for args in ((None, 1, p(verts), 3, p(fm), p(cr), p(sm), 1), (p(faces), 1, None, 3, p(fm), p(cr), p(sm), 1),
                 (p(faces), 1, p(verts), 3, None, p(cr), p(sm), 1), (p(faces), 1, p(verts), 3, p(fm), None, p(sm), 1),
                 (p(faces), 1, p(verts), 3, p(fm), p(cr), None, 1), (p(bad), 1, p(verts), 3, p(fm), p(cr), p(sm), 1),
                 (p(faces), 1, p(verts), 2, p(fm), p(cr), p(sm), 1)):
        assert fn(*args, 1, 0, *outs) == -1, args                                      # RT3_E_ARG
    for k in range(5):
        assert fn(p(faces), 1, p(verts), 3, p(fm), p(cr), p(sm), 1, 1, 0, *[None if i == k else o for i, o in enumerate(outs)]) == -1, k
    assert light[0] == 9 and point.tolist() == [9, 9, 9] and normal.tolist() == [9, 9, 9] and area[0] == 9 and pl[0] == 9      # a refused call writes nothing
    n = C.c_uint32(0)
    q, cdf = np.zeros(4, np.uint32), np.zeros(4, np.uint64)
    assert L.rt3_debug_light_table(None, p(q), p(cdf), 4, C.byref(n)) == -1             # RT3_E_ARG, as every entry point refuses a NULL context
    so = tmp_path / "libstubs.so"
    subprocess.check_call(["g++", "-shared", "-fPIC", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                           os.path.join(ROOT, "tools", "asan", "device_stubs.cpp")])
    stub = C.CDLL(str(so)).rt3_debug_light_table
    stub.restype = C.c_int
    assert stub(C.c_void_p(0x10), p(q), p(cdf), C.c_uint64(4), C.byref(n)) == -2        # RT3_E_DEVICE: "no device"


def test_cli_usage_errors():
    from test_cli import run
    rc, out, err = run("--light-sampling", "o.png")                                # the built-in scene without --spp is Mode R
    assert rc == -1 and "--light-sampling needs the path tracer (Mode X): pass --spp." in err, err
    rc, out, err = run("--scene", "three", "--spp", "4", "--env", "e.pfm", "--env-sampling", "--light-sampling", "o.png")
    assert rc == -1 and "--light-sampling is not available with --env-sampling." in err, err
    rc, out, err = run("--scene", "three", "--spp", "8", "--adaptive", "0.05", "--light-sampling", "o.png")
    assert rc == -1 and "--light-sampling is not available with --adaptive." in err, err
    rc, out, err = run("-h")
    assert rc == 0 and "--light-sampling" in out
