"""Scene updates (rt3_update_spheres*, rt3_update_mesh*) on the GPU: an update equals a full upload byte for byte
on every entry point, a refit of the same scene reproduces the build's counters, a scene that drifted far stays correct, chained updates and
the command line's --refit, the device / torch forms (no allocation, no host synchronisation), bad records, errors and state."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_denoise import set_mesh, set_spheres
from test_gpu_motion import slid, tessellated_sphere
from test_gpu_temporal import orbit_camera

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")
F = np.float32
E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def other(rt3, renderer):
    """A second context on the same device: the one that takes the full upload."""
    r = rt3.initialize_renderer(0)
    yield r
    r.close()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def stress_camera(rt3, w, h):
    """The camera the benchmarks look at scene_stress with."""
    return rt3.Camera().look_at(w, h, (0.0, 8.0, 12.0), (0.0, 6.0, -50.0), (0.0, 1.0, 0.0), 45.0, 1.0)


def with_normals(faces, verts):
    """The faces with the stored normal recomputed from the vertices (what a deforming mesh passes to update_mesh)."""
    f = faces.copy()
    p1, p2, p3 = (verts[f[k]][:, :3].astype(np.float64) for k in ("v1", "v2", "v3"))
    n = np.cross(p3 - p1, p2 - p1)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    f["normal"] = np.where(length > 0, n / np.where(length > 0, length, 1.0), faces["normal"]).astype(F)
    return f


def moved_spheres(cr):
    out = slid(cr, 1)
    out[5::7, 3] *= F(1.25)                                             # some rescaled (movers and others)
    out[8::11, 3] *= F(0.75)
    return out


def scene_pair(rt3, name):
    """(A, B, camera, flags, frame size): A and B as dicts of spheres / smats / faces / verts / fmats; B is A moved."""
    rng = np.random.default_rng(11)
    w, h, flags = 128, 96, 0
    A, B = {}, {}
    if name in ("weekend", "mixed"):
        cr, mats = rt3.scene_weekend(42)
        A.update(spheres=cr, smats=mats)
        B.update(spheres=moved_spheres(cr), smats=mats)
        cam = orbit_camera(rt3, w, h, 2.0)
    if name in ("stress4k", "stress120k"):
        cr, mats = rt3.scene_stress(4000 if name == "stress4k" else 120000, 43)
        A.update(spheres=cr, smats=mats)
        B.update(spheres=moved_spheres(cr), smats=mats)
        if name == "stress120k":
            w, h = 96, 72
        cam = stress_camera(rt3, w, h)
    if name == "cornell":
        faces, verts, fm = rt3.scene_cornell(16)
        v = verts.copy()
        third = len(v) // 3 // 3 * 3
        v[third:2 * third, :3] += rng.normal(0.0, 0.02, (third, 3)).astype(F)
        A.update(faces=faces, verts=verts, fmats=fm)
        B.update(faces=faces, verts=v, fmats=fm)
        cam, flags = rt3.main_camera(w, h), rt3.FLAG_BLACK_BACKGROUND
    if name in ("sphere_entity", "mixed"):
        at = (6.0, 0.6, 2.0) if name == "mixed" else (0.0, 0.0, -3.0)
        faces, verts = tessellated_sphere(rt3, at, 0.6)
        v = verts.copy()
        moved = rng.random(len(v)) < 0.5
        v[moved, :3] += rng.normal(0.0, 0.03, (int(moved.sum()), 3)).astype(F)
        A.update(faces=faces, verts=verts, fmats=None)
        B.update(faces=with_normals(faces, v), verts=v, fmats=None, new_faces=True)        # a morphing entity passes its new normals
        if name == "sphere_entity":
            cam = rt3.main_camera(w, h)
    return A, B, cam, flags, (w, h)


def upload(rt3, r, S):
    if "faces" in S:
        r.set_mesh(S["faces"], S["verts"], S["fmats"])
    else:
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    if "spheres" in S:
        r.set_spheres(S["spheres"], S["smats"])
    else:
        r.set_spheres(np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))


def update(r, S):
    if "faces" in S:
        r.update_mesh(S["verts"], S["faces"] if S.get("new_faces") else None)
    if "spheres" in S:
        r.update_spheres(S["spheres"])


def outputs(rt3, r, A, cam, flags, size, mode_r):
    """Everything the contract names, as bytes: path render, Mode R, AOVs, queries on the camera rays, the motion plane against A, and the
    path render through the unfiltered kernel."""
    w, h = size
    p = rt3.make_params(w, h, spp=3, max_depth=4, seed=5, flags=flags)
    p1 = rt3.make_params(w, h, spp=1, max_depth=1, seed=5, flags=flags)
    out = {"path": r.render_path(cam.c, p).tobytes()}
    if mode_r:
        frame = np.zeros((h, w), np.uint32)
        r._check(rt3.lib().rt3_render(r._ctx, C.byref(cam.c), w, h, ptr(frame)))
        out["mode_r"] = frame.tobytes()
    aov = r.render_aov(cam.c, p1)
    out["aov"] = aov.tobytes()
    rays = r.camera_rays(cam.c, p1)
    out["intersect"] = r.intersect(rays).tobytes()
    out["occluded"] = r.occluded(rays).tobytes()
    out["motion"] = r.motion(aov, cam.c, prev_center_radius=A.get("spheres"), prev_vertices=A.get("verts")).tobytes()
    r.force_brute(True)
    try:
        out["brute"] = r.render_path(cam.c, p).tobytes()
    finally:
        r.force_brute(False)
    return out


# ------------------------------------------------------------------------------------------------ 1: update equals upload
@pytest.mark.parametrize("scene", ["weekend", "stress4k", "stress120k", "cornell", "sphere_entity", "mixed"])
def test_an_update_equals_a_full_upload_bit_for_bit(rt3, renderer, other, scene):
    A, B, cam, flags, size = scene_pair(rt3, scene)
    upload(rt3, renderer, A)
    update(renderer, B)
    upload(rt3, other, B)
    mode_r = "faces" in A and "spheres" not in A and scene != "mixed"
    got = outputs(rt3, renderer, A, cam, flags, size, mode_r)
    want = outputs(rt3, other, A, cam, flags, size, mode_r)
    upload(rt3, other, A)
    unmoved = outputs(rt3, other, A, cam, flags, size, mode_r)
    for k in want:
        print("%s %s: %d bytes, equal %s" % (scene, k, len(want[k]), got[k] == want[k]))
    for k in want:
        assert got[k] == want[k], (scene, k)
    assert want["path"] == want["brute"] and got["path"] != unmoved["path"]            # the filter agrees with the arbiter; B is not A
    assert np.frombuffer(want["motion"], F).any()


def test_an_updated_scene_equals_the_cpu_oracle(rt3, renderer, oracle):
    O = oracle
    cr, mats = rt3.scene_three_spheres()
    B = cr.copy()
    B[0, :3] += np.array([0.2, 0.1, -0.15], F)
    B[1, 3] *= F(0.8)
    set_spheres(rt3, renderer, cr, mats)
    renderer.update_spheres(B)
    w, h = 96, 54
    cam = rt3.Camera().update(w, h, 1.0, F(w) / F(h) * F(2.0), 2.0)
    got = renderer.render_path(cam.c, rt3.make_params(w, h, spp=4, max_depth=4, seed=7, flags=rt3.FLAG_GAMMA2))
    ocam = O.Camera()
    for f in ("origin", "horizontal", "vertical", "lower_left_corner"):
        setattr(ocam, f, getattr(cam.c, f))
    ref, _ = O.render_path(ocam, O.make_params(w, h, spp=4, max_depth=4, seed=7, flags=O.FLAG_GAMMA2), spheres=B, smats=mats.view(O.MATERIAL))
    assert np.array_equal(got, ref), int((got != ref).sum())


# ------------------------------------------------------------------------------------------------ 2: the refit reproduces the build
COUNTERS = ("ray_casts", "filter_tests", "exact_tests", "bound_tests", "mfma_instructions")


@pytest.mark.parametrize("scene", ["weekend", "weekend_k64", "stress4k", "stress120k", "cornell", "mixed"])
def test_a_refit_of_the_same_scene_reproduces_the_builds_counters(rt3, renderer, scene):
    name = "weekend" if scene == "weekend_k64" else scene
    A, _, cam, flags, (w, h) = scene_pair(rt3, name)
    if scene == "weekend_k64":
        os.environ["RT3_MFMA_K64"] = "1"                                  # the K = 64 rows of the flat filter (d_sph_frag)
    try:
        upload(rt3, renderer, A)
        p = rt3.make_params(w, h, spp=2, max_depth=4, seed=9, flags=flags)
        first = renderer.render_path(cam.c, p)
        s1 = renderer.stats()
        update(renderer, A)
        second = renderer.render_path(cam.c, p)
        s2 = renderer.stats()
    finally:
        os.environ.pop("RT3_MFMA_K64", None)
    c1, c2 = [getattr(s1, k) for k in COUNTERS], [getattr(s2, k) for k in COUNTERS]
    print(scene, dict(zip(COUNTERS, c1)), dict(zip(COUNTERS, c2)))
    assert first.tobytes() == second.tobytes()
    assert c1 == c2 and s1.mfma_instructions > 0 and (s1.exact_tests > 0 or scene == "weekend_k64")      # (the K = 64 kernel keeps no pair list)


# ------------------------------------------------------------------------------------------------ 3: far drift
def test_a_scene_that_drifted_far_stays_correct(rt3, renderer, other):
    w, h = 96, 72
    off = np.array([6000.0, 0.0, 0.0], F)
    A, B, _, _, _ = scene_pair(rt3, "weekend")
    far = B["spheres"].copy()
    far[:, :3] += off
    upload(rt3, renderer, A)
    renderer.update_spheres(far)
    upload(rt3, other, dict(spheres=far, smats=B["smats"]))
    cam = rt3.Camera().look_at(w, h, (13.0 + 6000.0, 2.0, 3.0), (6000.0, 0.0, 0.0), vfov=20.0, focus_dist=10.0)
    p = rt3.make_params(w, h, spp=2, max_depth=4, seed=4)
    got, want = renderer.render_path(cam.c, p), other.render_path(cam.c, p)
    assert got.tobytes() == want.tobytes() and len(np.unique(want)) > 50

    A, B, cam, flags, _ = scene_pair(rt3, "cornell")
    far = B["verts"].copy()
    far[:, :3] += off
    upload(rt3, renderer, A)
    renderer.update_mesh(far)
    upload(rt3, other, dict(faces=B["faces"], verts=far, fmats=B["fmats"]))
    cam = rt3.main_camera(w, h)
    cam.c.origin[0] += 6000.0
    cam.c.lower_left_corner[0] += 6000.0
    p = rt3.make_params(w, h, spp=2, max_depth=4, seed=4, flags=flags)
    got, want = renderer.render_path(cam.c, p), other.render_path(cam.c, p)
    assert got.tobytes() == want.tobytes() and len(np.unique(want)) > 10


# ------------------------------------------------------------------------------------------------ 4: chained updates, the command line
def test_eight_chained_updates_equal_eight_fresh_uploads(rt3, renderer, other):
    w, h = 96, 72
    cr, mats = rt3.scene_stress(4000, 43)
    set_spheres(rt3, renderer, cr, mats)
    cam = stress_camera(rt3, w, h)
    for k in range(1, 9):
        cur = slid(cr, k)
        renderer.update_spheres(cur)
        set_spheres(rt3, other, cur, mats)
        p = rt3.make_params(w, h, spp=1, max_depth=8, seed=30 + k)
        got, want = renderer.render_path(cam.c, p), other.render_path(cam.c, p)
        assert got.tobytes() == want.tobytes(), k
    first = other.render_path(cam.c, p)
    set_spheres(rt3, other, cr, mats)
    assert other.render_path(cam.c, p).tobytes() != first.tobytes()      # the spheres did move


def test_the_command_lines_refit_sequence_is_byte_equal(tmp_path):
    w, h = 96, 72
    args = [EXE, "--scene", "weekend", "--spp", "1", "-W", str(w), "-H", str(h), "-f", "ppm", "--frames", "4", "--slide", "-0.1,0,0.05",
            "--denoise", "P"]
    dirs = []
    for extra in ((), ("--refit",)):
        d = tmp_path / ("refit" if extra else "upload")
        d.mkdir()
        subprocess.run(args + list(extra) + ["out.ppm"], cwd=str(d), check=True, capture_output=True, timeout=300)
        dirs.append(d)
    names = sorted(f.name for f in dirs[0].iterdir())
    assert names == sorted(f.name for f in dirs[1].iterdir()) and "P.3.pfm" in names and "out.ppm" in names
    for n in names:
        assert (dirs[0] / n).read_bytes() == (dirs[1] / n).read_bytes(), n
    assert (dirs[0] / "P.0.pfm").read_bytes() != (dirs[0] / "P.3.pfm").read_bytes()


# ------------------------------------------------------------------------------------------------ 5: device and torch forms
def test_the_torch_form_on_another_stream_allocates_nothing_and_equals_the_host_form(rt3, renderer, other):
    import torch
    w, h = 96, 72
    cr, mats = rt3.scene_stress(4000, 43)
    B = moved_spheres(cr)
    cam = stress_camera(rt3, w, h)
    p = rt3.make_params(w, h, spp=2, max_depth=4, seed=6)
    set_spheres(rt3, other, cr, mats)
    other.update_spheres(B)                                               # the host form
    want = other.render_path(cam.c, p)

    set_spheres(rt3, renderer, cr, mats)
    dev = torch.device("cuda", 0)
    frames = [torch.from_numpy(slid(B, k)).to(dev) for k in range(12)]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        renderer.update_spheres(frames[1])                                # warm-up
        free0 = torch.cuda.mem_get_info(dev)[0]
        for k in range(2, 12):
            renderer.update_spheres(frames[k])
        free1 = torch.cuda.mem_get_info(dev)[0]
        renderer.update_spheres(frames[0])                                # B itself, queued on the side stream ...
    got = renderer.render_path(cam.c, p)                                  # ... and rendered on the context's, with no host synchronisation between
    assert got.tobytes() == want.tobytes()
    assert free1 == free0, (free0, free1)
    big, big_mats = rt3.scene_stress(400000, 44)
    renderer.set_spheres(big, big_mats)                                   # the probe does see hipMalloc
    free2 = torch.cuda.mem_get_info(dev)[0]
    print("free device memory: %d before ten updates, %d after, %d after a set_spheres of 400 000" % (free0, free1, free2))
    assert free2 < free1

    # the mesh form: device vertices and faces on the side stream
    A, Bm, camm, flags, (w, h) = scene_pair(rt3, "sphere_entity")
    upload(rt3, other, Bm)
    pm = rt3.make_params(w, h, spp=2, max_depth=2, seed=6, flags=flags)
    want = other.render_path(camm.c, pm)
    upload(rt3, renderer, A)
    tv = torch.from_numpy(Bm["verts"]).to(dev)
    tf = torch.from_numpy(Bm["faces"].view(np.uint8).reshape(-1, 48)).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        renderer.update_mesh(tv, tf)
    got = renderer.render_path(camm.c, pm)
    renderer.synchronize()                                                # (no face index was out of range)
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ 6: bad records
def test_bad_records_become_spheres_nothing_can_hit(rt3, renderer, other):
    import torch
    w, h = 128, 96
    cr, mats = rt3.scene_weekend(42)
    mats = mats.copy()
    mats["kind"] = rt3.MAT_FLAT                                           # flat materials, depth 1, black background: a pixel shows its first hit
    cam = rt3.weekend_camera(w, h)
    p = rt3.make_params(w, h, spp=2, max_depth=1, seed=8, flags=rt3.FLAG_BLACK_BACKGROUND)
    set_spheres(rt3, renderer, cr, mats)
    before = renderer.render_path(cam.c, p)
    aov = renderer.render_aov(cam.c, p)
    seen = [int(i) for i in np.unique(aov["index"][aov["kind"] == rt3.HIT_SPHERE]) if i not in (0,)][:2]    # two visible spheres (not the ground)
    assert len(seen) == 2
    bad = cr.copy()
    bad[seen[0], 3] = 0.0
    bad[seen[1], 0] = np.nan
    gone = cr.copy()
    for k, i in enumerate(seen):
        gone[i] = (1e6 + k, 1e6, 1e6, 1e-3)                               # tiny, far outside the view
    renderer.update_spheres(torch.from_numpy(bad).to("cuda:0"))
    got = renderer.render_path(cam.c, p)
    motion = renderer.motion(aov, cam.c, prev_center_radius=cr)           # (runs; the records are reported as given)
    assert motion.shape == (h, w, 4)
    set_spheres(rt3, other, gone, mats)
    want = other.render_path(cam.c, p)
    assert got.tobytes() == want.tobytes() and got.tobytes() != before.tobytes()
    renderer.force_brute(True)
    try:
        assert renderer.render_path(cam.c, p).tobytes() == want.tobytes()
    finally:
        renderer.force_brute(False)
    # the host form refuses, and the scene is untouched
    set_spheres(rt3, renderer, cr, mats)
    assert rt3.lib().rt3_update_spheres(renderer._ctx, ptr(bad), len(bad)) == E_ARG
    assert renderer.render_path(cam.c, p).tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------------ 7: errors and state
def test_errors_and_state(rt3, renderer, other):
    import torch
    L = rt3.lib()
    cr, mats = rt3.scene_weekend(42)
    faces, verts = tessellated_sphere(rt3, (0.0, 0.0, -3.0), 0.6)
    fresh = rt3.initialize_renderer(0)
    try:
        assert L.rt3_update_spheres(fresh._ctx, ptr(cr), len(cr)) == E_STATE           # no scene
        assert L.rt3_update_mesh(fresh._ctx, None, ptr(verts), len(verts)) == E_STATE
    finally:
        fresh.close()
    renderer.set_mesh(faces, verts)
    renderer.set_spheres(cr, mats)
    ctx = renderer._ctx
    assert L.rt3_update_spheres(ctx, ptr(cr), len(cr) - 1) == E_ARG                    # wrong counts
    assert L.rt3_update_spheres(ctx, None, len(cr)) == E_ARG
    assert L.rt3_update_mesh(ctx, None, ptr(verts), len(verts) + 1) == E_ARG
    assert L.rt3_update_mesh(ctx, None, None, len(verts)) == E_ARG
    t = torch.zeros(4 * len(cr) + 4, dtype=torch.float32, device="cuda:0")
    assert L.rt3_update_spheres_device(ctx, C.c_void_p(t.data_ptr() + 4), len(cr), None) == E_ARG     # misaligned
    tv = torch.zeros(4 * len(verts) + 4, dtype=torch.float32, device="cuda:0")
    assert L.rt3_update_mesh_device(ctx, None, C.c_void_p(tv.data_ptr() + 4), len(verts), None) == E_ARG
    assert L.rt3_update_spheres(ctx, ptr(cr), len(cr)) == 0 and L.rt3_update_mesh(ctx, None, ptr(verts), len(verts)) == 0
    # a face index out of range: the host form refuses and leaves no mesh, as rt3_set_mesh does
    broken = faces.copy()
    broken["v2"][3] = len(verts)
    assert L.rt3_update_mesh(ctx, ptr(broken), ptr(verts), len(verts)) == E_ARG
    assert L.rt3_update_mesh(ctx, None, ptr(verts), len(verts)) == E_STATE
    # the device form keeps the scene (that face cannot be hit) and the next rt3_synchronize reports it, once
    renderer.set_mesh(faces, verts)
    tb = torch.from_numpy(broken.view(np.uint8).reshape(-1, 48)).to("cuda:0")
    tverts = torch.from_numpy(verts).to("cuda:0")
    torch.cuda.synchronize()
    assert L.rt3_update_mesh_device(ctx, C.c_void_p(tb.data_ptr()), C.c_void_p(tverts.data_ptr()), len(verts), None) == 0
    assert L.rt3_synchronize(ctx) == E_ARG and L.rt3_synchronize(ctx) == 0
    hole = renderer.intersect(renderer.camera_rays(rt3.main_camera(64, 48).c, rt3.make_params(64, 48)))
    assert 3 not in set(hole["index"][hole["kind"] == rt3.HIT_FACE])
    # entity buffers out of sync with the commit
    renderer.set_mesh(faces, verts)
    assert L.rt3_mesh_begin(ctx, len(faces), len(verts)) == 0
    assert L.rt3_update_mesh(ctx, None, ptr(verts), len(verts)) == E_STATE
    renderer.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    # a non-finite sphere at set time has no slot an update could fill
    odd = cr.copy()
    odd[7, 1] = np.inf
    renderer.set_spheres(odd, mats)
    assert L.rt3_update_spheres(ctx, ptr(cr), len(cr)) == E_STATE
    renderer.set_spheres(cr, mats)
    assert L.rt3_update_spheres(ctx, ptr(cr), len(cr)) == 0


def test_a_range_render_across_an_update_behaves_as_across_a_full_upload(rt3, renderer, other):
    w, h = 96, 72
    cr, mats = rt3.scene_weekend(42)
    B = moved_spheres(cr)
    cam = rt3.weekend_camera(w, h)
    p = rt3.make_params(w, h, spp=4, max_depth=4, seed=2)
    L = rt3.lib()
    results = []
    for r, change in ((renderer, lambda: renderer.update_spheres(B)), (other, lambda: other.set_spheres(B, mats))):
        set_spheres(rt3, r, cr, mats)
        out = np.zeros((h, w), np.uint32)
        rc0 = L.rt3_render_path_range(r._ctx, C.byref(cam.c), C.byref(p), 0, 2, ptr(out))
        change()
        rc1 = L.rt3_render_path_range(r._ctx, C.byref(cam.c), C.byref(p), 2, 2, ptr(out))
        results.append((rc0, rc1, out.tobytes()))
    assert results[0] == results[1] and results[0][0] == 0


# ------------------------------------------------------------------------------------------------ host form = device form, optional inputs present and absent
def test_update_mesh_with_and_without_faces(rt3, renderer):
    from test_gpu_host_forms import F, dev, mixed_scene
    _, faces, verts, cam, p = mixed_scene(rt3, renderer)
    v2 = verts.copy()
    v2[:, :3] += F(0.07)
    f2 = faces[::-1].copy()                                            # the two faces' records swapped: other indices, normals and colours
    for f in (None, f2):
        mixed_scene(rt3, renderer)
        renderer.update_mesh(v2, faces=f)
        want = [a.tobytes() for a in renderer.mesh_download()] + [renderer.render_aov(cam.c, p).tobytes(), renderer.render_path(cam.c, p).tobytes()]
        mixed_scene(rt3, renderer)
        renderer.update_mesh(dev(v2), faces=None if f is None else dev(f))
        renderer.synchronize()
        got = [a.tobytes() for a in renderer.mesh_download()] + [renderer.render_aov(cam.c, p).tobytes(), renderer.render_path(cam.c, p).tobytes()]
        assert got == want, f is not None
    mixed_scene(rt3, renderer)                                         # (a host-form scene again: regroup() and friends leave torch's stream)
