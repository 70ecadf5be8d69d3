"""rt3_regroup*  on the GPU: a regroup changes nothing any entry point returns, the order is the specified one word
for word, it is the host's split where that is unique, it undoes what refits let go stale, the event chain and the state rules, and the
command line's --regroup."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import regroup_ref as G
from test_gpu_denoise import set_mesh, set_spheres
from test_gpu_update import outputs, ptr, scene_pair, stress_camera, update, upload
from test_gpu_motion import tessellated_sphere

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracer-3_amd", "rt3")
F = np.float32
E_ARG, E_STATE = -1, -4
SPH, MESH = 1, 2
COUNTERS = ("filter_tests", "bound_tests", "exact_tests", "mfma_instructions")


@pytest.fixture(scope="module")
def other(rt3, renderer):
    """A second context on the same device: the one that takes the full upload."""
    r = rt3.initialize_renderer(0)
    yield r
    r.close()


def random_rays(rt3, lo, hi, n, seed):
    """Rays from points around the box [lo, hi] towards points inside it."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    mid, ext = (lo + hi) / 2, (hi - lo)
    o = (mid + rng.normal(0.0, 1.0, (n, 3)) * ext).astype(F)
    t = rng.uniform(lo, hi, (n, 3)).astype(F)
    return rt3.make_rays(o, t - o)


def scene_box(S):
    pts = []
    if "spheres" in S:
        pts.append(S["spheres"][:, :3])
    if "verts" in S:
        pts.append(S["verts"][:, :3])
    pts = np.concatenate(pts)
    lo, hi = np.percentile(pts, 2, axis=0), np.percentile(pts, 98, axis=0)      # (the ground sphere's centre is far below)
    return lo, np.maximum(hi, lo + 1.0)


def distinct_scene(rt3, n=20000, seed=3):
    """Spheres that share no coordinate value on any axis: each axis a random permutation of n multiples of 2^-9, small equal radii.
    A median split of such a scene has one answer: every cut is decided by values that differ."""
    rng = np.random.default_rng(seed)
    cr = np.empty((n, 4), F)
    for a in range(3):
        cr[:, a] = rng.permutation(n).astype(F) * F(2.0 ** -9)
    cr[:, 3] = F(0.05)
    mats = np.zeros(n, rt3.MATERIAL)
    mats["kind"] = rt3.MAT_LAMBERT
    mats["rgb"] = rng.uniform(0.2, 0.9, (n, 3)).astype(F)
    return cr, mats


# per frame: (50, 10, -25) lattice steps and 1/128 of one, about (0.1, 0.02, -0.05).  After 64 frames the odd spheres sit half a step off the
# lattice the even ones are on, and every sum is exact in f32: no two coordinates collide in the final positions.
SLIDE = tuple(F(s * (abs(m) + 1.0 / 128.0) * 2.0 ** -9) for m, s in ((50, 1), (10, 1), (25, -1)))


def slid_exact(cr, k):
    out = cr.copy()
    out[1::2, :3] += (F(k) * np.array(SLIDE, F)).astype(F)
    return out


def distinct_camera(rt3, w, h):
    return rt3.Camera().look_at(w, h, (20.0, 30.0, 110.0), (20.0, 20.0, 20.0), (0.0, 1.0, 0.0), 35.0, 1.0)


def member_tests(st):
    return st.bound_tests + st.exact_tests


# ------------------------------------------------------------------------------------------------ 1: same results
@pytest.mark.parametrize("scene,env", [("weekend", {}), ("stress4k", {}), ("stress4k", {"RT3_NO_RESIDENT": "1"}), ("stress4k", {"RT3_LEVELS": "3"}),
                                       ("stress4k", {"RT3_LEVELS": "4"}), ("cornell", {}), ("mixed", {})])
def test_a_regroup_changes_nothing_any_entry_point_returns(rt3, renderer, other, scene, env, monkeypatch):
    A, B, cam, flags, size = scene_pair(rt3, scene)
    upload(rt3, renderer, A)
    update(renderer, B)
    renderer.regroup()
    upload(rt3, other, B)                                                 # (B carries A's materials)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mode_r = scene == "cornell"
    got = outputs(rt3, renderer, A, cam, flags, size, mode_r)
    want = outputs(rt3, other, A, cam, flags, size, mode_r)
    rays = random_rays(rt3, *scene_box(B), 20000, 17)
    got.update(random_intersect=renderer.intersect(rays).tobytes(), random_occluded=renderer.occluded(rays).tobytes())
    want.update(random_intersect=other.intersect(rays).tobytes(), random_occluded=other.occluded(rays).tobytes())
    for k in want:
        print("%s %s %s: %d bytes, equal %s" % (scene, env, k, len(want[k]), got[k] == want[k]))
    for k in want:
        assert got[k] == want[k], (scene, k)
    assert want["path"] == want["brute"]                                  # the unfiltered kernel agrees
    hits = np.frombuffer(want["random_intersect"], rt3.HIT)
    assert (hits["kind"] != rt3.HIT_NONE).sum() > 100                      # the random rays do meet the scene


# ------------------------------------------------------------------------------------------------ 2: the specified order
@pytest.mark.parametrize("n", [700, 4097, 20000])
def test_the_sphere_order_is_the_specified_one(rt3, renderer, n):
    """700: one k_split_lds workgroup; 4097: one level above the LDS limit; 20 000: three."""
    rng = np.random.default_rng(n)
    cr = np.empty((n, 4), F)
    cr[:, :3] = rng.uniform(-40.0, 40.0, (n, 3)).astype(F) * np.array([1.0, 0.4, 1.7], F)
    cr[:, 3] = F(0.1)
    mats = np.zeros(n, rt3.MATERIAL)
    mats["kind"], mats["rgb"] = rt3.MAT_LAMBERT, (0.5, 0.5, 0.5)
    set_spheres(rt3, renderer, cr, mats)
    before = renderer.group_order(SPH)
    ids = before[before != G.PAD]
    assert len(ids) == n and len(before) == -(-n // 64) * 64
    B = cr.copy()
    B[:, :3] += rng.normal(0.0, 6.0, (n, 3)).astype(F)
    B[::5, 0] = np.round(B[::5, 0])                                       # some ties, and both zeros
    B[3::50, 1] = F(0.0)
    B[4::50, 1] = F(-0.0)
    renderer.update_spheres(B)
    assert np.array_equal(renderer.group_order(SPH), before)              # an update keeps the order
    renderer.regroup()
    got = renderer.group_order(SPH)
    want = G.padded(G.regroup_order(ids, G.sphere_centres(B)))
    print("n = %d: %d positions, %d differ from the restatement; %d moved" % (n, len(got), int((got != want).sum()), int((got != before).sum())))
    assert np.array_equal(got, want) and not np.array_equal(got, before)
    renderer.regroup()                                                    # nothing changed in between: the order stays
    assert np.array_equal(renderer.group_order(SPH), want)


@pytest.mark.parametrize("perturbed", [True, False])
def test_the_face_order_is_the_specified_one(rt3, renderer, perturbed):
    """cornell(16): the bounds' centres sit on a grid, so ties are frequent and the stable rule decides; perturbed: every vertex moved."""
    faces, verts, fm = rt3.scene_cornell(16)
    set_mesh(rt3, renderer, faces, verts, fm)
    before = renderer.group_order(MESH)
    ids = before[before != G.PAD]
    assert len(ids) == len(faces) and len(before) == -(-len(faces) // 64) * 64      # no face without a bounded hit region: no tail
    v = verts.copy()
    if perturbed:
        v[:, :3] += np.random.default_rng(8).normal(0.0, 0.03, (len(v), 3)).astype(F)
        renderer.update_mesh(v)
    renderer.regroup()
    got = renderer.group_order(MESH)
    centres = G.face_centres(faces, v)
    want = G.padded(G.regroup_order(ids, centres))
    ties = len(centres) * 3 - sum(len(np.unique(centres[:, a])) for a in range(3))
    print("cornell(16) perturbed=%s: %d positions, %d differ from the restatement; %d repeated coordinate values" % (perturbed, len(got), int((got != want).sum()), ties))
    assert np.array_equal(got, want)
    assert perturbed or ties > len(centres)


def test_a_mesh_above_the_lds_limit_and_faces_that_lost_their_bound(rt3, renderer, other):
    """cornell(24) is more than 4096 faces: the faces go through k_part_box / k_part_keys / the pair sort before k_split_lds.  Then an update
    collapses some faces to a point: their bound is no longer usable and they are sorted by the filter centre, the middle of the vertex box
    at commit time."""
    faces, verts, fm = rt3.scene_cornell(24)
    assert len(faces) > 4096
    set_mesh(rt3, renderer, faces, verts, fm)
    before = renderer.group_order(MESH)
    ids = before[before != G.PAD]
    assert len(ids) == len(faces) and len(before) == -(-len(faces) // 64) * 64
    centre = G.mesh_filter_centre(verts)
    renderer.regroup()                                                    # the grid as it is: ties on every axis
    want = G.padded(G.regroup_order(ids, G.face_centres(faces, verts, centre)))
    got = renderer.group_order(MESH)
    print("cornell(24): %d faces, %d positions differ from the restatement" % (len(faces), int((got != want).sum())))
    assert np.array_equal(got, want)
    rng = np.random.default_rng(12)
    v = verts.copy()
    v[:, :3] += rng.normal(0.0, 0.02, (len(v), 3)).astype(F)
    for f in rng.choice(len(faces), 40, replace=False):                   # forty faces collapse to their first vertex (and take neighbours along)
        v[faces["v2"][f], :3] = v[faces["v1"][f], :3]
        v[faces["v3"][f], :3] = v[faces["v1"][f], :3]
    centres = G.face_centres(faces, v, centre)
    lost = int((centres == centre).all(axis=1).sum())
    renderer.update_mesh(v)
    renderer.regroup()
    got = renderer.group_order(MESH)
    want = G.padded(G.regroup_order(ids, centres))
    print("after the update: %d faces without a usable bound, %d positions differ from the restatement" % (lost, int((got != want).sum())))
    assert lost >= 40 and np.array_equal(got, want)
    set_mesh(rt3, other, faces, v, fm)                                    # and nothing a render returns depends on it
    w, h = 96, 72
    cam, p = rt3.main_camera(w, h), rt3.make_params(w, h, spp=2, max_depth=4, seed=3, flags=rt3.FLAG_BLACK_BACKGROUND)
    assert renderer.render_path(cam.c, p).tobytes() == other.render_path(cam.c, p).tobytes()


def test_spheres_an_update_turned_into_pads_are_sorted_by_the_filter_centre(rt3, renderer, other):
    """The device form cannot refuse a record: r <= 0 or a non-finite value makes the sphere a pad, and the regroup sorts it by the filter
    centre, the component-wise median of the centres at rt3_set_spheres time.  5000 spheres: one level above the LDS limit."""
    import torch
    n = 5000
    rng = np.random.default_rng(21)
    cr = np.empty((n, 4), F)
    cr[:, :3] = rng.uniform(-30.0, 30.0, (n, 3)).astype(F)
    cr[:, 3] = F(0.2)
    mats = np.zeros(n, rt3.MATERIAL)
    mats["kind"], mats["rgb"] = rt3.MAT_LAMBERT, (0.5, 0.5, 0.5)
    set_spheres(rt3, renderer, cr, mats)
    before = renderer.group_order(SPH)
    ids = before[before != G.PAD]
    assert len(ids) == n
    centre = np.array([np.sort(cr[:, a])[n // 2] for a in range(3)], F)
    B = cr.copy()
    B[:, :3] += rng.normal(0.0, 4.0, (n, 3)).astype(F)
    B[5::97, 3] = F(0.0)
    B[6::97, 3] = F(-1.0)
    B[7::97, 0] = np.nan
    B[8::97, 2] = np.inf
    B[9::97, 3] = F(1e30)                                                 # r^2 is not finite
    renderer.update_spheres(torch.from_numpy(B).to("cuda:0"))
    renderer.regroup()
    got = renderer.group_order(SPH)
    centres = G.sphere_centres(B, centre)
    want = G.padded(G.regroup_order(ids, centres))
    pads = int((centres == centre).all(axis=1).sum())
    print("%d spheres became pads; %d positions differ from the restatement" % (pads, int((got != want).sum())))
    assert pads >= 5 * (n // 97) and np.array_equal(got, want)
    gone = B.copy()
    bad = (centres == centre).all(axis=1)
    gone[bad] = (1e6, 1e6, 1e6, 1e-3)                                     # tiny, far outside the view
    set_spheres(rt3, other, gone, mats)
    w, h = 96, 72
    cam = rt3.Camera().look_at(w, h, (0.0, 20.0, 90.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0)
    p = rt3.make_params(w, h, spp=2, max_depth=4, seed=4)
    assert renderer.render_path(cam.c, p).tobytes() == other.render_path(cam.c, p).tobytes()


# ------------------------------------------------------------------------------------------------ 3: the host's split
def test_on_distinct_coordinates_the_leaves_are_the_hosts(rt3, renderer):
    cr, mats = distinct_scene(rt3)
    for a in range(3):
        assert len(np.unique(cr[:, a])) == len(cr)
    set_spheres(rt3, renderer, cr, mats)
    w, h = 128, 96
    cam, p = distinct_camera(rt3, w, h), rt3.make_params(w, h, spp=1, max_depth=4, seed=3)
    host = renderer.group_order(SPH)
    frame0 = renderer.render_path(cam.c, p)
    s0 = renderer.stats()
    renderer.regroup()
    dev = renderer.group_order(SPH)
    frame1 = renderer.render_path(cam.c, p)
    s1 = renderer.stats()
    print("filter_tests %d / %d, bound + exact tests %d / %d, positions that differ %d" % (s0.filter_tests, s1.filter_tests, member_tests(s0), member_tests(s1), int((host != dev).sum())))
    assert G.leaf_sets(dev) == G.leaf_sets(host)
    assert frame0.tobytes() == frame1.tobytes() and s0.filter_tests == s1.filter_tests and s0.filter_tests > 0


# ------------------------------------------------------------------------------------------------ 4: the drift
def test_a_regroup_undoes_the_drift_of_64_refits(rt3, renderer, other):
    import torch
    cr, mats = distinct_scene(rt3)
    final = slid_exact(cr, 64)
    for a in range(3):
        assert len(np.unique(final[:, a])) == len(final)                  # test 3's condition holds for the final positions as well
    set_spheres(rt3, renderer, cr, mats)
    dev = torch.device("cuda", 0)
    for k in range(1, 65):
        renderer.update_spheres(torch.from_numpy(slid_exact(cr, k)).to(dev))     # the device form
    w, h = 128, 96
    cam, p = distinct_camera(rt3, w, h), rt3.make_params(w, h, spp=1, max_depth=4, seed=3)
    stale_frame = renderer.render_path(cam.c, p)
    stale = renderer.stats()
    renderer.regroup()
    frame = renderer.render_path(cam.c, p)
    fresh = renderer.stats()
    set_spheres(rt3, other, final, mats)
    want = other.render_path(cam.c, p)
    full = other.stats()
    print("bound + exact tests of a 1-spp frame: %d after 64 refits, %d after the regroup, %d after a full upload (casts %d)"
          % (member_tests(stale), member_tests(fresh), member_tests(full), fresh.ray_casts))
    assert stale_frame.tobytes() == want.tobytes() and frame.tobytes() == want.tobytes()
    assert member_tests(fresh) < member_tests(stale)
    assert G.leaf_sets(renderer.group_order(SPH)) == G.leaf_sets(other.group_order(SPH))


# ------------------------------------------------------------------------------------------------ 5: chain and state
def test_a_range_render_continues_across_an_update_and_a_regroup(rt3, renderer):
    w, h = 96, 72
    cr, mats = rt3.scene_stress(4000, 43)
    cam = stress_camera(rt3, w, h)
    p = rt3.make_params(w, h, spp=4, max_depth=4, seed=2)
    L = rt3.lib()
    set_spheres(rt3, renderer, cr, mats)
    want = renderer.render_path(cam.c, p)
    out = np.zeros((h, w), np.uint32)
    assert L.rt3_render_path_range(renderer._ctx, C.byref(cam.c), C.byref(p), 0, 2, ptr(out)) == 0
    renderer.update_spheres(cr)
    renderer.regroup()
    assert L.rt3_render_path_range(renderer._ctx, C.byref(cam.c), C.byref(p), 2, 2, ptr(out)) == 0
    assert out.tobytes() == want.tobytes()


def test_the_device_form_on_another_stream_is_seen_by_the_next_render_and_allocates_nothing(rt3, renderer, other):
    import torch
    L = rt3.lib()
    w, h = 96, 72
    cr, mats = rt3.scene_stress(4000, 43)
    rng = np.random.default_rng(2)
    B = cr.copy()
    B[:, :3] += rng.normal(0.0, 3.0, (len(B), 3)).astype(F)
    cam = stress_camera(rt3, w, h)
    p = rt3.make_params(w, h, spp=1, max_depth=4, seed=6)
    set_spheres(rt3, other, cr, mats)
    other.update_spheres(B)
    stale_frame = other.render_path(cam.c, p)
    stale = other.stats()
    other.regroup()                                                       # the synchronous form
    want = other.render_path(cam.c, p)
    st_want = other.stats()

    set_spheres(rt3, renderer, cr, mats)
    dev = torch.device("cuda", 0)
    tB = torch.from_numpy(B).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    ctx = renderer._ctx
    with torch.cuda.stream(side):
        renderer.update_spheres(tB)
        renderer.regroup()                                                # torch tensors in use: queued on the side stream (warm-up: the scratch)
        free0 = torch.cuda.mem_get_info(dev)[0]
        for _ in range(10):
            renderer.update_spheres(tB)
            assert L.rt3_regroup_device(ctx, SPH, C.c_void_p(side.cuda_stream)) == 0
        free1 = torch.cuda.mem_get_info(dev)[0]
        set_spheres(rt3, renderer, cr, mats)
        renderer.update_spheres(tB)
        assert L.rt3_regroup_device(ctx, SPH, C.c_void_p(side.cuda_stream)) == 0
    got = renderer.render_path(cam.c, p)                                  # on the context's own stream, no host synchronisation between
    st_got = renderer.stats()
    print("bound + exact tests: stale %d, regrouped %d (synchronous form: %d); free memory %d / %d" % (member_tests(stale), member_tests(st_got), member_tests(st_want), free0, free1))
    assert got.tobytes() == want.tobytes() and stale_frame.tobytes() == want.tobytes()
    assert [getattr(st_got, k) for k in COUNTERS] == [getattr(st_want, k) for k in COUNTERS]
    assert member_tests(st_got) != member_tests(stale)                            # the render did see the new order
    assert np.array_equal(renderer.group_order(SPH), other.group_order(SPH))
    assert free1 == free0, (free0, free1)


def test_errors_and_state(rt3, renderer):
    L = rt3.lib()
    cr, mats = rt3.scene_weekend(42)
    faces, verts = tessellated_sphere(rt3, (0.0, 0.0, -3.0), 0.6)
    buf = np.zeros(1 << 16, np.uint32)
    n = C.c_uint32(0)
    fresh = rt3.initialize_renderer(0)
    try:
        for what in (SPH, MESH, SPH | MESH):
            assert L.rt3_regroup(fresh._ctx, what) == E_STATE             # no scene
            assert L.rt3_regroup_device(fresh._ctx, what, None) == E_STATE
        assert L.rt3_debug_group_order(fresh._ctx, SPH, ptr(buf), len(buf), C.byref(n)) == E_STATE
    finally:
        fresh.close()
    renderer.set_mesh(faces, verts)
    renderer.set_spheres(cr, mats)
    ctx = renderer._ctx
    for what in (0, 4, SPH | 8, 0x80000000):
        assert L.rt3_regroup(ctx, what) == E_ARG and L.rt3_regroup_device(ctx, what, None) == E_ARG
    for what in (0, SPH | MESH, 4):
        assert L.rt3_debug_group_order(ctx, what, ptr(buf), len(buf), C.byref(n)) == E_ARG
    n.value = 0
    assert L.rt3_debug_group_order(ctx, SPH, ptr(buf), 8, C.byref(n)) == E_ARG and n.value == len(renderer.group_order(SPH)) > 8
    n.value = 0
    assert L.rt3_debug_group_order(ctx, MESH, ptr(buf), 8, C.byref(n)) == E_ARG and n.value == len(renderer.group_order(MESH)) >= len(faces)
    assert L.rt3_regroup(ctx, SPH | MESH) == 0 and L.rt3_regroup_device(ctx, MESH, None) == 0 and L.rt3_synchronize(ctx) == 0
    # only one class has a scene
    renderer.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    assert L.rt3_regroup(ctx, MESH) == E_STATE and L.rt3_regroup(ctx, SPH | MESH) == E_STATE and L.rt3_regroup(ctx, SPH) == 0
    renderer.regroup()                                                    # the method names the classes that are there
    # entity buffers out of sync with the commit
    renderer.set_mesh(faces, verts)
    assert L.rt3_mesh_begin(ctx, len(faces), len(verts)) == 0
    assert L.rt3_regroup(ctx, MESH) == E_STATE and L.rt3_regroup(ctx, SPH) == 0
    renderer.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    # a non-finite sphere at set time was left out of the group order
    odd = cr.copy()
    odd[7, 1] = np.inf
    renderer.set_spheres(odd, mats)
    assert L.rt3_regroup(ctx, SPH) == E_STATE
    renderer.set_spheres(cr, mats)
    assert L.rt3_regroup(ctx, SPH) == 0


def test_an_all_direct_scene_is_a_successful_no_op(rt3, renderer):
    one = np.array([[0.0, 0.0, -3.0, 1.0]], F)
    mats = np.zeros(1, rt3.MATERIAL)
    mats["kind"], mats["rgb"] = rt3.MAT_LAMBERT, (0.5, 0.5, 0.5)
    set_spheres(rt3, renderer, one, mats)
    w, h = 64, 48
    cam, p = rt3.main_camera(w, h), rt3.make_params(w, h, spp=2, max_depth=3, seed=1)
    before = renderer.render_path(cam.c, p)
    assert len(renderer.group_order(SPH)) == 0                            # the sphere is on the direct list: no rows
    assert rt3.lib().rt3_regroup(renderer._ctx, SPH) == 0 and rt3.lib().rt3_regroup_device(renderer._ctx, SPH, None) == 0
    renderer.regroup()
    assert renderer.render_path(cam.c, p).tobytes() == before.tobytes() and len(np.unique(before)) > 10


# ------------------------------------------------------------------------------------------------ 6: the command line
def test_the_command_lines_regroup_sequence_is_byte_equal(tmp_path):
    w, h = 96, 72
    args = [EXE, "--scene", "weekend", "--spp", "1", "-W", str(w), "-H", str(h), "-f", "ppm", "--frames", "6", "--slide", "-0.1,0,0.05",
            "--denoise", "P", "--refit"]
    dirs = []
    for extra in ((), ("--regroup", "2")):
        d = tmp_path / ("regroup" if extra else "refit")
        d.mkdir()
        subprocess.run(args + list(extra) + ["out.ppm"], cwd=str(d), check=True, capture_output=True, timeout=300)
        dirs.append(d)
    names = sorted(f.name for f in dirs[0].iterdir())
    assert names == sorted(f.name for f in dirs[1].iterdir()) and "P.5.pfm" in names and "out.ppm" in names
    for n in names:
        assert (dirs[0] / n).read_bytes() == (dirs[1] / n).read_bytes(), n
    assert (dirs[0] / "P.0.pfm").read_bytes() != (dirs[0] / "P.5.pfm").read_bytes()
