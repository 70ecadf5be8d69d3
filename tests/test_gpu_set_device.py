"""A full scene upload from device arrays (rt3_set_spheres_device / rt3_set_mesh_device) on the GPU: every entry point
returns what it returns after the host upload, the state is the host upload's followed by a regroup, counts change on one context, updates
and regroups work on the result, left-out spheres and refusals, and streams.  All comparisons are exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import regroup_ref as G
import scene_build_ref as B
from test_gpu_motion import tessellated_sphere
from test_gpu_regroup import COUNTERS, random_rays, scene_box
from test_gpu_temporal import orbit_camera
from test_gpu_update import moved_spheres, outputs, ptr, scene_pair, stress_camera, upload

pytestmark = pytest.mark.gpu

F = np.float32
E_ARG, E_STATE = -1, -4
SPH, MESH = 1, 2
W, H = 64, 48


@pytest.fixture(scope="module")
def other(rt3, renderer):
    """A second context on the same device: the one that takes the host upload."""
    r = rt3.initialize_renderer(0)
    yield r
    r.close()


def dev(a):
    """A numpy array (records as bytes) as a torch tensor on the GPU."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to("cuda:0")


def device_upload(rt3, r, S):
    """upload() of test_gpu_update.py through the device forms, both classes (a class the scene lacks is cleared by n = 0).  Returns the
    tensors and bit-exact copies of them."""
    if "faces" in S:
        t = [dev(S["faces"]), dev(S["verts"]), None if S["fmats"] is None else dev(S["fmats"])]
    else:
        t = [dev(np.zeros(0, rt3.GFACE)), dev(np.zeros((0, 4), F)), None]
    if "spheres" in S:
        t += [dev(S["spheres"]), dev(S["smats"])]
    else:
        t += [dev(np.zeros((0, 4), F)), dev(np.zeros(0, rt3.MATERIAL))]
    copies = [None if x is None else x.clone() for x in t]
    r.set_mesh(t[0], t[1], t[2])
    r.set_spheres(t[3], t[4])
    return t, copies


def unchanged(tensors, copies):
    import torch
    torch.cuda.synchronize()
    def same_bytes(a, b):                                                 # (bytes: a NaN equals itself; an empty tensor has nothing to view)
        return a.shape == b.shape and (a.numel() == 0 or torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))
    return all(a is None or same_bytes(a, b) for a, b in zip(tensors, copies))


def lambert(rt3, n, seed=0):
    mats = np.zeros(n, rt3.MATERIAL)
    mats["kind"] = rt3.MAT_LAMBERT
    mats["rgb"] = np.random.default_rng(seed).uniform(0.2, 0.9, (n, 3)).astype(F)
    return mats


@functools.lru_cache(None)
def cornell_above_4096(rt3):
    g = 16
    while len(rt3.scene_cornell(g)[0]) <= 4096:
        g += 1
    return g


def scene(rt3, name):
    """(scene dict, camera, flags, Mode R too) on the small frame."""
    if name == "weekend":
        cr, mats = rt3.scene_weekend(42)
        return dict(spheres=cr, smats=mats), orbit_camera(rt3, W, H, 2.0), 0, False
    if name.startswith("stress"):
        cr, mats = rt3.scene_stress(int(name[6:]), 43)
        return dict(spheres=cr, smats=mats), stress_camera(rt3, W, H), 0, False
    if name.startswith("cornell"):
        faces, verts, fm = rt3.scene_cornell(cornell_above_4096(rt3) if name == "cornell_big" else int(name[7:]))
        return dict(faces=faces, verts=verts, fmats=fm), rt3.main_camera(W, H), rt3.FLAG_BLACK_BACKGROUND, True
    if name == "sphere_entity":
        faces, verts = tessellated_sphere(rt3, (0.0, 0.0, -3.0), 0.6)
        return dict(faces=faces, verts=verts, fmats=None), rt3.main_camera(W, H), 0, True
    assert name == "mixed"
    A = scene_pair(rt3, "mixed")[0]
    return A, orbit_camera(rt3, W, H, 2.0), 0, False


def frame(rt3, r, cam, flags=0, seed=5):
    return r.render_path(cam.c, rt3.make_params(W, H, spp=2, max_depth=4, seed=seed, flags=flags)).tobytes()


# ------------------------------------------------------------------------------------------------ 1: same results
@pytest.mark.parametrize("name,env", [("weekend", {})] + [("stress%d" % n, {}) for n in (1, 63, 64, 65, 512, 513, 4097)] +
                         [("stress4097", {"RT3_NO_RESIDENT": "1"}), ("stress4097", {"RT3_LEVELS": "3"}), ("stress4097", {"RT3_LEVELS": "4"}),
                          ("cornell4", {}), ("cornell_big", {}), ("sphere_entity", {}), ("mixed", {})])
def test_the_device_form_returns_what_the_host_form_returns(rt3, renderer, other, name, env, monkeypatch):
    S, cam, flags, mode_r = scene(rt3, name)
    tensors, copies = device_upload(rt3, renderer, S)
    upload(rt3, other, S)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = outputs(rt3, renderer, S, cam, flags, (W, H), mode_r)
    want = outputs(rt3, other, S, cam, flags, (W, H), mode_r)
    rays = random_rays(rt3, *scene_box(S), 20000, 17)
    got.update(random_intersect=renderer.intersect(rays).tobytes(), random_occluded=renderer.occluded(rays).tobytes())
    want.update(random_intersect=other.intersect(rays).tobytes(), random_occluded=other.occluded(rays).tobytes())
    for k in want:
        print("%s %s %s: %d bytes, equal %s" % (name, env, k, len(want[k]), got[k] == want[k]))
    for k in want:
        assert got[k] == want[k], (name, k)
    assert want["path"] == want["brute"]                                  # the unfiltered kernel agrees
    assert len(np.unique(np.frombuffer(want["path"], np.uint32))) > 10    # and the frame shows the scene
    assert unchanged(tensors, copies)


# ------------------------------------------------------------------------------------------------ 2: same state as host + regroup
def random_spheres(rt3, n):
    """Test 2 of test_gpu_regroup.py's final positions: random, with ties and both zeros."""
    rng = np.random.default_rng(n)
    cr = np.empty((n, 4), F)
    cr[:, :3] = rng.uniform(-40.0, 40.0, (n, 3)).astype(F) * np.array([1.0, 0.4, 1.7], F)
    cr[:, 3] = F(0.1)
    cr[:, :3] += rng.normal(0.0, 6.0, (n, 3)).astype(F)
    cr[::5, 0] = np.round(cr[::5, 0])
    cr[3::50, 1] = F(0.0)
    cr[4::50, 1] = F(-0.0)
    return cr, lambert(rt3, n)


def one_frame_counters(rt3, r, cam):
    r.render_path(cam.c, rt3.make_params(W, H, spp=1, max_depth=4, seed=3))
    st = r.stats()
    return [getattr(st, k) for k in COUNTERS]


@pytest.mark.parametrize("name", ["random700", "random4097", "random20000", "weekend"])
def test_the_sphere_state_is_the_host_uploads_after_a_regroup(rt3, renderer, other, name):
    if name == "weekend":
        cr, mats = rt3.scene_weekend(42)
        cam = orbit_camera(rt3, W, H, 2.0)
    else:
        cr, mats = random_spheres(rt3, int(name[6:]))
        cam = rt3.Camera().look_at(W, H, (0.0, 20.0, 150.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0)
    assert B.choice_is_unique(cr)                                         # the guard: the direct list has one answer
    S = dict(spheres=cr, smats=mats)
    device_upload(rt3, renderer, S)
    upload(rt3, other, S)
    other.regroup()
    centre, direct = renderer.sphere_build()
    plan_centre, plan_direct = rt3.sphere_plan(cr)
    got = renderer.group_order(SPH)
    want = G.padded(G.regroup_order(B.usable_ids(cr, plan_direct), G.sphere_centres(cr, plan_centre)))
    host = other.group_order(SPH)
    print("%s: centre %s / %s, direct %s / %s, %d positions, %d differ from the restatement, %d from host + regroup"
          % (name, centre, plan_centre, direct, plan_direct, len(got), int((got != want).sum()) if len(got) == len(want) else -1,
             int((got != host).sum()) if len(got) == len(host) else -1))
    assert np.array_equal(centre, plan_centre) and np.array_equal(centre, B.filter_centre(cr))
    assert np.array_equal(direct, plan_direct) and np.array_equal(direct, B.direct_set(cr))
    assert np.array_equal(got, want) and np.array_equal(got, host)
    a, b = one_frame_counters(rt3, renderer, cam), one_frame_counters(rt3, other, cam)
    print("%s: counters %s / %s" % (name, a, b))
    assert a == b and a[0] > 0


def test_the_mesh_state_is_the_host_uploads_after_a_regroup(rt3, renderer, other):
    """More than 4096 bounded faces (the levels above the LDS limit), seven faces without a bounded hit region scattered among them (the
    tail), and neither part a whole number of rows."""
    faces, verts, fm = rt3.scene_cornell(cornell_above_4096(rt3))
    at = np.array([5, 77, 1000, 1001, 2500, 4100, len(faces) - 1])
    faces = faces.copy()
    for k in ("v2", "v3"):
        faces[k][at] = faces["v1"][at]                                    # coincident vertices: no bounded hit region
    bounded = np.setdiff1d(np.arange(len(faces)), at).astype(np.uint32)
    assert len(bounded) > 4096 and len(bounded) % 64 != 0
    S = dict(faces=faces, verts=verts, fmats=fm)
    device_upload(rt3, renderer, S)
    upload(rt3, other, S)
    other.regroup()
    centre = G.mesh_filter_centre(verts)
    want = np.concatenate([G.padded(G.regroup_order(bounded, G.face_centres(faces, verts, centre))), G.padded(at.astype(np.uint32))])
    got, host = renderer.group_order(MESH), other.group_order(MESH)
    print("%d faces: %d positions, %d differ from the restatement, %d from host + regroup"
          % (len(faces), len(got), int((got != want).sum()) if len(got) == len(want) else -1, int((got != host).sum()) if len(got) == len(host) else -1))
    assert np.array_equal(got, want) and np.array_equal(got, host)
    cam = rt3.main_camera(W, H)
    p = rt3.make_params(W, H, spp=1, max_depth=4, seed=3, flags=rt3.FLAG_BLACK_BACKGROUND)
    stats = []
    for r in (renderer, other):
        r.render_path(cam.c, p)
        stats.append([getattr(r.stats(), k) for k in COUNTERS])
    print("counters %s / %s" % tuple(stats))
    assert stats[0] == stats[1] and stats[0][0] > 0
    f, v = renderer.mesh_download()                                       # the merged entity buffers hold the caller's arrays
    assert f.tobytes() == faces.tobytes() and v.tobytes() == verts.tobytes()


# ------------------------------------------------------------------------------------------------ 3: counts change on one context
def test_counts_change_on_one_context(rt3, renderer, other):
    cam = stress_camera(rt3, W, H)
    renderer.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    other.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))

    def same(cr, mats, device, camera=cam, flags=0):
        if device:
            renderer.set_spheres(dev(cr), dev(mats))
        else:
            renderer.set_spheres(cr, mats)
        other.set_spheres(cr, mats)
        got, want = frame(rt3, renderer, camera, flags), frame(rt3, other, camera, flags)
        print("%d spheres, device form %s: equal %s" % (len(cr), device, got == want))
        return got == want

    for n, device in ((20000, True), (100, True), (4097, True), (513, False), (700, True)):
        assert same(*rt3.scene_stress(n, 43), device), n
    # four large spheres: every one is on the direct list, no rows (after a grouped scene: no stale counts)
    big = np.array([[0.0, 0.0, -30.0, 8.0], [12.0, 3.0, -34.0, 9.0], [-13.0, -2.0, -38.0, 10.0], [1.0, 14.0, -36.0, 7.0]], F)
    assert B.candidates(big)[0].tolist() == [0, 1, 2, 3]
    assert same(big, lambert(rt3, 4, 1), True)
    assert len(renderer.group_order(SPH)) == 0 and renderer.sphere_build()[1].tolist() == [0, 1, 2, 3]
    # new materials on the same positions
    cr, mats = rt3.scene_stress(700, 43)
    assert same(cr, mats, True)
    before = frame(rt3, renderer, cam)
    assert same(cr, lambert(rt3, 700, 9), True) and frame(rt3, renderer, cam) != before
    # n = 0 beside a mesh: the spheres are gone
    faces, verts = tessellated_sphere(rt3, (0.0, 0.0, -3.0), 0.6)
    mcam = rt3.main_camera(W, H)
    for r in (renderer, other):
        r.set_mesh(faces, verts)
    with_spheres = frame(rt3, renderer, mcam)
    renderer.set_spheres(dev(np.zeros((0, 4), F)), dev(np.zeros(0, rt3.MATERIAL)))
    other.set_spheres(np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))
    assert rt3.lib().rt3_set_spheres_device(renderer._ctx, None, None, 0, None) == 0      # (NULL pointers are fine with n = 0)
    got = frame(rt3, renderer, mcam)
    assert got == frame(rt3, other, mcam) and got != with_spheres
    assert rt3.lib().rt3_regroup(renderer._ctx, SPH) == E_STATE           # no spheres
    assert rt3.lib().rt3_set_mesh_device(renderer._ctx, None, 0, None, 0, None, None) == 0
    assert rt3.lib().rt3_regroup(renderer._ctx, MESH) == E_STATE          # and no mesh


# ------------------------------------------------------------------------------------------------ 4: what follows works
def test_updates_and_regroups_work_on_the_result(rt3, renderer, other):
    A, Bm, cam, flags, size = scene_pair(rt3, "mixed")
    cam = orbit_camera(rt3, W, H, 2.0)
    device_upload(rt3, renderer, A)
    upload(rt3, other, A)
    renderer.update_spheres(dev(Bm["spheres"]))
    renderer.update_mesh(dev(Bm["verts"]), dev(Bm["faces"]))
    renderer.regroup()
    renderer.synchronize()
    other.update_spheres(Bm["spheres"])
    other.update_mesh(Bm["verts"], Bm["faces"])
    other.regroup()
    for what in (SPH, MESH):
        assert np.array_equal(renderer.group_order(what), other.group_order(what))
    got = outputs(rt3, renderer, A, cam, flags, (W, H), False)
    want = outputs(rt3, other, A, cam, flags, (W, H), False)
    for k in want:
        assert got[k] == want[k], k
    # a larger sphere scene: the levels above the LDS limit
    cr, mats = rt3.scene_stress(5000, 43)
    scam = stress_camera(rt3, W, H)
    for r in (renderer, other):
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    renderer.set_spheres(dev(cr), dev(mats))
    other.set_spheres(cr, mats)
    moved = moved_spheres(cr)
    renderer.update_spheres(dev(moved))
    renderer.regroup()
    other.update_spheres(moved)
    other.regroup()
    assert np.array_equal(renderer.group_order(SPH), other.group_order(SPH))
    assert frame(rt3, renderer, scam) == frame(rt3, other, scam)


def test_a_range_render_continues_across_a_device_set_of_the_same_scene(rt3, renderer):
    L = rt3.lib()
    cr, mats = rt3.scene_stress(4097, 43)
    cam = stress_camera(rt3, W, H)
    p = rt3.make_params(W, H, spp=4, max_depth=4, seed=2)
    renderer.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    renderer.set_spheres(cr, mats)
    want = renderer.render_path(cam.c, p)
    out = np.zeros((H, W), np.uint32)
    assert L.rt3_render_path_range(renderer._ctx, C.byref(cam.c), C.byref(p), 0, 2, ptr(out)) == 0
    renderer.set_spheres(dev(cr), dev(mats))
    assert L.rt3_render_path_range(renderer._ctx, C.byref(cam.c), C.byref(p), 2, 2, ptr(out)) == 0
    assert out.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ 5: left-out spheres and refusals
def test_left_out_spheres_are_the_hosts(rt3, renderer, other):
    cr, mats = rt3.scene_stress(700, 43)
    cr = cr.copy()
    cr[17, 1] = np.nan
    cr[300, 3] = np.inf
    cam = stress_camera(rt3, W, H)
    S = dict(spheres=cr, smats=mats)
    tensors, copies = device_upload(rt3, renderer, S)
    upload(rt3, other, S)
    got = outputs(rt3, renderer, S, cam, 0, (W, H), False)
    want = outputs(rt3, other, S, cam, 0, (W, H), False)
    for k in want:
        assert got[k] == want[k], k
    centre, direct = renderer.sphere_build()
    plan_centre, plan_direct = rt3.sphere_plan(cr)
    assert B.choice_is_unique(cr) and np.array_equal(centre, plan_centre) and np.array_equal(direct, plan_direct) and 300 in direct
    order = renderer.group_order(SPH)                                     # the region is the usable ids only
    assert np.array_equal(order, G.padded(G.regroup_order(B.usable_ids(cr, plan_direct), G.sphere_centres(cr, plan_centre))))
    assert 17 not in order and 300 not in order
    L, ctx = rt3.lib(), renderer._ctx
    assert L.rt3_update_spheres_device(ctx, C.c_void_p(tensors[3].data_ptr()), len(cr), None) == E_STATE
    assert L.rt3_update_spheres(ctx, ptr(cr), len(cr)) == E_STATE and L.rt3_regroup(ctx, SPH) == E_STATE
    assert unchanged(tensors, copies)


def test_refusals_leave_the_scene_untouched(rt3, renderer):
    L, ctx = rt3.lib(), renderer._ctx
    cr, mats = rt3.scene_stress(700, 43)
    cam = stress_camera(rt3, W, H)
    renderer.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    renderer.set_spheres(dev(cr), dev(mats))
    before = frame(rt3, renderer, cam)
    order = renderer.group_order(SPH)
    for what, i, value in (("r = 0", 419, 0.0), ("r = NaN", 23, np.nan), ("r < 0", 5, -1.0)):
        bad = cr.copy()
        bad[i, 3] = value
        bad[650, 3] = value                                               # (the message names the lowest index)
        t = dev(bad), dev(mats)
        copies = [x.clone() for x in t]
        with pytest.raises(rt3.Fatal, match=r"sphere %d has a non-positive radius" % i):
            renderer.set_spheres(*t)
        assert unchanged(t, copies), what
    odd = mats.copy()
    odd["kind"][77] = 7
    with pytest.raises(rt3.Fatal, match="unknown material kind"):
        renderer.set_spheres(dev(cr), dev(odd))
    tc, tm = dev(cr), dev(mats)
    pc, pm = tc.data_ptr(), tm.data_ptr()
    assert L.rt3_set_spheres_device(ctx, C.c_void_p(pc + 4), C.c_void_p(pm), 8, None) == E_ARG        # misaligned
    assert L.rt3_set_spheres_device(ctx, C.c_void_p(pc), C.c_void_p(pm + 2), 8, None) == E_ARG
    assert L.rt3_set_spheres_device(ctx, None, C.c_void_p(pm), 8, None) == E_ARG                       # NULL with n > 0
    assert L.rt3_set_spheres_device(ctx, C.c_void_p(pc), None, 8, None) == E_ARG
    assert L.rt3_set_spheres_device(None, C.c_void_p(pc), C.c_void_p(pm), 8, None) == E_ARG
    assert frame(rt3, renderer, cam) == before and np.array_equal(renderer.group_order(SPH), order)
    assert L.rt3_update_spheres(ctx, ptr(cr), len(cr)) == 0 and frame(rt3, renderer, cam) == before


def test_mesh_refusals(rt3, renderer):
    L, ctx = rt3.lib(), renderer._ctx
    faces, verts, fm = rt3.scene_cornell(4)
    cam = rt3.main_camera(W, H)
    renderer.set_spheres(np.zeros((0, 4), F), np.zeros(0, rt3.MATERIAL))
    renderer.set_mesh(dev(faces), dev(verts), dev(fm))
    before = frame(rt3, renderer, cam, rt3.FLAG_BLACK_BACKGROUND)
    odd = fm.copy()
    odd["kind"][3] = 7
    with pytest.raises(rt3.Fatal, match="unknown material kind"):
        renderer.set_mesh(dev(faces), dev(verts), dev(odd))
    tf, tv, tm = dev(faces), dev(verts), dev(fm)
    pf, pv, pm = tf.data_ptr(), tv.data_ptr(), tm.data_ptr()
    nf, nv = len(faces), len(verts)
    assert L.rt3_set_mesh_device(ctx, C.c_void_p(pf + 8), nf - 1, C.c_void_p(pv), nv, None, None) == E_ARG      # misaligned
    assert L.rt3_set_mesh_device(ctx, C.c_void_p(pf), nf, C.c_void_p(pv + 4), nv - 1, None, None) == E_ARG
    assert L.rt3_set_mesh_device(ctx, C.c_void_p(pf), nf, C.c_void_p(pv), nv, C.c_void_p(pm + 2), None) == E_ARG
    assert L.rt3_set_mesh_device(ctx, None, nf, C.c_void_p(pv), nv, None, None) == E_ARG                          # NULL with a count
    assert L.rt3_set_mesh_device(ctx, C.c_void_p(pf), nf, None, nv, None, None) == E_ARG
    assert L.rt3_set_mesh_device(None, C.c_void_p(pf), nf, C.c_void_p(pv), nv, None, None) == E_ARG
    assert frame(rt3, renderer, cam, rt3.FLAG_BLACK_BACKGROUND) == before
    assert L.rt3_regroup(ctx, MESH) == 0 and frame(rt3, renderer, cam, rt3.FLAG_BLACK_BACKGROUND) == before
    # a face index out of range: RT3_E_ARG and no mesh, as after rt3_set_mesh
    bad = faces.copy()
    bad["v2"][9] = nv
    t = dev(bad), dev(verts), dev(fm)
    copies = [x.clone() for x in t]
    with pytest.raises(rt3.Fatal, match="a face references a vertex out of range"):
        renderer.set_mesh(*t)
    assert unchanged(t, copies)
    assert L.rt3_regroup(ctx, MESH) == E_STATE
    p = rt3.make_params(W, H, spp=1, max_depth=1, seed=1)
    out = np.zeros((H, W), np.uint32)
    assert L.rt3_render_path(ctx, C.byref(cam.c), C.byref(p), ptr(out)) == E_STATE      # no scene at all
    renderer.set_mesh(tf, tv, tm)                                         # and the context takes the next mesh
    assert frame(rt3, renderer, cam, rt3.FLAG_BLACK_BACKGROUND) == before


# ------------------------------------------------------------------------------------------------ 6: streams
def test_a_device_set_on_a_side_stream_is_seen_by_the_next_render(rt3, renderer, other):
    import torch
    cr, mats = rt3.scene_stress(4097, 43)
    new = moved_spheres(cr)[:3000]
    cam = stress_camera(rt3, W, H)
    p = rt3.make_params(W, H, spp=2, max_depth=4, seed=6)
    for r in (renderer, other):
        r.set_mesh(np.zeros(0, rt3.GFACE), np.zeros((0, 4), F))
    other.set_spheres(cr, mats)
    old_frame = other.render_path(cam.c, p).tobytes()
    other.set_spheres(new, mats[:3000])
    want = other.render_path(cam.c, p).tobytes()
    renderer.set_spheres(cr, mats)
    device = torch.device("cuda", 0)
    base, tm = dev(new), dev(mats[:3000])
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        t = base + 0.0                                                    # produced on the side stream
        renderer.set_spheres(t, tm)
    d_out = torch.empty((H, W), dtype=torch.int32, device=device)
    third = torch.cuda.Stream(device)
    third.wait_stream(torch.cuda.current_stream(device))                  # (d_out's allocation; the scene is ordered by the context's event chain)
    renderer.render_path_device(cam.c, p, d_out.data_ptr(), third.cuda_stream)
    third.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).tobytes()
    assert got == want and want != old_frame
