"""Lens sequences (include/rt3.h "Lens sequences") restated in numpy float32: turns, the inverse lens law, and the temporal
denoiser and the motion plane of a frame rendered through a lens.  Every operation is an IEEE f32 one rounded on its own and nothing is fused, so
this file reproduces rt3_debug_turns and rt3_debug_optic_pixel (host) and the lens forms of k_temporal_reproject and k_motion (device) bit for
bit.  The forward law is lens_ref's; what 4.24 leaves alone of 4.12 and 4.13 is motion_ref's, temporal_ref's and denoise_ref's.

turns(c, s) -> float32, elementwise.
project(prev_lens, width, height, r (..., 3)) -> (x', y', zhat, face, valid).
denoise_temporal_lens(colour, aov, lens, prev=None or (history, prev_lens), motion=None, ...) -> (out, history).
motion_lens(lens, aov, spheres=None, mesh=None) -> (H, W, 4) float32.
project64 / turns64: the same positions in float64 with numpy's arctan2, the truth the f32 law is held against."""
from unittest import mock

import numpy as np

import lens_ref as L
import motion_ref as M
import temporal_ref as T

F = np.float32
EQUIRECT, FISHEYE, ORTHO, CUBE = L.EQUIRECT, L.FISHEYE, L.ORTHO, L.CUBE
A = [F(v) for v in (-0.3333314528, 0.1999355085, -0.1420889944, 0.1065626393, -0.0752896400, 0.0429096138, -0.0161657367, 0.0028662257)]   # a2 .. a16


def turns(c, s):
    c, s = np.broadcast_arrays(np.asarray(c, F), np.asarray(s, F))
    ac, as_ = np.abs(c), np.abs(s)
    hi = np.where(ac > as_, ac, as_)
    lo = np.where(ac > as_, as_, ac)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        bad = ~np.isfinite(ac) | ~np.isfinite(as_) | ~(hi > F(0.0))
        t = (lo / hi).astype(F)
        z = t * t
        p = np.full(t.shape, A[7], F)
        for k in A[6::-1]:
            p = p * z
            p = p + k
        p = p * z
        p = p + F(1.0)
        u = (t * p) * F(0.159154937)
        u = np.where(as_ > ac, F(0.25) - u, u)
        u = np.where(c < F(0.0), F(0.5) - u, u)
        u = np.where(s < F(0.0), F(1.0) - u, u)
        u = np.where(u >= F(1.0), F(0.0), u)
    return np.where(bad, F(np.nan), u).astype(F)


def turns64(c, s):
    """The angle of (c, s) in turns in [0, 1), float64."""
    return np.mod(np.arctan2(np.asarray(s, np.float64), np.asarray(c, np.float64)) / (2.0 * np.pi), 1.0)


def same_optic(a, b):
    """Bit equality of what the inverse law reads: model, origin, axes and the model's own parameter."""
    if int(a.model) != int(b.model):
        return False
    bits = lambda v: np.array(list(v), F).view(np.uint32)      # noqa: E731
    same = all(np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in ("origin", "right", "up", "forward"))
    if int(a.model) == FISHEYE:
        same = same and np.array_equal(bits([a.half_fov_turns]), bits([b.half_fov_turns]))
    if int(a.model) == ORTHO:
        same = same and np.array_equal(bits(a.half_extent), bits(b.half_extent))
    return same


def cube_face(v):
    """The face cases of the environment lookup law for v (..., 3) -> (f, m, sc, tc)."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    c0 = (ax >= ay) & (ax >= az)
    c1 = ~c0 & (ay >= az)
    f = np.where(c0, np.where(x < 0, 1, 0), np.where(c1, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
    m = np.where(c0, ax, np.where(c1, ay, az))
    sc = np.where(c0, np.where(x < 0, z, -z), np.where(c1, x, np.where(z < 0, -x, x)))
    tc = np.where(c0, -y, np.where(c1, np.where(y < 0, -z, z), -y))
    return f.astype(np.int64), m, sc, tc


def project(lens, width, height, r):
    """project<MODEL> of 4.24 for points r (..., 3) relative to the lens's origin -> (x', y', zhat float32, face int64, valid bool).  (An ORTHO
    miss is the caller's business: it is not projected.)"""
    r = np.asarray(r, F)
    W, H = F(width), F(height)
    right, up, forward = (L._vec(lens, k) for k in ("right", "up", "forward"))
    model = int(lens.model)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        lx, ly, lz = T.dot(r, right), T.dot(r, up), T.dot(r, forward)
        zhat = lz if model == ORTHO else np.sqrt(T.dot(r, r))
        face = np.zeros(lx.shape, np.int64)
        pole = np.zeros(lx.shape, bool)
        if model == EQUIRECT:
            hxz = np.sqrt(lx * lx + lz * lz)
            a = turns(-lz, -lx)
            b = F(2.0) * turns(ly, hxz)
            px, py = a * W, b * H
        elif model == FISHEYE:
            hxy = np.sqrt(lx * lx + ly * ly)
            tau = turns(lz, hxy)
            rr = tau / F(lens.half_fov_turns)
            off = hxy > F(0.0)
            nx = np.where(off, rr * (lx / hxy), F(0.0)).astype(F)
            ny = np.where(off, rr * (ly / hxy), F(0.0)).astype(F)
            pole = ~off & ~(tau == F(0.0))
            m = F(0.5) * F(min(width, height))
            px, py = nx * m + F(0.5) * W, F(0.5) * H - ny * m
        elif model == ORTHO:
            nx = lx / F(lens.half_extent[0])
            ny = ly / F(lens.half_extent[1])
            px, py = ((nx + F(1.0)) * F(0.5)) * W, ((F(1.0) - ny) * F(0.5)) * H
        elif model == CUBE:
            face, m, sc, tc = cube_face(np.stack([lx, ly, -lz], -1))
            px = ((sc / m) * F(0.5) + F(0.5)) * W
            py = (face * width).astype(F) + ((tc / m) * F(0.5) + F(0.5)) * W
        else:
            raise ValueError("unknown lens model")
        xp, yp = (px - F(0.5)).astype(F), (py - F(0.5)).astype(F)
    valid = ~pole & ~np.isnan(xp) & ~np.isnan(yp)
    if model == FISHEYE:
        xp, yp = np.where(pole, F(np.nan), xp), np.where(pole, F(np.nan), yp)
    return xp, yp, zhat.astype(F), face, valid


def project64(lens, width, height, r):
    """The frame position (x', y') of r in float64 with numpy's arctan2 (no tap rules, no validity: the caller avoids the poles)."""
    r = np.asarray(r, np.float64)
    right, up, forward = (L._vec(lens, k).astype(np.float64) for k in ("right", "up", "forward"))
    lx, ly, lz = r @ right, r @ up, r @ forward
    model = int(lens.model)
    W, H = float(width), float(height)
    if model == EQUIRECT:
        px, py = turns64(-lz, -lx) * W, 2.0 * turns64(ly, np.hypot(lx, lz)) * H
    elif model == FISHEYE:
        hxy = np.hypot(lx, ly)
        rr = turns64(lz, hxy) / float(F(lens.half_fov_turns))
        m = 0.5 * min(width, height)
        with np.errstate(invalid="ignore", divide="ignore"):
            nx, ny = np.where(hxy > 0, rr * lx / hxy, 0.0), np.where(hxy > 0, rr * ly / hxy, 0.0)
        px, py = nx * m + 0.5 * W, 0.5 * H - ny * m
    elif model == ORTHO:
        px = (lx / float(F(lens.half_extent[0])) + 1.0) * 0.5 * W
        py = (1.0 - ly / float(F(lens.half_extent[1]))) * 0.5 * H
    else:
        f, m, sc, tc = cube_face(np.stack([lx, ly, -lz], -1))
        px, py = (sc / m * 0.5 + 0.5) * W, f * W + (tc / m * 0.5 + 0.5) * W
    return px - 0.5, py - 0.5


def centre_rays(lens, width, height):
    """The centre ray of every pixel (the lens law at spp 1: no jitter) -> (origin (H, W, 3), unit direction (H, W, 3)), float32."""
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    rec = L.rays(lens, width, height, 1, 0, xx.reshape(-1), yy.reshape(-1), 0)
    return rec["origin"].reshape(height, width, 3).astype(F), rec["direction"].reshape(height, width, 3).astype(F)


def shown_point(lens, w, h, z):
    """P = o_p + z d per component (non-finite where z is)."""
    o, d = centre_rays(lens, w, h)
    with np.errstate(invalid="ignore", over="ignore"):
        return (o + z[..., None] * d).astype(F)


class Reprojected:
    """What steps 2 and 3 hand step 4 besides (ok, x', y'): r, the depth the history's is compared with, and the cube face of the taps."""

    def __init__(self, r, zhat, face, model):
        self.r, self.zhat, self.face, self.model = r, zhat, face, model


def reproject(lens, prev_lens, w, h, z, motion=None):
    """Steps 2 and 3 of 4.12 as 4.24 restates them: (Reprojected, ok, x', y') per pixel."""
    model = int(lens.model)
    assert int(prev_lens.model) == model
    o, d = centre_rays(lens, w, h)
    po = L._vec(prev_lens, "origin")
    hit = ~np.isinf(z)
    moved = np.zeros((h, w), bool) if motion is None else hit & (motion[..., 3] != F(0.0))
    with np.errstate(invalid="ignore", over="ignore"):
        pt = (o + z[..., None] * d).astype(F)
        if motion is not None:
            pt = np.where(moved[..., None], pt + motion[..., :3].astype(F), pt)
        r = np.where(hit[..., None], pt - po, d).astype(F)
    xp, yp, zhat, face, ok = project(prev_lens, w, h, r)
    xs, ys = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    keep = np.zeros((h, w), bool)
    if same_optic(lens, prev_lens):
        keep = ~moved
    if model == ORTHO:
        keep = keep | ~hit
    xp, yp, ok = np.where(keep, xs, xp), np.where(keep, ys, yp), np.where(keep, True, ok)
    if model == CUBE:
        face = np.where(keep, ys.astype(np.int64) // w, face)
    return Reprojected(r, zhat, face, model), ok, xp.astype(F), yp.astype(F)


def gather_history(hist, n, z, gz, view, ok, xp, yp, depth_tolerance, normal_tolerance):
    """Step 4 of 4.12 with 4.24's taps (EQUIRECT wraps columns, CUBE stays on the face) and depth -> (sw, si, s1, s2, nmin)."""
    hh, ww = z.shape
    sw = np.zeros((hh, ww), F)
    si = np.zeros((hh, ww, 3), F)
    s1, s2 = np.zeros((hh, ww), F), np.zeros((hh, ww), F)
    nmin = np.full((hh, ww), np.inf, F)
    with np.errstate(invalid="ignore"):
        ok = ok & (xp > F(-1.0)) & (xp < F(ww)) & (yp > F(-1.0)) & (yp < F(hh))
    zhat = view.zhat
    with np.errstate(invalid="ignore", over="ignore"):
        bound = F(depth_tolerance) * (gz + F(1e-3) * zhat)
    x0 = np.floor(np.where(ok, xp, F(0.0)))
    y0 = np.floor(np.where(ok, yp, F(0.0)))
    fx, fy = (np.where(ok, xp, F(0.0)) - x0).astype(F), (np.where(ok, yp, F(0.0)) - y0).astype(F)
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    one = F(1.0)
    weights = [(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy]
    hit = ~np.isinf(z)
    for k, wt in enumerate(weights):
        qx, qy = ix + (k & 1), iy + (k >> 1)
        if view.model == EQUIRECT:
            qx = np.where(qx < 0, qx + ww, np.where(qx >= ww, qx - ww, qx))
        inside = ok & (wt != F(0.0)) & (qx >= 0) & (qx < ww) & (qy >= 0) & (qy < hh)
        if view.model == CUBE:
            inside = inside & (qy >= view.face * ww) & (qy < (view.face + 1) * ww)
        rec = hist[np.clip(qy, 0, hh - 1), np.clip(qx, 0, ww - 1)]
        zq = rec["depth"].astype(F)
        with np.errstate(invalid="ignore"):
            geo = (np.abs(zq - zhat) <= bound) & (T.dot(n, rec["normal"].astype(F)) >= F(normal_tolerance))
        consistent = np.where(hit & ~np.isinf(zq), geo, ~hit & np.isinf(zq))
        use = inside & consistent
        wt = wt.astype(F)
        sw = np.where(use, sw + wt, sw)
        si = np.where(use[..., None], si + wt[..., None] * rec["colour"].astype(F), si)
        s1 = np.where(use, s1 + wt * rec["moments"][..., 0].astype(F), s1)
        s2 = np.where(use, s2 + wt * rec["moments"][..., 1].astype(F), s2)
        nmin = np.where(use, np.fmin(nmin, rec["length"].astype(F)), nmin)
    return sw, si, s1, s2, nmin


def denoise_temporal_lens(colour, aov, lens, prev=None, motion=None, **kw):
    """rt3_denoise_temporal_optic: motion_ref.denoise_temporal with steps 2 to 4 replaced by the two functions above (it takes them from its
    module, so those two names are what is swapped for the call); steps 1 and 5 to 7 are the ones stated there."""
    with mock.patch.object(M, "reproject", reproject), mock.patch.object(M, "gather_history", gather_history):
        return M.denoise_temporal(colour, aov, lens, prev, motion, **kw)


def motion_lens(lens, aov, spheres=None, mesh=None):
    """rt3_motion_optic: motion_ref.motion with step 2's point on the lens's centre ray (the one name swapped for the call)."""
    with mock.patch.object(M, "shown_point", shown_point):
        return M.motion(lens, aov, spheres, mesh)
