"""The motion plane of DESIGN.md 4.13 (rt3_motion) and the steps of 4.12 it changes (rt3_denoise_temporal_motion) restated in numpy float32,
vectorised over the pixels, in the kernels' operation order.  Everything 4.13 leaves alone is temporal_ref's and denoise_ref's.

motion(cam, aov (H, W) AOV records, spheres=None or (current (n, 4), previous (n, 4)), mesh=None or (faces GFACE records or (n, 3) vertex
    indices, current vertices (nv, 4), previous vertices (nv, 4))) -> (H, W, 4) float32, (mx, my, mz, moved).
denoise_temporal(colour, aov, cam, prev, motion=None, ...) -> (out, history) as temporal_ref.denoise_temporal, which it equals bit for bit
    wherever moved == 0."""
import numpy as np

import denoise_ref as R
import temporal_ref as T

F = np.float32
HIT_FACE, HIT_SPHERE = 1, 2


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def shown_point(cam, w, h, z):
    """Step 2: P = o + z d per component, d the unit pixel-centre direction of 4.12 step 2 (non-finite where z is)."""
    d, o = T.world_point(cam, w, h, z)
    with np.errstate(invalid="ignore", over="ignore"):
        return (o + z[..., None] * d).astype(F)


def motion(cam, aov, spheres=None, mesh=None):
    z = aov["depth"].astype(F)
    h, w = z.shape
    kind, index = aov["kind"].astype(np.int64), aov["index"].astype(np.int64)
    hit = ~np.isinf(z)
    P = shown_point(cam, w, h, z)
    out = np.zeros((h, w, 4), F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if spheres is not None:
            cur, prev = (np.ascontiguousarray(a, F).reshape(-1, 4) for a in spheres)
            assert cur.shape == prev.shape
            n = len(cur)
            sel = hit & (kind == HIT_SPHERE) & (index < n) & (n > 0)
            i = np.where(sel, index, 0) if n else np.zeros_like(index)
            if n:
                c, q = cur[i], prev[i]
                same = (bits(c) == bits(q)).all(-1)
                k = q[..., 3] * (F(1.0) / c[..., 3])
                Q = (q[..., :3] + (P - c[..., :3]) * k[..., None]).astype(F)
                use = sel & ~same
                out[..., :3] = np.where(use[..., None], Q - P, out[..., :3])
                out[..., 3] = np.where(use, F(1.0), out[..., 3])
        if mesh is not None:
            faces, cur, prev = mesh
            if getattr(faces, "dtype", None) is not None and faces.dtype.names:
                faces = np.stack([faces["v1"], faces["v2"], faces["v3"]], -1)
            faces = np.asarray(faces, np.int64).reshape(-1, 3)
            cur, prev = (np.ascontiguousarray(a, F).reshape(-1, 4)[:, :3] for a in (cur, prev))
            assert cur.shape == prev.shape
            n, nv = len(faces), len(cur)
            sel = hit & (kind == HIT_FACE) & (index < n) & (n > 0)
            if n:
                f = faces[np.where(sel, index, 0)]
                sel = sel & (f < nv).all(-1)
                f = np.where(sel[..., None], f, 0)
                A, B, Cc = (np.ascontiguousarray(cur[f[..., j]]) for j in range(3))
                A1, B1, C1 = (np.ascontiguousarray(prev[f[..., j]]) for j in range(3))
                same = (bits(A) == bits(A1)).all(-1) & (bits(B) == bits(B1)).all(-1) & (bits(Cc) == bits(C1)).all(-1)
                e1, e2, wv = B - A, Cc - A, P - A
                d00, d01, d11 = T.dot(e1, e1), T.dot(e1, e2), T.dot(e2, e2)
                d20, d21 = T.dot(wv, e1), T.dot(wv, e2)
                den = d00 * d11 - d01 * d01
                b2 = (d11 * d20 - d01 * d21) / den
                b3 = (d00 * d21 - d01 * d20) / den
                Q = ((A1 + b2[..., None] * (B1 - A1)) + b3[..., None] * (C1 - A1)).astype(F)
                use = sel & ~same & (den != F(0.0))
                out[..., :3] = np.where(use[..., None], Q - P, out[..., :3])
                out[..., 3] = np.where(use, F(1.0), out[..., 3])
    return out


def reproject(cam, prev_cam, w, h, z, motion=None):
    """Steps 2 and 3 of 4.12 with the motion term: (r, ok, x', y') per pixel.  A pixel that hit and has moved != 0 adds m to its world
    point and is projected even under a byte-equal camera; every other pixel is temporal_ref.reproject's."""
    d, o = T.world_point(cam, w, h, z)
    po, L, n, a_u, a_v, ln = T.projection_constants(prev_cam)
    hit = ~np.isinf(z)
    moved = np.zeros((h, w), bool) if motion is None else hit & (motion[..., 3] != F(0.0))
    with np.errstate(invalid="ignore", over="ignore"):
        pt = (o + z[..., None] * d).astype(F)
        if motion is not None:
            pt = np.where(moved[..., None], pt + motion[..., :3].astype(F), pt)
        r = np.where(hit[..., None], pt - po, d).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = ln / T.dot(r, n)
        P = (s[..., None] * r - L).astype(F)
        xp = (T.dot(P, a_u) * (F(w) - F(1.0))).astype(F)
        yp = ((F(h) - F(1.0)) - T.dot(P, a_v) * (F(h) - F(1.0))).astype(F)
        ok = np.isfinite(s) & (s > F(0.0))
    if T.same_camera(cam, prev_cam):
        xs, ys = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
        xp, yp, ok = np.where(moved, xp, xs), np.where(moved, yp, ys), np.where(moved, ok, True)
    return r, ok, xp, yp


def gather_history(hist, n, z, gz, r, ok, xp, yp, depth_tolerance, normal_tolerance):
    """Step 4 of 4.12: the sums over the consistent bilinear taps -> (sw, si, s1, s2, nmin)."""
    hh, ww = z.shape
    sw = np.zeros((hh, ww), F)
    si = np.zeros((hh, ww, 3), F)
    s1, s2 = np.zeros((hh, ww), F), np.zeros((hh, ww), F)
    nmin = np.full((hh, ww), np.inf, F)
    with np.errstate(invalid="ignore"):
        ok = ok & (xp > F(-1.0)) & (xp < F(ww)) & (yp > F(-1.0)) & (yp < F(hh))
    with np.errstate(invalid="ignore", over="ignore"):
        zhat = np.sqrt(T.dot(r, r))
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
        inside = ok & (wt != F(0.0)) & (qx >= 0) & (qx < ww) & (qy >= 0) & (qy < hh)
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


def history_weight(aov, cam, hist, prev_cam, motion=None, depth_tolerance=2.0, normal_tolerance=0.9):
    """sw of step 4 per pixel: a pixel has a valid history where sw >= 0.01."""
    _, _, _, n, z, gz = R.prepare(np.zeros(aov.shape + (4,), F), aov)
    hh, ww = z.shape
    r, ok, xp, yp = reproject(cam, prev_cam, ww, hh, z, motion)
    return gather_history(hist, n, z, gz, r, ok, xp, yp, depth_tolerance, normal_tolerance)[0]


def denoise_temporal(colour, aov, cam, prev=None, motion=None, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0, alpha=0.2,
                     moments_alpha=0.2, depth_tolerance=2.0, normal_tolerance=0.9):
    """temporal_ref.denoise_temporal with the motion plane in steps 2 and 3; steps 5 to 7 are restated as they stand there."""
    squarings = int(normal_power).bit_length() - 1
    assert 1 << squarings == normal_power
    sl, sz = F(sigma_luminance), F(sigma_depth)
    i_cur, l_cur, albedo, n, z, gz = R.prepare(colour, aov)
    hh, ww = z.shape
    if prev is not None:
        hist, prev_cam = prev
        r, ok, xp, yp = reproject(cam, prev_cam, ww, hh, z, None if motion is None else np.asarray(motion, F))
        sw, si, s1, s2, nmin = gather_history(hist, n, z, gz, r, ok, xp, yp, depth_tolerance, normal_tolerance)
    else:
        sw, si, s1, s2 = np.zeros((hh, ww), F), np.zeros((hh, ww, 3), F), np.zeros((hh, ww), F), np.zeros((hh, ww), F)
        nmin = np.full((hh, ww), np.inf, F)
    valid = sw >= F(0.01)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        length = np.where(valid, np.fmin(nmin + F(1.0), F(65535.0)), F(1.0)).astype(F)
        a1 = np.fmax(F(alpha), F(1.0) / length)[..., None]
        a2 = np.fmax(F(moments_alpha), F(1.0) / length)
        i_blend = ((F(1.0) - a1) * (si / sw[..., None]) + a1 * i_cur).astype(F)
        m1_blend = ((F(1.0) - a2) * (s1 / sw) + a2 * l_cur).astype(F)
        m2_blend = ((F(1.0) - a2) * (s2 / sw) + a2 * (l_cur * l_cur)).astype(F)
    i = np.where(valid[..., None], i_blend, i_cur).astype(F)
    m1 = np.where(valid, m1_blend, l_cur).astype(F)
    m2 = np.where(valid, m2_blend, l_cur * l_cur).astype(F)
    L = R.lum(i)
    v = np.where(length >= F(4.0), np.maximum(F(0.0), m2 - m1 * m1), R.moments(L, n, z, gz, squarings, sz)).astype(F)
    first = None
    for k in range(iterations):
        i, v = R.atrous_pass(i, v, n, z, gz, 1 << k, squarings, sl, sz)
        if k == 0:
            first = i
    out = np.zeros(i.shape[:2] + (4,), F)
    out[..., :3] = np.where(albedo > R.THRESHOLD, i * albedo, i)
    hist_out = np.zeros((hh, ww), T.HISTORY)
    hist_out["colour"] = first
    hist_out["length"] = length
    hist_out["moments"] = np.stack([m1, m2], -1)
    hist_out["depth"] = z
    hist_out["normal"] = n
    return out, hist_out
