"""The temporal denoiser of DESIGN.md 4.12 (rt3_denoise_temporal) restated in numpy float32, vectorised over the pixels, in the kernels'
operation order.  The spatial parts (demodulation, depth slopes, the 7 x 7 variance, the a-trous passes, remodulation) are denoise_ref's.

denoise_temporal(colour (H, W, 4), aov (H, W) AOV records, cam, prev=None or (history (H, W) HISTORY records, prev_cam), ...)
    -> (out (H, W, 4) float32, history (H, W) HISTORY records).
A camera is anything with origin, horizontal, vertical and lower_left_corner sequences (the ctypes rt3_camera, or a Cam below)."""
import numpy as np

import denoise_ref as R

F = np.float32
HISTORY = np.dtype([("colour", "<f4", 3), ("length", "<f4"), ("moments", "<f4", 2), ("depth", "<f4"), ("_pad0", "<f4"),
                    ("normal", "<f4", 3), ("_pad1", "<f4")])
TEMPORAL_DEFAULTS = dict(alpha=0.2, moments_alpha=0.2, depth_tolerance=2.0, normal_tolerance=0.9)
FIELDS = ("origin", "horizontal", "vertical", "lower_left_corner")


class Cam:
    """A plain camera: the four vectors of rt3_camera as float32 arrays."""

    def __init__(self, origin, horizontal, vertical, lower_left_corner):
        self.origin, self.horizontal, self.vertical, self.lower_left_corner = (np.array(v, F) for v in
                                                                               (origin, horizontal, vertical, lower_left_corner))


def vecs(cam):
    return [np.array(list(getattr(cam, f)), F) for f in FIELDS]


def same_camera(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(vecs(a), vecs(b)))


def dot(a, b):
    """(x x' + y y') + z z' over the last axis (broadcasting)."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(h, v):
    return np.array([h[1] * v[2] - h[2] * v[1], h[2] * v[0] - h[0] * v[2], h[0] * v[1] - h[1] * v[0]], F)


def projection_constants(prev_cam):
    """Step 3's per-call constants in the library's order: L = llc' - o', n = h x v, a_u = (v x n) / (h . (v x n)), a_v = (n x h) /
    (v . (n x h)), L . n."""
    o, h, v, llc = vecs(prev_cam)
    L = (llc - o).astype(F)
    n = cross(h, v)
    vn = cross(v, n)
    a_u = (vn / dot(h, vn)).astype(F)
    nh = cross(n, h)
    a_v = (nh / dot(v, nh)).astype(F)
    return o, L, n, a_u, a_v, F(dot(L, n))


def world_point(cam, w, h, z):
    """Step 2: r per pixel ((H, W, 3) float32) relative to the origin o' subtracted later; returns (unit direction d, o)."""
    o, hor, ver, llc = vecs(cam)
    x = np.arange(w, dtype=F)[None, :]
    y = np.arange(h)[:, None]
    u = np.broadcast_to(x / (F(w) - F(1.0)), (h, w))
    v = np.broadcast_to((h - 1 - y).astype(F) / (F(h) - F(1.0)), (h, w))
    d = np.stack([((llc[c] + u * hor[c]) + v * ver[c]) - o[c] for c in range(3)], -1).astype(F)
    inv = F(1.0) / np.sqrt(dot(d, d))
    return (d * inv[..., None]).astype(F), o


def reproject(cam, prev_cam, w, h, z, shortcut=True):
    """Steps 2 and 3: (r, ok, x', y') per pixel.  shortcut=False projects even when the cameras are equal byte for byte."""
    d, o = world_point(cam, w, h, z)
    po, L, n, a_u, a_v, ln = projection_constants(prev_cam)
    hit = ~np.isinf(z)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(hit[..., None], (o + z[..., None] * d) - po, d).astype(F)
    if shortcut and same_camera(cam, prev_cam):
        xs, ys = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
        return r, np.ones((h, w), bool), xs, ys
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = ln / dot(r, n)
        P = (s[..., None] * r - L).astype(F)
        xp = dot(P, a_u) * (F(w) - F(1.0))
        yp = (F(h) - F(1.0)) - dot(P, a_v) * (F(h) - F(1.0))
    return r, np.isfinite(s) & (s > F(0.0)), xp.astype(F), yp.astype(F)


def denoise_temporal(colour, aov, cam, prev=None, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0, alpha=0.2,
                     moments_alpha=0.2, depth_tolerance=2.0, normal_tolerance=0.9, blended_out=None):
    """The whole call.  blended_out: a dict that receives the blended I, the moments, length and v (the pass input)."""
    squarings = int(normal_power).bit_length() - 1
    assert 1 << squarings == normal_power
    sl, sz = F(sigma_luminance), F(sigma_depth)
    i_cur, l_cur, albedo, n, z, gz = R.prepare(colour, aov)
    hh, ww = z.shape
    sw = np.zeros((hh, ww), F)
    si = np.zeros((hh, ww, 3), F)
    s1, s2 = np.zeros((hh, ww), F), np.zeros((hh, ww), F)
    nmin = np.full((hh, ww), np.inf, F)
    if prev is not None:
        hist, prev_cam = prev
        r, ok, xp, yp = reproject(cam, prev_cam, ww, hh, z)
        ok = ok & (xp > F(-1.0)) & (xp < F(ww)) & (yp > F(-1.0)) & (yp < F(hh))
        with np.errstate(invalid="ignore", over="ignore"):
            zhat = np.sqrt(dot(r, r))
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
                geo = (np.abs(zq - zhat) <= bound) & (dot(n, rec["normal"].astype(F)) >= F(normal_tolerance))
            consistent = np.where(hit & ~np.isinf(zq), geo, ~hit & np.isinf(zq))
            use = inside & consistent
            wt = wt.astype(F)
            sw = np.where(use, sw + wt, sw)
            si = np.where(use[..., None], si + wt[..., None] * rec["colour"].astype(F), si)
            s1 = np.where(use, s1 + wt * rec["moments"][..., 0].astype(F), s1)
            s2 = np.where(use, s2 + wt * rec["moments"][..., 1].astype(F), s2)
            nmin = np.where(use, np.fmin(nmin, rec["length"].astype(F)), nmin)
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
    if blended_out is not None:
        blended_out.update(i=i, m1=m1, m2=m2, length=length, v=v)
    first = None
    for k in range(iterations):
        i, v = R.atrous_pass(i, v, n, z, gz, 1 << k, squarings, sl, sz)
        if k == 0:
            first = i
    out = np.zeros(i.shape[:2] + (4,), F)
    out[..., :3] = np.where(albedo > R.THRESHOLD, i * albedo, i)
    hist_out = np.zeros((hh, ww), HISTORY)
    hist_out["colour"] = first
    hist_out["length"] = length
    hist_out["moments"] = np.stack([m1, m2], -1)
    hist_out["depth"] = z
    hist_out["normal"] = n
    return out, hist_out
