"""The lens models' ray law (include/rt3.h "Lens models") restated in numpy float32.

Every operation of the law is an IEEE f32 one rounded on its own, and the fused multiply-adds inside sincos2pi are environment_sample_ref.fma32, so this
file reproduces rt3_debug_lens_ray (host) and k_lens_rays (device) bit for bit: the tests compare bit patterns.  rays64() evaluates the same pixel
positions in float64 with the library's sin / cos: the truth the f32 law's directions are held against."""
import numpy as np

from environment_sample_ref import fma32, hash_u32, u01
from light_sample_ref import sincos2pi

F = np.float32
U = np.uint32
EQUIRECT, FISHEYE, ORTHO, CUBE = 1, 2, 3, 4
RAY = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("_pad", "<u4")])


def hash2(a, b):
    return hash_u32(np.asarray(a, U) ^ hash_u32(b))


def edge_of(spp):
    e = int(np.sqrt(spp))
    while e * e > spp:
        e -= 1
    while (e + 1) * (e + 1) <= spp:
        e += 1
    return e if (e * e == spp and spp > 1) else 0


def jitter(x, y, s, width, spp, seed):
    """(jx, jy) of rt3_render_path's ray cast 0: counters 1 and 2 of the path's base, stratified when spp is a perfect square > 1."""
    x, y, s = (np.asarray(v, U) for v in (x, y, s))
    with np.errstate(over="ignore"):
        base = hash2(y * U(width) + x, hash2(s, U(seed)))
    if spp <= 1:
        z = np.zeros(base.shape, F)
        return z, z.copy()
    xi0, xi1 = u01(hash2(base, U(1))), u01(hash2(base, U(2)))
    e = edge_of(spp)
    if e:
        sy = s // U(e)
        sx = s - sy * U(e)
        return (sx.astype(F) + xi0) / F(e) - F(0.5), (sy.astype(F) + xi1) / F(e) - F(0.5)
    return xi0 - F(0.5), xi1 - F(0.5)


def _vec(lens, name):
    return np.array([getattr(lens, name)[c] for c in range(3)], F)


FACE_ROWS = (lambda s, t, o: (o, -t, -s), lambda s, t, o: (-o, -t, s), lambda s, t, o: (s, o, t),
             lambda s, t, o: (s, -o, -t), lambda s, t, o: (s, -t, o), lambda s, t, o: (-s, -t, -o))


def pixel_position(x, y, s, width, height, spp, seed):
    """(px, py, jy) in f32, as the law computes them."""
    jx, jy = jitter(x, y, s, width, spp, seed)
    px = (np.asarray(x, U).astype(F) + F(0.5)) + jx
    py = (np.asarray(y, U).astype(F) + F(0.5)) - jy
    return px, py, jy


def rays(lens, width, height, spp, seed, x, y, s):
    """RAY records of samples s of frame pixels (x, y) (arrays of one shape), by the law, in f32."""
    x, y, s = (np.asarray(v, U).reshape(-1) for v in np.broadcast_arrays(x, y, s))
    W, H = F(width), F(height)
    px, py, jy = pixel_position(x, y, s, width, height, spp, seed)
    a = px / W
    b = py / H
    origin, right, up, forward = (_vec(lens, k) for k in ("origin", "right", "up", "forward"))
    o = np.broadcast_to(origin, (len(x), 3)).astype(F).copy()
    model = int(lens.model)
    if model == EQUIRECT:
        ct, st = sincos2pi(b * F(0.5))
        cp, sp = sincos2pi(a)
        lx, ly, lz = -sp * st, ct, -cp * st
    elif model == FISHEYE:
        m = F(0.5) * F(min(width, height))
        nx = (px - F(0.5) * W) / m
        ny = (F(0.5) * H - py) / m
        r = np.sqrt(nx * nx + ny * ny)
        tau = np.fmin(r * F(lens.half_fov_turns), F(0.5))
        c, sn = sincos2pi(tau)
        with np.errstate(invalid="ignore", divide="ignore"):
            k = np.where(r > 0, sn / r, F(0.0)).astype(F)
        lx, ly, lz = nx * k, ny * k, c
    elif model == ORTHO:
        nx = a * F(2.0) - F(1.0)
        ny = F(1.0) - b * F(2.0)
        e1 = nx * F(lens.half_extent[0])
        e2 = ny * F(lens.half_extent[1])
        o = ((origin[None, :] + e1[:, None] * right[None, :]) + e2[:, None] * up[None, :]).astype(F)
        lx, ly, lz = np.zeros(len(x), F), np.zeros(len(x), F), np.ones(len(x), F)
    elif model == CUBE:
        n = width
        f = x * U(0) + y // U(n)
        j = y - f * U(n)
        sc = a * F(2.0) - F(1.0)
        tc = (((j.astype(F) + F(0.5)) - jy) / F(n)) * F(2.0) - F(1.0)
        one = np.ones(len(x), F)
        v = np.zeros((len(x), 3), F)
        for face in range(6):
            sel = f == face
            v[sel] = np.stack(FACE_ROWS[face](sc, tc, one), axis=-1)[sel]
        lx, ly, lz = v[:, 0], v[:, 1], -v[:, 2]
    else:
        raise ValueError("unknown lens model")
    w = ((lx[:, None] * right[None, :] + ly[:, None] * up[None, :]) + lz[:, None] * forward[None, :]).astype(F)
    inv = F(1.0) / np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    out = np.zeros(len(x), RAY)
    out["origin"] = o
    out["t_max"] = np.inf
    out["direction"] = w * inv[:, None]
    return out


def frame_rays(lens, params, sample_begin=0, sample_count=None, rows=None):
    """What rt3_lens_rays returns: record (s - begin) * npix + pix over the owned pixels (rows: their frame rows; default: the whole frame)."""
    W, H = params.width, params.height
    rows = np.arange(H) if rows is None else np.asarray(rows)
    sc = params.spp - sample_begin if sample_count is None else sample_count
    yy, xx = np.meshgrid(rows, np.arange(W), indexing="ij")
    parts = [rays(lens, W, H, params.spp, params.seed, xx.reshape(-1), yy.reshape(-1), np.full(xx.size, s)) for s in range(sample_begin, sample_begin + sc)]
    return np.concatenate(parts) if parts else np.zeros(0, RAY)


def directions64(lens, width, height, spp, seed, x, y, s):
    """Unit directions of the same (px, py, jy) — the f32 pixel positions — with everything behind them in float64 (numpy's sin / cos)."""
    x, y, s = (np.asarray(v, U).reshape(-1) for v in np.broadcast_arrays(x, y, s))
    px, py, jy = (v.astype(np.float64) for v in pixel_position(x, y, s, width, height, spp, seed))
    W, H = float(width), float(height)
    a, b = px / W, py / H
    right, up, forward = (_vec(lens, k).astype(np.float64) for k in ("right", "up", "forward"))
    model = int(lens.model)
    if model == EQUIRECT:
        th, ph = np.pi * b, 2.0 * np.pi * a
        l = np.stack([-np.sin(ph) * np.sin(th), np.cos(th), -np.cos(ph) * np.sin(th)], axis=-1)
    elif model == FISHEYE:
        m = 0.5 * min(width, height)
        nx, ny = (px - 0.5 * W) / m, (0.5 * H - py) / m
        r = np.sqrt(nx * nx + ny * ny)
        tau = np.minimum(r * float(F(lens.half_fov_turns)), 0.5) * 2.0 * np.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            k = np.where(r > 0, np.sin(tau) / r, 0.0)
        l = np.stack([nx * k, ny * k, np.cos(tau)], axis=-1)
    elif model == ORTHO:
        l = np.tile(np.array([0.0, 0.0, 1.0]), (len(x), 1))
    else:
        n = width
        f = y // U(n)
        j = (y - f * U(n)).astype(np.float64)
        sc = a * 2.0 - 1.0
        tc = ((j + 0.5 - jy) / n) * 2.0 - 1.0
        one = np.ones(len(x))
        v = np.zeros((len(x), 3))
        for face in range(6):
            sel = f == face
            v[sel] = np.stack(FACE_ROWS[face](sc, tc, one), axis=-1)[sel]
        l = v * np.array([1.0, 1.0, -1.0])
    w = l[:, 0:1] * right + l[:, 1:2] * up + l[:, 2:3] * forward
    return w / np.linalg.norm(w, axis=-1, keepdims=True)
