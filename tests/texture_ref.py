"""The image texture law (include/rt3.h "Image textures") restated in numpy float32: the lookup of (u, v), a sphere's (u, v) from its unit
outward normal, a face's (u, v) from a point of its plane, and the inputs the tests put through them.

Every operation of the law is an IEEE f32 one rounded on its own, so float32 arrays reproduce the device's tex_modulate and the host's
rt3_debug_texture_* bit for bit: the tests compare bit patterns, not values."""
import numpy as np

from optic_ref import turns

F = np.float32
REPEAT, CLAMP = 0, 1
NONE = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _axis(u, n, wrap):
    """One coordinate over n texels -> (i0, i1, w): the wrap, fx, floor, weight, the clamp in float before the conversion, the taps."""
    u = np.asarray(u, F)
    with np.errstate(all="ignore"):
        if wrap == REPEAT:
            u = u - np.floor(u)
        fx = u * F(n) - F(0.5)
        x0 = np.floor(fx)
        w = fx - x0
        k = np.fmin(np.fmax(x0, F(-1.0)), F(n) - F(1.0)).astype(np.int64)       # fmax / fmin drop a NaN: it gives -1
    if wrap == REPEAT:
        return np.where(k < 0, n - 1, k), np.where(k + 1 > n - 1, 0, k + 1), w.astype(F)
    return np.maximum(k, 0), np.minimum(k + 1, n - 1), w.astype(F)


def lookup(image, uv, wrap=REPEAT):
    """tex(u, v): image (H, W, 3 | 4) float32, row 0 on top, uv (K, 2) float32 -> (K, 3) float32."""
    image = np.asarray(image, F)
    h, w = image.shape[:2]
    uv = np.asarray(uv, F).reshape(-1, 2)
    i0, i1, wx = _axis(uv[:, 0], w, wrap)
    j0, j1, wy = _axis(uv[:, 1], h, wrap)
    rgb = image[..., :3]
    c00, c10, c01, c11 = rgb[j0, i0], rgb[j0, i1], rgb[j1, i0], rgb[j1, i1]        # cAB: column iA, row jB
    wx, wy = wx[:, None], wy[:, None]
    with np.errstate(all="ignore"):
        top = c00 + wx * (c10 - c00)
        bot = c01 + wx * (c11 - c01)
        return (top + wy * (bot - top)).astype(F)


def sphere_uv(n):
    """(u, v) of unit outward normals (K, 3) float32 -> (K, 2) float32."""
    n = np.asarray(n, F).reshape(-1, 3)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        hxz = np.sqrt(nx * nx + nz * nz)
        u = np.where(hxz > F(0.0), turns(-nx, nz), F(0.0))
        v = F(2.0) * turns(ny, hxz)
    return np.stack([u, v], axis=-1).astype(F)


def sphere_uv64(n):
    """The book's formula in float64 (v = 0 at the north pole): u = (atan2(-z, x) + pi) / 2 pi, v = acos(y) / pi, of the normalised n."""
    n = np.asarray(n, np.float64).reshape(-1, 3)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    u = (np.arctan2(-n[:, 2], n[:, 0]) + np.pi) / (2.0 * np.pi)
    v = np.arctan2(np.hypot(n[:, 0], n[:, 2]), n[:, 1]) / np.pi
    return np.stack([u, v], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def face_uv(p1, p2, p3, uv6, p):
    """(u, v) at the points p (K, 3) of faces with vertices p1, p2, p3 (3,) or (K, 3) and uv6 (6,) or (K, 6), all float32 -> (K, 2) float32."""
    p = np.asarray(p, F).reshape(-1, 3)
    p1, p2, p3 = (np.broadcast_to(np.asarray(x, F).reshape(-1, 3), p.shape) for x in (p1, p2, p3))
    t = np.broadcast_to(np.asarray(uv6, F).reshape(-1, 6), (len(p), 6))
    with np.errstate(all="ignore"):
        e1, e2, q = p2 - p1, p3 - p1, p - p1
        d11, d12, d22, q1, q2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(q, e1), _dot(q, e2)
        den = d11 * d22 - d12 * d12
        zero = den == F(0.0)
        b2 = np.where(zero, F(0.0), (d22 * q1 - d12 * q2) / den).astype(F)
        b3 = np.where(zero, F(0.0), (d11 * q2 - d12 * q1) / den).astype(F)
        b1 = (F(1.0) - b2) - b3
        u = (b1 * t[:, 0] + b2 * t[:, 2]) + b3 * t[:, 4]
        v = (b1 * t[:, 1] + b2 * t[:, 3]) + b3 * t[:, 5]
    return np.stack([u, v], axis=-1).astype(F)


def modulate(rgb, texel):
    """The shading rule: the material's rgb times the texel, per channel, in f32."""
    return (np.asarray(rgb, F) * np.asarray(texel, F)).astype(F)


def random_image(w, h, seed=0, channels=4):
    """A random texture with texels in [0, 2): float32 (h, w, channels)."""
    return np.random.default_rng(7000 + 100 * seed + 13 * w + h).uniform(0.0, 2.0, (h, w, channels)).astype(F)


def lookup_points(w, h, seed=3):
    """The (u, v) of the lookup-law tests for a w x h image: random ones in [-3, 3), every texel corner and centre (the REPEAT seam and both CLAMP
    edges among them) and their float32 neighbours, points just outside [0, 1], large and tiny values, signed zeros, NaN and +-inf."""
    rng = np.random.default_rng(seed + 31 * w + h)
    out = [rng.uniform(-3.0, 3.0, (2048, 2)), rng.uniform(0.0, 1.0, (1024, 2))]
    xs = np.concatenate([np.arange(w + 1) / w, (np.arange(w) + 0.5) / w]).astype(F)
    ys = np.concatenate([np.arange(h + 1) / h, (np.arange(h) + 0.5) / h]).astype(F)
    for dx in (xs, np.nextafter(xs, F(-9)), np.nextafter(xs, F(9)), xs + F(1), xs - F(1), xs - F(2)):
        for dy in (ys, np.nextafter(ys, F(-9)), np.nextafter(ys, F(9)), ys - F(1)):
            gx, gy = np.meshgrid(dx, dy)
            out.append(np.stack([gx.ravel(), gy.ravel()], axis=-1))
    special = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30, 1e-10, -1e-10, 0.99999994, 1.0000001, -0.99999994, 123456.75, -123456.75, 1e9, -1e9,
                        3e38, -3e38, np.inf, -np.inf, np.nan, 0.5, 0.25], F)
    gx, gy = np.meshgrid(special, special)
    out.append(np.stack([gx.ravel(), gy.ravel()], axis=-1))
    return np.ascontiguousarray(np.concatenate(out), F)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def sphere_normals(seed=4):
    """The normals of the sphere-law tests: random unit vectors; the two poles, exact and nearly; the u seam (z = 0 with x > 0, where u wraps from 1 to
    0) from both sides and with signed zeros; the other three meridians of the axes; vectors that are not finite."""
    rng = np.random.default_rng(seed)
    out = [unit(rng.normal(0.0, 1.0, (4096, 3)))]
    out.append(np.array([[0, 1, 0], [0, -1, 0], [0.0, 1, -0.0], [-0.0, -1, 0.0], [1e-30, 1, 0], [0, 1, 1e-30], [1e-20, -1, -1e-20], [1e-4, 1, 0],
                         [0, -1, -1e-4]], F))
    eps = [0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 1e-4, -1e-4]
    seam = [[x, y, z] for x in (1.0, 0.6, -1.0, -0.6) for y in (0.0, 0.8, -0.8) for z in eps if abs(x) < 1.0 or y == 0.0]
    seam += [[z, y, x] for x in (1.0, 0.6, -1.0, -0.6) for y in (0.0, 0.8, -0.8) for z in eps if abs(x) < 1.0 or y == 0.0]
    out.append(np.array(seam, F))
    out.append(np.array([[np.nan, 0, 1], [0, np.nan, 1], [1, 0, np.inf], [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, 0]], F))
    return np.ascontiguousarray(np.concatenate(out), F)


def bound_everything(n_sph, n_faces, slot=0):
    """Bindings that put `slot` on every primitive: (sphere slots | None, face slots | None)."""
    return (np.full(n_sph, slot, np.uint32) if n_sph else None, np.full(n_faces, slot, np.uint32) if n_faces else None)
