"""The emitters' sampling table and sampling law (include/rt3.h "Emitters: sampling") restated in numpy float32 and Python integers.

The table is integers wherever something is added up and every float operation of the law is an IEEE f32 one rounded on its own, so this file
reproduces rt3_debug_light_sample (host) and the device's table and shadow rays bit for bit: the tests compare bit patterns.  The fused multiply-adds
of the law are environment_sample_ref.fma32 (exact product, round-to-odd sum in float64, one rounding to f32)."""
import numpy as np

from environment_sample_ref import FLT_MAX, PI32, QUANTUM, fma32, hash_u32, u01

F = np.float32
U = np.uint32
MAT_FLAT = 0
NO_LIGHT = 0xFFFFFFFF
FOUR_PI32 = F(12.566371)
MATERIAL = np.dtype([("rgb", "<f4", 3), ("param", "<f4"), ("kind", "<u4")])      # rt3_material


def dotf(a, b):
    """z z' + (y y' + x x') as two fused multiply-adds; a, b (..., 3) float32."""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def sincos2pi(u):
    u = np.asarray(u, F)
    a = u * F(4.0)
    k = a.astype(np.int32)
    f = a - k.astype(F)
    x = f * F(1.57079637)
    x2 = x * x
    p = fma32(x2, F(-2.50521084e-8), F(2.75573192e-6))
    p = fma32(x2, p, F(-1.98412698e-4))
    p = fma32(x2, p, F(8.33333333e-3))
    p = fma32(x2, p, F(-1.66666667e-1))
    s = fma32(x * x2, p, x)
    q = fma32(x2, F(2.08767570e-9), F(-2.75573192e-7))
    q = fma32(x2, q, F(2.48015873e-5))
    q = fma32(x2, q, F(-1.38888889e-3))
    q = fma32(x2, q, F(4.16666667e-2))
    q = fma32(x2, q, F(-0.5))
    c = fma32(x2, q, F(1.0))
    kk = k & 3
    c_out = np.where(kk == 0, c, np.where(kk == 1, -s, np.where(kk == 2, -c, s)))
    s_out = np.where(kk == 0, s, np.where(kk == 1, c, np.where(kk == 2, -s, -c)))
    return c_out.astype(F), s_out.astype(F)


def unit_vector(xi0, xi1):
    """The scatter's own random unit vector (rt3_kernel_common.hpp), (K, 3) float32."""
    xi0 = np.asarray(xi0, F)
    z = fma32(F(-2.0), xi0, F(1.0))
    rr = fma32(-z, z, F(1.0))
    r = np.sqrt(np.where(rr > 0, rr, F(0.0)).astype(F))
    c, s = sincos2pi(xi1)
    return np.stack([r * c, r * s, z], axis=-1).astype(F)


def brightness(materials):
    """(n,) float32 of MATERIAL records: the positive parts of a FLAT material's rgb added (NaN-dropping max), +inf clamped; any other kind: 0."""
    rgb = np.asarray(materials["rgb"], F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        l = (np.fmax(rgb[:, 0], F(0)) + np.fmax(rgb[:, 1], F(0))) + np.fmax(rgb[:, 2], F(0))
        l = np.fmin(l, F(FLT_MAX)).astype(F)
    return np.where(np.asarray(materials["kind"]).reshape(-1) == MAT_FLAT, l, F(0.0)).astype(F)


class Faces:
    """p1, the edges, their cross product x and g2 = |x|^2 (the fused chain) of every face; all (n, 3) / (n,) float32."""
    def __init__(self, faces, verts):
        v = np.asarray(verts, F).reshape(-1, 4)[:, :3]
        with np.errstate(all="ignore"):
            self.p1 = v[faces["v1"]].reshape(-1, 3)
            self.e1 = (v[faces["v2"]].reshape(-1, 3) - self.p1).astype(F)
            self.e2 = (v[faces["v3"]].reshape(-1, 3) - self.p1).astype(F)
            e1, e2 = self.e1, self.e2
            self.x = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                               e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                               e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(F)
            self.g2 = dotf(self.x, self.x)
            self.area = (F(0.5) * np.sqrt(self.g2)).astype(F)


def weight(l, a):
    with np.errstate(all="ignore"):
        w = (l * a).astype(F)
        ok = (a > 0) & (a < np.inf) & ~np.isnan(w)
        return np.where(ok, np.fmin(w, F(FLT_MAX)), F(0.0)).astype(F)


class Table:
    """faces (GFACE) with verts and one MATERIAL each, spheres (n, 4) with one MATERIAL each; either class may be None / empty."""
    def __init__(self, faces, verts, face_materials, center_radius, sphere_materials):
        faces = np.zeros(0, np.dtype([("v1", "<u4"), ("v2", "<u4"), ("v3", "<u4")])) if faces is None else np.asarray(faces)
        fm = np.zeros(0, MATERIAL) if face_materials is None else np.asarray(face_materials)
        cr = np.zeros((0, 4), F) if center_radius is None else np.asarray(center_radius, F).reshape(-1, 4)
        sm = np.zeros(0, MATERIAL) if sphere_materials is None else np.asarray(sphere_materials)
        self.n_faces, self.n_spheres = len(faces), len(cr)
        self.faces = Faces(faces, verts if verts is not None else np.zeros((1, 4), F)) if len(faces) else None
        self.cr = cr
        with np.errstate(all="ignore"):
            sa = (FOUR_PI32 * (cr[:, 3] * cr[:, 3])).astype(F)
        self.sphere_area = sa
        wf = weight(brightness(fm), self.faces.area) if len(faces) else np.zeros(0, F)
        ws = weight(brightness(sm), sa) if len(cr) else np.zeros(0, F)
        w = np.concatenate([wf, ws]).astype(F)
        self.w = w
        wmax = w.max() if len(w) else F(0)
        with np.errstate(all="ignore"):
            scaled = np.floor(w / wmax * QUANTUM)
        self.q = np.where(w == 0, 0, np.maximum(np.nan_to_num(scaled), 1)).astype(np.uint32)
        run, sums = 0, []
        for v in self.q:                                                       # Python integers: no width, no order
            run += int(v)
            sums.append(run)
        self.cdf_ints = sums
        self.total = run
        self.cdf = np.array(sums, np.uint64)
        self.rgb = np.concatenate([np.asarray(fm["rgb"], F).reshape(-1, 3), np.asarray(sm["rgb"], F).reshape(-1, 3)])


def sample(table, base, depth):
    """The law for arrays of (base, depth): (light uint32, point (K, 3), light normal (K, 3), area, pl, a, b), all float32.  table.total must not be 0."""
    T = table
    base = np.asarray(base, U).reshape(-1)
    depth = np.broadcast_to(np.asarray(depth, U).reshape(-1), base.shape)
    with np.errstate(over="ignore"):
        ctr = U(1) + U(8) * (depth + U(1))
        w3, w4, w5, w6 = (hash_u32(base ^ hash_u32(ctr + U(k))) for k in (3, 4, 5, 6))
    targets = [(((int(h) << 32) | int(l)) * T.total) >> 64 for h, l in zip(w3, w4)]
    light = np.searchsorted(T.cdf, np.array(targets, np.uint64), side="right").astype(np.int64)     # the first index with cdf > target
    a, b = u01(w5), u01(w6)
    k = len(base)
    point, normal, area = np.zeros((k, 3), F), np.zeros((k, 3), F), np.zeros(k, F)
    isf = light < T.n_faces
    with np.errstate(all="ignore"):
        if isf.any():
            i = light[isf]
            fa, fb = a[isf], b[isf]
            flip = fa + fb > F(1.0)
            fa = np.where(flip, F(1.0) - fa, fa).astype(F)
            fb = np.where(flip, F(1.0) - fb, fb).astype(F)
            G = T.faces
            point[isf] = np.stack([fma32(fb, G.e2[i, c], fma32(fa, G.e1[i, c], G.p1[i, c])) for c in range(3)], axis=1)
            inv = (F(1.0) / np.sqrt(G.g2[i])).astype(F)
            normal[isf] = G.x[i] * inv[:, None]
            area[isf] = G.area[i]
        if (~isf).any():
            s = T.cr[light[~isf] - T.n_faces]
            v = unit_vector(a[~isf], b[~isf])
            point[~isf] = np.stack([fma32(s[:, 3], v[:, c], s[:, c]) for c in range(3)], axis=1)
            normal[~isf] = v
            area[~isf] = T.sphere_area[light[~isf] - T.n_faces]
    pl = (T.q[light].astype(F) / F(np.float64(T.total))).astype(F)
    return light.astype(U), point, normal, area, pl, a, b


def connect(table, light, point, normal, area, pl, p, n):
    """The shadow ray from hit points p (K, 3) with normals n turned towards the ray: (keep bool (K,), direction (K, 3), k (K,)) in float32, by the law's
    own operations: dropped when d2 is not finite and > 0, not cl > 0, not c > 0, or the sampled point is on the far side of a sphere seen from outside."""
    T = table
    p, n = np.asarray(p, F).reshape(-1, 3), np.asarray(n, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        D = (point - p).astype(F)
        d2 = dotf(D, D)
        inv = (F(1.0) / np.sqrt(d2)).astype(F)
        w = (D * inv[:, None]).astype(F)
        dl = dotf(normal, w)
        cl = np.abs(dl)
        c = dotf(n, w)
        keep = (d2 > 0) & (d2 < np.inf) & (cl > 0) & (c > 0)
        sph = light.astype(np.int64) >= T.n_faces
        s = T.cr[np.where(sph, light.astype(np.int64) - T.n_faces, 0)] if T.n_spheres else np.zeros((len(p), 4), F)
        u = (p - s[:, :3]).astype(F)
        outside = dotf(u, u) > s[:, 3] * s[:, 3]
        keep &= ~(sph & outside & (dl >= 0))
        k = (((c * cl) * area) / ((PI32 * d2) * pl)).astype(F)
    return keep, w, k
