"""The denoiser of DESIGN.md 4.11 (rt3_denoise) restated in numpy float32, vectorised over the pixels, in the kernels' operation order: every
product and sum rounds to float32 where the kernels round, and every sum adds its taps in the order of the specification.  exp is the one
function the specification leaves open; here it is the kernels' own dn_exp, step for step, so the two agree bit for bit.

denoise(colour (H, W, 4) float32, aov (H, W) AOV records or the fields albedo / normal / depth, ...) -> (H, W, 4) float32."""
import numpy as np

F = np.float32
THRESHOLD = F(2.0 ** -10)
EPS = F(1e-10)
K1 = [F(0.25), F(0.5), F(0.25)]                                         # (1, 2, 1) / 4
H1 = [F(1.0 / 16.0), F(0.25), F(0.375), F(0.25), F(1.0 / 16.0)]
DEFAULTS = dict(iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0)


EXP_POLY = [F(1.98412701e-4), F(1.38888892e-3), F(8.33333377e-3), F(4.16666679e-2), F(0.166666672), F(0.5), F(1.0), F(1.0)]


def exp32(x):
    """dn_exp of rt3_denoise.hip: k = rint(x log2 e), r = (x - k ln2_hi) - k ln2_lo, a degree-7 polynomial in Horner form, ldexp; 0 below -104."""
    x = np.asarray(x, F)
    low = ~(x >= F(-104.0)) & ~np.isnan(x)
    xx = np.where(low, F(0.0), x)
    k = np.rint(xx * F(1.44269502))
    r = (xx - k * F(0.693145751953125)) - k * F(1.42860677e-6)
    p = EXP_POLY[0]
    for c in EXP_POLY[1:]:
        p = p * r + c
    with np.errstate(invalid="ignore"):
        e = np.ldexp(p, np.where(np.isnan(k), 0, k).astype(np.int32)).astype(F)
    return np.where(low, F(0.0), e)


def lum(i):
    return (F(0.2126) * i[..., 0] + F(0.7152) * i[..., 1]) + F(0.0722) * i[..., 2]


def shift(a, dx, dy):
    """(a[y + dy, x + dx] where that pixel lies in the frame, else 0; the in-frame mask)."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    m = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        m[y0:y1, x0:x1] = True
    return out, m


def normal_weight(n_p, n_q, squarings):
    both_zero = (n_p == 0).all(-1) & (n_q == 0).all(-1)
    w = np.maximum(F(0.0), (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2])
    for _ in range(squarings):
        w = w * w
    return np.where(both_zero, F(1.0), w)


def depth_term(z_p, z_q, gz_p, d, sigma_z):
    """e_z of pairs whose depths are both finite or both infinite (other pairs: anything; the caller masks them)."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(z_p - z_q) / (sigma_z * gz_p * F(d) + EPS)
    return np.where(np.isinf(z_p), F(0.0), e)


def one_infinite(z_p, z_q):
    return np.isinf(z_p) != np.isinf(z_q)


def geometry_weight(n_p, z_p, n_q, z_q, gz_p, d, squarings, sigma_z):
    with np.errstate(over="ignore", invalid="ignore"):
        w = normal_weight(n_p, n_q, squarings) * exp32(-depth_term(z_p, z_q, gz_p, d, sigma_z))
    return np.where(one_infinite(z_p, z_q), F(0.0), w)


def fields(aov):
    if isinstance(aov, dict):
        return (np.asarray(aov["albedo"], F), np.asarray(aov["normal"], F), np.asarray(aov["depth"], F))
    return aov["albedo"].astype(F), aov["normal"].astype(F), aov["depth"].astype(F)


def prepare(colour, aov):
    """(I, L(I), albedo, normals, depths, depth slopes)."""
    albedo, n, z = fields(aov)
    c = np.asarray(colour, F)[..., :3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        i = np.where(albedo > THRESHOLD, c / albedo, c).astype(F)
    gz = np.zeros(z.shape, F)
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        zq, m = shift(z, dx, dy)
        ok = m & ~np.isinf(zq)
        with np.errstate(invalid="ignore"):
            gz = np.where(ok, np.maximum(gz, np.abs(zq - z)), gz)
    gz = np.where(np.isinf(z), F(0.0), gz).astype(F)
    return i, lum(i), albedo, n, z, gz


def moments(L, n, z, gz, squarings, sigma_z):
    sw, s1, s2 = (np.zeros(L.shape, F) for _ in range(3))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            lq, m = shift(L, dx, dy)
            if dx == 0 and dy == 0:
                w = np.ones(L.shape, F)
            else:
                w = geometry_weight(n, z, shift(n, dx, dy)[0], shift(z, dx, dy)[0], gz, max(abs(dx), abs(dy)), squarings, sigma_z)
            sw = np.where(m, sw + w, sw)
            s1 = np.where(m, s1 + w * lq, s1)
            s2 = np.where(m, s2 + w * (lq * lq), s2)
    m1, m2 = s1 / sw, s2 / sw
    return np.maximum(F(0.0), m2 - m1 * m1)


def atrous_pass(i, v, n, z, gz, step, squarings, sigma_l, sigma_z):
    gn, gd = np.zeros(v.shape, F), np.zeros(v.shape, F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, m = shift(v, dx, dy)
            k = K1[dy + 1] * K1[dx + 1]
            if dx == 0 and dy == 0:
                w = np.full(v.shape, k, F)
            else:
                w = k * geometry_weight(n, z, shift(n, dx, dy)[0], shift(z, dx, dy)[0], gz, 1, squarings, sigma_z)
            gd = np.where(m, gd + w, gd)
            gn = np.where(m, gn + w * vq, gn)
    sig = sigma_l * np.sqrt(gn / gd) + EPS
    lp = lum(i)
    sw, sv = np.zeros(v.shape, F), np.zeros(v.shape, F)
    si = np.zeros(i.shape, F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            iq, m = shift(i, step * dx, step * dy)
            vq = shift(v, step * dx, step * dy)[0]
            h = H1[dy + 2] * H1[dx + 2]
            if dx == 0 and dy == 0:
                w = np.full(v.shape, h, F)
            else:
                nq, zq = shift(n, step * dx, step * dy)[0], shift(z, step * dx, step * dy)[0]
                ez = depth_term(z, zq, gz, step * max(abs(dx), abs(dy)), sigma_z)
                el = np.abs(lp - lum(iq)) / sig
                with np.errstate(over="ignore", invalid="ignore"):
                    w = (h * normal_weight(n, nq, squarings)) * exp32(-(ez + el))
                w = np.where(one_infinite(z, zq), F(0.0), w)
            sw = np.where(m, sw + w, sw)
            si = np.where(m[..., None], si + w[..., None] * iq, si)
            sv = np.where(m, sv + (w * w) * vq, sv)
    return si / sw[..., None], sv / (sw * sw)


def denoise(colour, aov, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0, passes_out=None):
    """The whole call.  passes_out: a list that receives (I, v) after the moments and after every pass but the last."""
    squarings = int(normal_power).bit_length() - 1
    assert 1 << squarings == normal_power
    sl, sz = F(sigma_luminance), F(sigma_depth)
    i, L, albedo, n, z, gz = prepare(colour, aov)
    v = moments(L, n, z, gz, squarings, sz)
    for k in range(iterations):
        if passes_out is not None:
            passes_out.append((i, v))
        i, v = atrous_pass(i, v, n, z, gz, 1 << k, squarings, sl, sz)
    out = np.zeros(i.shape[:2] + (4,), F)
    out[..., :3] = np.where(albedo > THRESHOLD, i * albedo, i)
    return out


# ------------------------------------------------------------------------------------------------ a per-pixel form, for the self-checks
def denoise_scalar(colour, aov, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0):
    """The same specification written one pixel and one tap at a time (numpy float32 scalars): slow, for tiny frames only."""
    albedo, nrm, dep = fields(aov)
    hh, ww = dep.shape
    sq = int(normal_power).bit_length() - 1
    sl, sz = F(sigma_luminance), F(sigma_depth)
    inside = lambda x, y: 0 <= x < ww and 0 <= y < hh                        # noqa: E731

    def lum1(c):
        return (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]

    def wg(p, q, gzp, d, with_exp=None):
        zp, zq = dep[p], dep[q]
        if np.isinf(zp) != np.isinf(zq):
            return F(0.0)
        np_, nq = nrm[p], nrm[q]
        if (np_ == 0).all() and (nq == 0).all():
            wn = F(1.0)
        else:
            wn = max(F(0.0), (np_[0] * nq[0] + np_[1] * nq[1]) + np_[2] * nq[2])
            for _ in range(sq):
                wn = wn * wn
        ez = F(0.0) if np.isinf(zp) else F(abs(zp - zq) / (sz * gzp * F(d) + EPS))
        if with_exp is None:
            return F(wn * exp32(-ez)[()])
        return wn, ez

    I = np.zeros((hh, ww, 3), F)
    for y in range(hh):
        for x in range(ww):
            for c in range(3):
                a, col = albedo[y, x, c], F(colour[y, x, c])
                I[y, x, c] = col / a if a > THRESHOLD else col
    gz = np.zeros((hh, ww), F)
    for y in range(hh):
        for x in range(ww):
            if np.isinf(dep[y, x]):
                continue
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if inside(x + dx, y + dy) and not np.isinf(dep[y + dy, x + dx]):
                    gz[y, x] = max(gz[y, x], abs(dep[y + dy, x + dx] - dep[y, x]))
    L = np.array([[lum1(I[y, x]) for x in range(ww)] for y in range(hh)], F)
    v = np.zeros((hh, ww), F)
    for y in range(hh):
        for x in range(ww):
            sw = s1 = s2 = F(0.0)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    if not inside(x + dx, y + dy):
                        continue
                    w = F(1.0) if dx == dy == 0 else wg((y, x), (y + dy, x + dx), gz[y, x], max(abs(dx), abs(dy)))
                    lq = L[y + dy, x + dx]
                    sw, s1, s2 = F(sw + w), F(s1 + w * lq), F(s2 + w * F(lq * lq))
            m1, m2 = F(s1 / sw), F(s2 / sw)
            v[y, x] = max(F(0.0), F(m2 - F(m1 * m1)))
    for it in range(iterations):
        step = 1 << it
        I2, v2 = np.zeros_like(I), np.zeros_like(v)
        for y in range(hh):
            for x in range(ww):
                gn = gd = F(0.0)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if not inside(x + dx, y + dy):
                            continue
                        k = F(K1[dy + 1] * K1[dx + 1])
                        w = k if dx == dy == 0 else F(k * wg((y, x), (y + dy, x + dx), gz[y, x], 1))
                        gd, gn = F(gd + w), F(gn + w * v[y + dy, x + dx])
                sig = F(sl * np.sqrt(F(gn / gd)) + EPS)
                lp = lum1(I[y, x])
                sw = sv = F(0.0)
                si = np.zeros(3, F)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + step * dx, y + step * dy
                        if not inside(qx, qy):
                            continue
                        h = F(H1[dy + 2] * H1[dx + 2])
                        if dx == dy == 0:
                            w = h
                        elif np.isinf(dep[y, x]) != np.isinf(dep[qy, qx]):
                            continue
                        else:
                            wn, ez = wg((y, x), (qy, qx), gz[y, x], step * max(abs(dx), abs(dy)), with_exp=True)
                            el = F(abs(lp - lum1(I[qy, qx])) / sig)
                            w = F(F(h * wn) * exp32(-F(ez + el))[()])
                        sw = F(sw + w)
                        si = (si + w * I[qy, qx]).astype(F)
                        sv = F(sv + F(w * w) * v[qy, qx])
                I2[y, x] = si / sw
                v2[y, x] = F(sv / F(sw * sw))
        I, v = I2, v2
    out = np.zeros((hh, ww, 4), F)
    for y in range(hh):
        for x in range(ww):
            for c in range(3):
                a = albedo[y, x, c]
                out[y, x, c] = I[y, x, c] * a if a > THRESHOLD else I[y, x, c]
    return out
