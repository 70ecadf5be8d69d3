"""Float64 truth for Mode X's geometry and scattering laws.  TEST INFRASTRUCTURE.

Written from the geometry, not from oracle/rt3_oracle.c: a ray meets a sphere where |o + t d - C| = r, a triangle where the point of
its plane has non-negative barycentric coordinates; a mirror keeps the tangential part of a direction and negates the normal part; a
refracted ray keeps ri times the tangential part (Snell).  Imports neither the oracle nor the library: numpy only.

Every float32 input (vertex, centre, radius, origin, direction) is promoted to float64 exactly, so the only difference between this file
and a correct float32 evaluation is the float32 rounding, which the error bounds below count.  u = 2^-24 throughout.
"""
import numpy as np

U = 2.0 ** -24
NONE, FACE, SPHERE = 0, 1, 2
NO_INDEX = 0xFFFFFFFF
SQRT3 = 3.0 ** 0.5


# ====================================================================================================================== error bounds
def error_bound_t_face(M, t, cos, longest_edge, sin_corner, origin_err=0.0, dir_err=0.0):
    """First-order bound on |t32 - t64| of a ray/plane intersection evaluated in float32 as t = (n.p1 - n.o) / (n.d) with a stored unit
    normal n that was itself computed in float32 as normalize(cross(edge, edge)).

    M = max |coordinate| over the origin and the three vertices, cos = the cosine of the incidence angle, |d| = 1.

    * n.p1, unfused: 3 products and 2 sums, each rounded once: error <= 3u sum|n_i p_i| <= 3u |n| |p1| <= 3 sqrt(3) u M.
    * n.o: the same, 3 sqrt(3) u M.
    * the difference: one rounding of a value of at most 2 sqrt(3) M: 2 sqrt(3) u M.
      Numerator: 8 sqrt(3) u M absolute; divided by |n.d| = |cos|.
    * n.d: 3u sum|n_i d_i| <= 3u absolute, i.e. 3u / |cos| relative to the quotient; the division itself: u relative.
    * the stored normal: each edge component carries one rounding (u relative); a cross-product component a - b carries the two
      propagated edge errors and its own rounding per product (3u(|a| + |b|)) and the rounding of the difference (u |a - b|): at most
      4u |e1| |e2| per component, 4 sqrt(3) u |e1| |e2| as a vector, against a length of |e1| |e2| sin(corner): an angle of
      4 sqrt(3) u / sin(corner) <= 7u / sin(corner); normalising multiplies each component by one rounded factor (u more).  A normal tilted
      by the angle a about a point of the plane moves the hit by a |P - p1| / |cos| <= a L / |cos| along the ray, L the longest edge.
      Together 8u L / (sin(corner) |cos|).
    * a ray whose origin is only known to origin_err and whose direction to the angle dir_err (a scattered ray) adds
      (origin_err + |t| dir_err) / |cos|.

    bound = (8 sqrt(3) u M + 8u L / sin(corner) + origin_err + |t| dir_err) / |cos| + |t| u (3 / |cos| + 1)
    """
    ac = np.abs(cos)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (8.0 * SQRT3 * U * M + 8.0 * U * longest_edge / sin_corner + origin_err + np.abs(t) * dir_err) / ac \
            + np.abs(t) * U * (3.0 / ac + 1.0)


def error_bound_bary(dt, M, t, smallest_height, longest_edge, origin_err=0.0, dir_err=0.0):
    """Bound on the error of a barycentric coordinate of the float32 hit point: the point's displacement over the triangle's height on the
    edge concerned.

    * along the ray: dt (the bound above).
    * hit = o + t d: per component the product rounds (u |t d_i| <= 2u M) and the sum rounds (u M): 3 sqrt(3) u M <= 6u M as a vector.
    * hit - p: one rounding of a value of at most L per component: sqrt(3) u L <= 2u L.
    * the edge function, a cross product of an edge with hit - p and a dot product with the unit normal: 4u |e| |hit - p| as in
      error_bound_t_face, over twice the area: 4u L / height, i.e. a displacement of 4u L.
    * the ray's own uncertainty: origin_err + |t| dir_err.

    bound = (dt + 6u M + 6u L + origin_err + |t| dir_err) / smallest height
    """
    return (dt + 6.0 * U * M + 6.0 * U * longest_edge + origin_err + np.abs(t) * dir_err) / smallest_height


def error_bound_disc(eps_a, b=0.0, Q=1.0, origin_err=0.0, dir_err_oc=0.0):
    """Bound on the error of disc = h^2 - c relative to Q = |oc|^2 + r^2, for the float32 evaluation oc = C - o, h = fma chain of oc.d,
    c = fma chain of oc.oc - r^2, disc = fma(h, h, -c), which takes a = d.d to be 1.

    * oc: one rounding per component, u relative.
    * h: 3 roundings of partial sums of at most sum|oc_i d_i| <= |oc|, and the propagated u of oc: 4u |oc|.
    * c: r*r rounded (u r^2), 3 roundings of partial sums of at most |oc|^2 + r^2, twice the propagated u of oc (2u |oc|^2): <= 5u Q.
    * disc: 2 |h| dh + dc + its own rounding: 8u |oc|^2 + 5u Q + u |disc| <= 14u Q.
    * a = d.d differs from 1 by eps_a: disc64 = h^2 - a c moves by eps_a |c| <= eps_a Q.
    * a ray uncertain by origin_err and the angle dir_err passes the centre at a distance b uncertain by db = origin_err + |oc| dir_err;
      disc = a r^2 - a b^2 moves by 2 b db + db^2.

    bound = 14u + eps_a + (2 b db + db^2) / Q
    """
    db = origin_err + dir_err_oc
    return 14.0 * U + eps_a + (2.0 * b * db + db * db) / Q


def error_bound_t_sphere(oc_len, Q, s, t, c_abs, eps_a, b=0.0, origin_err=0.0, dir_err=0.0):
    """First-order bound on |t32 - t64| of a root t = h -+ sqrt(disc) of the float32 evaluation above; s = sqrt(disc64), Q = |oc|^2 + r^2.

    * dh = 4u |oc|.
    * sqrt: d(disc) / (2 s) + its own rounding = (13u Q + u s^2) / (2 s) + u s = 6.5u Q / s + 1.5u s.
    * the sum h -+ s: u |t|.
    * a != 1: dt/da = -t/a + c/(2 a s): eps_a (|t| + |c| / (2 s)).
    * an uncertain ray: dh <= db and ds <= b db / s with db = origin_err + |oc| dir_err: db (1 + b / s).

    bound = 4u |oc| + 6.5u Q / s + 1.5u s + u |t| + eps_a (|t| + |c| / (2 s)) + db (1 + b / s)
    """
    db = origin_err + oc_len * dir_err
    with np.errstate(divide="ignore", invalid="ignore"):
        return 4.0 * U * oc_len + 6.5 * U * Q / s + 1.5 * U * s + U * np.abs(t) + eps_a * (np.abs(t) + c_abs / (2.0 * s)) + db * (1.0 + b / s)


def error_bound_normal_face(sin_corner):
    """Angle between the stored float32 normal and the plane's: 8u / sin(corner), derived in error_bound_t_face."""
    return 8.0 * U / sin_corner


def error_bound_normal_sphere(dt, M, r):
    """Angle between (fma(t, d, o) - C) * (1 / r) in float32 and the float64 normal: the point is off by dt along the ray and by one rounding
    per component (sqrt(3) u M); p - C rounds once more (u r as a vector, generously), 1 / r and the product twice (2u relative, no angle,
    counted all the same): (dt + sqrt(3) u M) / r + 3u."""
    return (dt + SQRT3 * U * M) / r + 3.0 * U


def error_bound_dir(cam, width, height, dir_len, lens_radius=0.0):
    """Angle between Mode X's float32 primary direction and camera_ray's, for dir = ((llc + u hor) + v ver) - org, normalised.

    * the jitter (s + xi) / e - 1/2 from an exact xi: 3 roundings of values of at most 1 after the division: 3u pixels.
    * u = (x + j) / (W - 1): the sum rounds once (u (x + 1)), the quotient once: du <= (u (x + 1) + 3u) / (W - 1) + u <= 2u + 4u / (W - 1); v alike.
    * per component, with S_i = |llc_i| + |hor_i| + |ver_i| + |org_i| bounding every intermediate: 2 products and 3 sums, 5 roundings of at most
      u S_i, and du |hor_i| + dv |ver_i| <= du S_i.  As a vector: (5 + 2 + 4 / (min(W, H) - 1)) u |S|.
    * thin lens: offset = (R sqrt(xi) cos) U + (R sqrt(xi) sin) V.  sincos2pi is a Taylor polynomial on [0, pi/2): truncation x^13 / 13! <=
      5.7e-8 < u, the rounded constant pi/2 and the product by it 3u of an argument below 1.6, Horner's last two steps 2u: 6u absolute on
      cos and sin.  sqrt, the two products and the rounded unit axes (a dot product, a sqrt, a division: 3.5u) add 6.5u relative; the sum of the two
      terms one rounding each: 14u R per axis term, 20u R as a vector.  It enters the direction once, and one more rounding of at most u S_i.
    * normalising: each component times one rounded factor: u of angle; a 2u margin covers the second-order terms.

    bound = ((8 + 4 / (min(W, H) - 1)) u |S| + 20u R) / |dir| + 2u
    """
    S = sum(np.abs(np.asarray(getattr(cam, f), np.float64)) for f in ("lower_left_corner", "horizontal", "vertical", "origin"))
    Sn = float(np.linalg.norm(S))
    return ((8.0 + 4.0 / (min(width, height) - 1.0)) * U * Sn + 20.0 * U * lens_radius) / dir_len + 2.0 * U


def error_bound_origin(cam, lens_radius=0.0):
    """|origin32 - origin64| of a primary ray: the lens offset's 20u R (error_bound_dir) and the rounding of org + offset, u (|org| + R)."""
    o = float(np.linalg.norm(np.asarray(cam.origin, np.float64)))
    return 20.0 * U * lens_radius + U * (o + lens_radius)


# ====================================================================================================================== nearest hit
def _face_arrays(faces, verts):
    v = np.asarray(verts, np.float64)[:, :3]
    if getattr(faces, "dtype", None) is not None and faces.dtype.names:
        idx = np.stack([faces["v1"], faces["v2"], faces["v3"]], axis=1).astype(np.int64)
    else:
        idx = np.asarray(faces, np.int64).reshape(-1, 3)
    p1, p2, p3 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    e1, e2, e3 = p2 - p1, p3 - p1, p3 - p2
    g = np.cross(e1, e2)
    a2 = np.linalg.norm(g, axis=1)
    l1, l2, l3 = (np.linalg.norm(e, axis=1) for e in (e1, e2, e3))
    L = np.maximum(np.maximum(l1, l2), l3)
    A2, A3 = np.cross(e2, g) / (a2 * a2)[:, None], np.cross(g, e1) / (a2 * a2)[:, None]
    return dict(p1=p1, g=g, a2=a2, L=L, hmin=a2 / L, sin1=a2 / (l1 * l2), gp1=(g * p1).sum(axis=1), A2=A2, A3=A3,
                A2p1=(A2 * p1).sum(axis=1), A3p1=(A3 * p1).sum(axis=1),
                M=np.max(np.abs(np.concatenate([p1, p2, p3], axis=1)), axis=1))


def _min_ratio(slacks, bounds):
    """Signed slack / bound of the most critical condition, with that condition's |slack| and bound."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.stack([np.where(b > 0, s / b, np.where(s > 0, np.inf, np.where(s < 0, -np.inf, 0.0))) for s, b in zip(slacks, bounds)])
    rho = np.where(np.isnan(rho), 0.0, rho)
    k = np.argmin(rho, axis=0)[None]
    pick = lambda a: np.take_along_axis(np.stack([np.broadcast_to(x, rho.shape[1:]) for x in a]), k, axis=0)[0]   # noqa: E731
    return pick(list(rho)), np.abs(pick(slacks)), pick(bounds)


def nearest_hit(origins, directions, t_min, t_max, spheres=None, faces=None, verts=None, origin_err=0.0, dir_err=0.0, chunk=1024):
    """Brute-force float64 nearest hit of N rays against faces (tested first) and spheres.

    Sphere: the two roots of a t^2 - 2 h t + c = 0 (a = d.d, h = (C - o).d, c = |C - o|^2 - r^2); the near root if it is > t_min, else
    the far root; a hit needs t > t_min.  Triangle: the plane of the three vertices, barycentric coordinates >= 0, t >= t_min.  A hit
    needs t < t_max; on equal t the earlier primitive wins, faces before spheres.

    Returns a dict of arrays over the rays: kind, index, t (+inf on a miss), normal (geometric, facing the ray; 0 on a miss), t_bound
    (error_bound_t of the winner), normal_bound, and the margin record: own_edge / own_bound (the winner's distance from its most critical
    decision edge — disc relative to |oc|^2 + r^2, a barycentric coordinate, t - t_min, t_max - t, a root's distance from t_min — and that
    edge's bound), gap / gap_bound (the runner-up's t minus the winner's; the sum of the two error_bound_t), other_edge / other_bound (the
    same edge distance of the non-winner closest to its own decision edge among those that would have won had they hit).  ambiguous =
    any distance below its bound.  origin_err / dir_err (scalars or per ray): what is already uncertain about the rays themselves.
    t_max: a scalar, one value per ray, or a function (slice of the rays, the t an unlimited ray would hit at) -> that slice's t_max, for
    limits drawn around the true hit; the record's t_max holds what it returned."""
    o_all = np.asarray(origins, np.float64).reshape(-1, 3)
    d_all = np.asarray(directions, np.float64).reshape(-1, 3)
    N = len(o_all)
    tmax_all = None if callable(t_max) else np.broadcast_to(np.asarray(t_max, np.float64), (N,))
    eo_all = np.broadcast_to(np.asarray(origin_err, np.float64), (N,))
    ed_all = np.broadcast_to(np.asarray(dir_err, np.float64), (N,))
    t_min = float(t_min)
    nf = 0 if faces is None else len(faces)
    ns = 0 if spheres is None else len(spheres)
    F = _face_arrays(faces, verts) if nf else None
    S = np.asarray(spheres, np.float64).reshape(-1, 4) if ns else None
    out = dict(kind=np.zeros(N, np.uint32), index=np.full(N, NO_INDEX, np.uint32), t=np.full(N, np.inf), normal=np.zeros((N, 3)),
               t_bound=np.zeros(N), normal_bound=np.zeros(N), own_edge=np.full(N, np.inf), own_bound=np.zeros(N), gap=np.full(N, np.inf),
               gap_bound=np.zeros(N), other_edge=np.full(N, np.inf), other_bound=np.zeros(N), t_max=np.full(N, np.inf))
    for lo in range(0, N, chunk):
        sl = slice(lo, min(lo + chunk, N))
        o, d = o_all[sl], d_all[sl]
        eo, ed = eo_all[sl][:, None], ed_all[sl][:, None]
        n = len(o)
        a = (d * d).sum(axis=1)[:, None]
        dl = np.sqrt(a)
        # per primitive class, (n, P) arrays: the candidate t and its bound; signed slack / bound of the most critical condition other than
        # t < t_max, with that condition's |slack| and bound; the same for a sphere's root choice; the decision without t_max
        T, DT, RHO, EDGE, BND, ROOT, ROOT_EDGE, ROOT_BND, HIT = [], [], [], [], [], [], [], [], []
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if nf:
                gd = d @ F["g"].T                                       # (n, F)
                t = (F["gp1"][None] - o @ F["g"].T) / gd
                cos = gd / (F["a2"][None] * dl)
                # barycentric coordinates of P = o + t d: the weights of p2 and p3 are linear in P, (P - p1).A2 and (P - p1).A3
                b2 = (o @ F["A2"].T - F["A2p1"][None]) + t * (d @ F["A2"].T)
                b3 = (o @ F["A3"].T - F["A3p1"][None]) + t * (d @ F["A3"].T)
                b1 = 1.0 - b2 - b3
                M = np.maximum(F["M"][None], np.abs(o).max(axis=1)[:, None])
                tl = t * dl                                             # length along the ray
                dt = error_bound_t_face(M, tl, cos, F["L"][None], F["sin1"][None], eo, ed) / dl
                bb = error_bound_bary(dt * dl, M, tl, F["hmin"][None], F["L"][None], eo, ed)
                rho, edge, bnd = _min_ratio([np.minimum(np.minimum(b1, b2), b3), t - t_min], [bb, dt])
                dead = ~np.isfinite(t)                                  # n.d = 0: no intersection
                rho = np.where(dead, -np.inf, rho)
                HIT.append((b1 >= 0) & (b2 >= 0) & (b3 >= 0) & (t >= t_min) & ~dead)
                T.append(np.where(dead, np.inf, t)); DT.append(np.where(dead, 0.0, dt)); RHO.append(rho); EDGE.append(edge); BND.append(bnd)
                ROOT.append(np.full(t.shape, np.inf)); ROOT_EDGE.append(np.zeros(t.shape)); ROOT_BND.append(np.zeros(t.shape))
            if ns:
                oc = S[None, :, :3] - o[:, None]                        # (n, S, 3)
                r = S[None, :, 3]
                h = (oc * d[:, None]).sum(axis=2)
                oc2 = (oc * oc).sum(axis=2)
                c = oc2 - r * r
                Q = oc2 + r * r
                disc = h * h - a * c
                ocl = np.sqrt(oc2)
                bimp = np.sqrt(np.maximum(oc2 - h * h / a, 0.0))
                eps_a = np.abs(a - 1.0)
                s = np.sqrt(np.maximum(disc, 0.0))
                near, far = (h - s) / a, (h + s) / a
                t = np.where(near > t_min, near, far)
                bd = error_bound_disc(eps_a, bimp, Q, eo, ocl * ed)
                dt0 = error_bound_t_sphere(ocl, Q, s, 0.0, np.abs(c), eps_a, bimp, eo, ed)      # the part that does not depend on the root
                per_t = U + eps_a
                dt, dtn, dtf = dt0 + per_t * np.abs(t), dt0 + per_t * np.abs(near), dt0 + per_t * np.abs(far)
                rho, edge, bnd = _min_ratio([disc / Q, far - t_min], [bd, dtf])
                HIT.append((disc > 0) & (t > t_min))
                ROOT.append(np.where(disc > 0, np.abs(near - t_min) / dtn, np.inf))             # the root choice itself
                ROOT_EDGE.append(np.abs(near - t_min)); ROOT_BND.append(dtn)
                graze = disc <= 0                                       # would hit near the closest approach, if at all
                t = np.where(graze, h / a, t)
                dt = np.where(graze, np.sqrt(2.0 * bd * Q) + 8.0 * U * ocl, dt)
                T.append(t); DT.append(dt); RHO.append(rho); EDGE.append(edge); BND.append(bnd)
        if not T:
            continue
        t, dt, rho, edge, bnd, root, root_edge, root_bnd, hit = (
            np.concatenate(x, axis=1) for x in (T, DT, RHO, EDGE, BND, ROOT, ROOT_EDGE, ROOT_BND, HIT))
        rows = np.arange(n)
        if callable(t_max):                                             # drawn from the hit an unlimited ray would have
            tmax = np.asarray(t_max(sl, np.where(hit, t, np.inf).min(axis=1)), np.float64)
            out["t_max"][sl] = tmax
        else:
            tmax = tmax_all[sl]
        tmax = tmax[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            if np.isfinite(tmax).any():                                 # the condition t < t_max joins the others
                st = tmax - t
                rt = np.where(dt > 0, st / dt, np.where(st > 0, np.inf, -np.inf))
                rt = np.where(np.isnan(rt), 0.0, rt)
                use = rt < rho
                rho, edge, bnd = np.where(use, rt, rho), np.where(use, np.abs(st), edge), np.where(use, dt, bnd)
                hit = hit & (t < tmax)
            use = root < np.abs(rho)                                    # an uncertain root choice leaves the whole pair uncertain
            rho, edge, bnd = np.where(use, np.where(rho < 0, -root, root), rho), np.where(use, root_edge, edge), np.where(use, root_bnd, bnd)
        tw = np.where(hit, t, np.inf)
        w = np.argmin(tw, axis=1)                                       # first minimum: faces first, then the earlier index
        has = np.isfinite(tw[rows, w])
        t_win = np.where(has, tw[rows, w], np.inf)
        dt_win = np.where(has, dt[rows, w], 0.0)
        kind = np.where(has, np.where(w < nf, FACE, SPHERE), NONE).astype(np.uint32)
        index = np.where(has, np.where(w < nf, w, w - nf), NO_INDEX).astype(np.uint32)
        notw = np.ones_like(hit)
        notw[rows[has], w[has]] = False
        with np.errstate(invalid="ignore", divide="ignore"):
            # the runner-up among the reference's own hits
            gb = dt + dt_win[:, None]
            gr = np.where(hit & notw, (t - t_win[:, None]) / gb, np.inf)
            gr = np.where(np.isnan(gr), 0.0, gr)
            k = np.argmin(gr, axis=1)
            has_gap = np.isfinite(gr[rows, k]) & has
            gap = np.where(has_gap, t[rows, k] - t_win, np.inf)
            gap_bound = np.where(has_gap, gb[rows, k], 0.0)
            # non-winners close to their own decision edge that would win if the edge fell the other way
            threat = notw & (np.abs(rho) < 1.0) & (t - dt < (t_win + dt_win)[:, None])
            ar = np.where(threat, np.abs(rho), np.inf)
            k2 = np.argmin(ar, axis=1)
            has_o = np.isfinite(ar[rows, k2])
        out["kind"][sl], out["index"][sl], out["t"][sl] = kind, index, t_win
        out["t_bound"][sl] = dt_win
        out["own_edge"][sl] = np.where(has, edge[rows, w], np.inf)
        out["own_bound"][sl] = np.where(has, bnd[rows, w], 0.0)
        out["gap"][sl], out["gap_bound"][sl] = gap, gap_bound
        out["other_edge"][sl] = np.where(has_o, edge[rows, k2], np.inf)
        out["other_bound"][sl] = np.where(has_o, bnd[rows, k2], 0.0)
        # the geometric normal facing the ray
        nrm = np.zeros((n, 3))
        nb = np.zeros(n)
        isf = kind == FACE
        if isf.any():
            fi = index[isf].astype(np.int64)
            g = F["g"][fi] / F["a2"][fi][:, None]
            nrm[isf] = g
            nb[isf] = error_bound_normal_face(F["sin1"][fi])
        iss = kind == SPHERE
        if iss.any():
            si = index[iss].astype(np.int64)
            p = o[iss] + t_win[iss][:, None] * d[iss]
            nrm[iss] = (p - S[si, :3]) / S[si, 3:4]
            Ms = np.maximum(np.abs(o[iss]).max(axis=1), np.abs(S[si, :3]).max(axis=1) + S[si, 3])
            nb[iss] = error_bound_normal_sphere(dt_win[iss] * dl[iss, 0], Ms, S[si, 3])
        flip = (nrm * d).sum(axis=1) > 0
        nrm[flip] = -nrm[flip]
        out["normal"][sl], out["normal_bound"][sl] = nrm, nb
    out["ambiguous"] = ambiguous(out)
    return out


def ambiguous(rec):
    """A ray is ambiguous when any margin of its record is below that margin's bound."""
    return (rec["own_edge"] < rec["own_bound"]) | (rec["gap"] < rec["gap_bound"]) | (rec["other_edge"] < rec["other_bound"])


# ====================================================================================================================== camera
def hash_u32(x):
    """The one-at-a-time hash step h(x) of DESIGN.md 4.2 on uint32 arrays."""
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    m = np.uint64(0xFFFFFFFF)
    x = (x + (x << np.uint64(10))) & m
    x = x ^ (x >> np.uint64(6))
    x = (x + (x << np.uint64(3))) & m
    x = x ^ (x >> np.uint64(11))
    x = (x + (x << np.uint64(15))) & m
    return x.astype(np.uint32)


def hash2(a, b):
    """h2(a, b) = h(a ^ h(b))."""
    return hash_u32(np.asarray(a, np.uint32) ^ hash_u32(b))


def u01(m):
    """u01(m) = bits((m & 0x7FFFFF) | 0x3F800000) - 1: the 23 low bits as a fraction, exact in float64."""
    return (np.asarray(m, np.uint32) & np.uint32(0x7FFFFF)).astype(np.float64) * 2.0 ** -23


def sample_keys(width, seed, x, y, s):
    """base = h2(y W + x, h2(s, seed)); x, y of the full frame."""
    pix = (np.asarray(y, np.uint64) * np.uint64(width) + np.asarray(x, np.uint64)).astype(np.uint32)
    return hash2(pix, hash2(np.asarray(s, np.uint32), np.uint32(seed)))


def rnd(base, ctr):
    return u01(hash2(base, np.uint32(ctr)))


def camera_samples(width, spp, seed, x, y, s):
    """(jitter (n, 2) in pixel units, lens sample (n, 2) = (xi2, xi3), base keys) of samples s of pixels (x, y): counters 1-4 of DESIGN.md 4.1."""
    base = sample_keys(width, seed, x, y, s)
    s = np.asarray(s, np.int64)
    jit = np.zeros((len(base), 2))
    if spp > 1:
        xi0, xi1 = rnd(base, 1), rnd(base, 2)
        e = int(round(spp ** 0.5))
        if e * e == spp:
            jit[:, 0] = ((s % e) + xi0) / e - 0.5
            jit[:, 1] = ((s // e) + xi1) / e - 0.5
        else:
            jit[:, 0], jit[:, 1] = xi0 - 0.5, xi1 - 0.5
    return jit, np.stack([rnd(base, 3), rnd(base, 4)], axis=1), base


def camera_ray(cam, params, x, y, jitter=None, lens_sample=None):
    """The primary ray of pixel (x, y) (full frame, row 0 on top) in float64 from the four camera vectors: through the image-plane point
    llc + u hor + v ver, u = (x + jx) / (W - 1), v = (H - 1 - y + jy) / (H - 1); from the camera origin, or (thin lens, lens_radius > 0,
    lens_sample = (xi2, xi3)) from origin + r (cos phi hor/|hor| + sin phi ver/|ver|), r = lens_radius sqrt(xi2), phi = 2 pi xi3, through
    the same image-plane point.  Returns (origin (n, 3), unit direction (n, 3), |unnormalised direction| (n,))."""
    org, hor, ver, llc = (np.asarray(getattr(cam, f), np.float64) for f in ("origin", "horizontal", "vertical", "lower_left_corner"))
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    j = np.zeros((len(x), 2)) if jitter is None else np.asarray(jitter, np.float64)
    u = (x + j[:, 0]) / (params.width - 1.0)
    v = ((params.height - 1.0 - y) + j[:, 1]) / (params.height - 1.0)
    target = llc[None] + u[:, None] * hor[None] + v[:, None] * ver[None]
    o = np.broadcast_to(org, target.shape).copy()
    R = float(params.lens_radius)
    if R > 0.0:
        ls = np.asarray(lens_sample, np.float64)
        rr = R * np.sqrt(ls[:, 0])
        phi = 2.0 * np.pi * ls[:, 1]
        o = o + (rr * np.cos(phi))[:, None] * (hor / np.linalg.norm(hor))[None] + (rr * np.sin(phi))[:, None] * (ver / np.linalg.norm(ver))[None]
    d = target - o
    ln = np.linalg.norm(d, axis=1)
    return o, d / ln[:, None], ln


def owned_rows(params):
    """Full-frame rows of a shard, in the order of its compact buffer: row y belongs to shard (y div tile_rows) mod tile_count."""
    ys = np.arange(params.height)
    if params.tile_count <= 1:
        return ys
    return ys[(ys // params.tile_rows) % params.tile_count == params.tile_index]


# ====================================================================================================================== scattering
def reflect(d, n):
    """Mirror law: the normal component of d changes sign, d - 2 (d.n) n."""
    d, n = np.asarray(d, np.float64), np.asarray(n, np.float64)
    return d - 2.0 * (d * n).sum(axis=-1, keepdims=True) * n


def refract(d, n, ri):
    """Snell: unit d meets the surface with unit normal n (facing d: d.n < 0), ri = n_in / n_out.  The tangential part scales by ri,
    the normal part is what keeps the length 1.  Returns (direction, total-internal-reflection mask); the direction is NaN where total."""
    d, n = np.asarray(d, np.float64), np.asarray(n, np.float64)
    ri = np.asarray(ri, np.float64)[..., None] if np.ndim(ri) else ri
    cos = -(d * n).sum(axis=-1, keepdims=True)
    tang = ri * (d + cos * n)
    k = 1.0 - (tang * tang).sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        out = tang - np.sqrt(k) * n
    return out, (k < 0.0)[..., 0]


def schlick(cos, ri):
    """Schlick's reflectance: r0 + (1 - r0) (1 - cos)^5 with r0 = ((1 - ri) / (1 + ri))^2."""
    r0 = ((1.0 - ri) / (1.0 + ri)) ** 2
    return r0 + (1.0 - r0) * (1.0 - np.asarray(cos, np.float64)) ** 5


def form_factor_sphere(p, n, centre, radius):
    """The fraction of a cosine-weighted hemisphere at the surface point p (unit normal n) that a sphere wholly above p's horizon fills:
    (R / D)^2 cos(theta), D = |C - p|, theta between n and C - p (the Nusselt analogue of a spherical cap).  Asserts the horizon condition
    n.(C - p) > R."""
    w = np.asarray(centre, np.float64)[None] - np.asarray(p, np.float64)
    D = np.linalg.norm(w, axis=-1)
    up = (w * n).sum(axis=-1)
    assert (up > radius).all(), "the sphere dips below a hit point's horizon"
    return (radius / D) ** 2 * (up / D)


def reflect_error(dir_err, normal_err):
    """Angle error of a reflected direction: a mirror is an isometry of d (dir_err passes unchanged), and turning the normal by an angle turns
    the reflected ray by twice that; 2 (d.n) and the three fmas round 4 times on values of at most 2, the normalisation after it once
    more: 10u."""
    return dir_err + 2.0 * normal_err + 10.0 * U


def refract_error(dir_err, normal_err, ri, cos_in, cos_out):
    """Angle error of a refracted direction.  sin(out) = ri sin(in): d(out) = ri cos(in) / cos(out) d(in); the incidence angle is uncertain by
    dir_err + normal_err, and the frame the outgoing angle is measured in turns with the normal (normal_err).  The float32 evaluation
    (cos, the tangential part times ri, sqrt|1 - |tang|^2|, two fmas, normalise) rounds about 12 times on values of at most 1; the
    square root amplifies the error of |tang|^2 (4u) by 1 / (2 cos(out)^2) in angle: 12u + 4u / cos(out)^2."""
    return ri * cos_in / cos_out * (dir_err + normal_err) + normal_err + 12.0 * U + 4.0 * U / (cos_out * cos_out)


# ====================================================================================================================== closed forms
def integrating_sphere(r, R, albedo, E, max_depth):
    """A FLAT sphere of radius r and radiance E at the centre of a Lambert sphere of radius R and albedo a, seen from between the two by a
    ray that meets the wall first.  At every wall point the emitter fills the same cosine-weighted share of the hemisphere, F = (r / R)^2
    (form_factor_sphere with D = R and theta = 0), and everything else of it is wall.  A path therefore meets the emitter after j wall
    hits with probability (1 - F)^(j - 1) F and then returns a^j E; max_depth = D casts at most D rays, so j runs from 1 to D - 1 (the
    first cast meets the wall, the j-th scattered ray is cast j + 1) and a path still on the wall after D casts returns 0.  Ray j + 1 is
    cast iff the first j - 1 scattered rays met the wall.  Exact, so the standard deviation of a sample is exact too."""
    F = (float(r) / float(R)) ** 2
    j = np.arange(1, int(max_depth), dtype=np.float64)
    alive = (1.0 - F) ** (j - 1.0)
    mean = E * F * (albedo ** j * alive).sum()
    second = E * E * F * (albedo ** (2.0 * j) * alive).sum()
    return dict(F=F, mean=mean, second=second, sigma=float(np.sqrt(second - mean * mean)), casts=1.0 + alive.sum())


def fuzz_absorption(cos, f):
    """Metal with fuzz f: the scattered direction is r + f u, r the unit mirror direction (r.n = cos, the cosine of incidence) and u
    uniform on the unit sphere; the sample is absorbed iff (r + f u).n <= 0, i.e. u.n <= -cos / f.  u.n is uniform on [-1, 1]
    (Archimedes: the area of a sphere between two parallel planes depends on their distance only), so P = max(0, (1 - cos / f) / 2)."""
    return np.maximum(0.0, 0.5 * (1.0 - np.asarray(cos, np.float64) / f))


def sky(d):
    """The two-colour sky along unit directions d: (1 - t) (1, 1, 1) + t (0.5, 0.7, 1.0), t = (d_y + 1) / 2."""
    d = np.asarray(d, np.float64)
    t = 0.5 * (d[..., 1] / np.linalg.norm(d, axis=-1) + 1.0)
    return (1.0 - t)[..., None] * np.ones(3) + t[..., None] * np.array([0.5, 0.7, 1.0])


def error_bound_sky(dir_err):
    """|channel32 - channel64| of the sky along a float32 primary direction that is dir_err (an angle, error_bound_dir: the normalisation
    is counted there) off the float64 one.

    * d_y moves by at most dir_err.  The sky normalises once more, y / sqrt(d.d): the dot product rounds 5 times on values of at most 1
      (2.5u on the length), the square root and the quotient once each: 4.5u on a value of at most 1.
    * t = (y + 1) / 2, rounded once: dt <= (dir_err + 4.5u) / 2 + u.
    * a channel 1 - t (1 - c), c >= 0.5, evaluated as (1 - t) + t c: it moves by (1 - c) dt <= dt / 2; 1 - t, the product t c and the sum
      round once each on values of at most 1 (3u); the float32 constant 0.7 is within 0.7u of 0.7 (u more, generously).

    bound = dir_err / 4 + 1.625u + 4u <= dir_err / 4 + 6u
    """
    return 0.25 * np.asarray(dir_err, np.float64) + 6.0 * U


def pack(rgb, gamma2):
    """RGBA8 of linear float32 colours (n, 3), promoted exactly: byte = round(255 clip(g(x), 0, 1)), g the square root (gamma 2) or the
    identity; r << 24 | g << 16 | b << 8 | 0xFF.  Returns (words, bytes (n, 3), tie): tie marks the channels whose 255 g(x) lies within
    255 * 4u * max(1, g(x)) of a half-integer — the float32 evaluation rounds g(x) and the product by 255 once each (2u relative) and is
    given twice that."""
    x = np.asarray(rgb, np.float32).astype(np.float64).reshape(-1, 3)
    g = np.sqrt(np.maximum(x, 0.0)) if gamma2 else x
    v = 255.0 * np.clip(g, 0.0, 1.0)
    b = np.floor(v + 0.5).astype(np.uint32)
    raw = 255.0 * g
    tie = (np.abs(raw - np.floor(raw) - 0.5) <= 255.0 * 4.0 * U * np.maximum(1.0, g)) & (raw > 0.0) & (raw < 255.5)
    return (b[:, 0] << 24) | (b[:, 1] << 16) | (b[:, 2] << 8) | np.uint32(0xFF), b, tie
