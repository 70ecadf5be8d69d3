"""The specular-chain law (include/rt3.h "Specular-chain AOVs") restated in numpy float32, with the tracer injected.

Every operation of the law is an IEEE f32 one rounded on its own and every fused multiply-add is fma32, so this file reproduces rt3_debug_aov_bounce
(host) and rt3_render_aov_specular* (device) bit for bit, given a tracer that returns what the query engine returns: the tests compare bit patterns.
The texture and environment lookups are the restatements of texture_ref.py and environment_ref.py."""
import numpy as np

import environment_ref
import texture_ref
from environment_sample_ref import fma32

F = np.float32
MAT_FLAT, MAT_LAMBERT, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2, 3
HIT_NONE, HIT_FACE, HIT_SPHERE, HIT_INVALID = 0, 1, 2, 3
# where a chain ended (chain_aov's second result)
END_MISS, END_SURFACE, END_INVALID = 0, 1, 2


def dot(a, b):
    """Mode X's dot: fma(az, bz, fma(ay, by, ax * bx)) on (K, 3) float32."""
    return fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))


def scale(v, k):
    return (v * k[:, None]).astype(F)


def ray_valid(o, d):
    with np.errstate(all="ignore"):
        finite = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
        return finite & (np.abs(dot(d, d) - F(1.0)) <= F(2.0 ** -20))


def device_record(mats):
    """(K, 4) float32 records as the device keeps them: (rgb, param); a dielectric: (1 / ior, ., ., ior) — the law reads only [0] and [3] of it."""
    m = np.zeros((len(mats), 4), F)
    m[:, :3] = mats["rgb"]
    m[:, 3] = mats["param"]
    g = mats["kind"] == MAT_DIELECTRIC
    with np.errstate(all="ignore"):
        m[g, 0] = F(1.0) / mats["param"][g]
    return m


def step(d, p, n, mk, m, T, b, max_bounces, max_fuzz):
    """One hit of K chains: d, p, n, T (K, 3), mk (K,), m (K, 4) device records, b bounces used -> (follow (K,) bool, rgb, normal, direction)."""
    d, p, n, m, T = (np.asarray(v, F) for v in (d, p, n, m, T))
    mk = np.asarray(mk)
    max_fuzz = F(max_fuzz)
    with np.errstate(all="ignore"):
        front = dot(d, n) < F(0.0)
        n = np.where(front[:, None], n, -n).astype(F)
        glass = mk == MAT_DIELECTRIC
        colour = np.where(glass[:, None], F(1.0), m[:, :3]).astype(F)
        rgb = (T * colour).astype(F)
        may = (b < max_bounces) & (((mk == MAT_METAL) & (m[:, 3] <= max_fuzz)) | glass)
        dn = dot(d, n)
        k2 = F(2.0) * dn
        mir = np.stack([fma32(-k2, n[:, c], d[:, c]) for c in range(3)], axis=1)
        # metal
        r = scale(mir, F(1.0) / np.sqrt(dot(mir, mir)))
        absorbed = ~(dot(r, n) > F(0.0))
        # dielectric
        ri = np.where(front, m[:, 0], m[:, 3]).astype(F)
        cosv = np.where(-dn > F(1.0), F(1.0), -dn).astype(F)
        s2 = fma32(-cosv, cosv, np.full_like(cosv, 1.0))
        sinv = np.sqrt(np.where(s2 > F(0.0), s2, F(0.0)).astype(F))
        cannot = ri * sinv > F(1.0)
        e = np.stack([fma32(cosv, n[:, c], d[:, c]) * ri for c in range(3)], axis=1).astype(F)
        par = -np.sqrt(np.abs(F(1.0) - dot(e, e)))
        refr = np.stack([fma32(par, n[:, c], e[:, c]) for c in range(3)], axis=1)
        s = np.where(glass[:, None], np.where(cannot[:, None], mir, refr), r).astype(F)
        out = scale(s, F(1.0) / np.sqrt(dot(s, s)))
        follow = may & ~(~glass & absorbed) & ray_valid(p, out)
    direction = np.where(follow[:, None], out, F(0.0)).astype(F)
    return follow, rgb, n, direction


def sky(d):
    """sky() of the kernels in float32 (unfused, left to right)."""
    with np.errstate(all="ignore"):
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        t = F(0.5) * (d[:, 1] / ln + F(1.0))
        a = F(1.0) - t
        return np.stack([a * F(1.0) + t * F(c) for c in (0.5, 0.7, 1.0)], axis=1).astype(F)


def surface(scene, o, d, kind, idx, t):
    """Hit point, normal before the flip, material kind and device record (after any texture) of K hits, as k_aov_accumulate takes them."""
    k = len(o)
    p, n, m = np.zeros((k, 3), F), np.zeros((k, 3), F), np.zeros((k, 4), F)
    mk = np.zeros(k, np.uint32)
    tex = scene.get("textures")
    with np.errstate(all="ignore"):
        f = kind == HIT_FACE
        if f.any():
            faces, i = scene["faces"], idx[f]
            p[f] = (o[f] + (t[f, None] * d[f]).astype(F)).astype(F)
            n[f] = faces["normal"][i]
            fm = scene.get("fmats")
            if fm is None:
                m[f, :3], mk[f] = faces["color"][i], MAT_FLAT
            else:
                m[f], mk[f] = device_record(fm[i]), fm["kind"][i]
        s = kind == HIT_SPHERE
        if s.any():
            cr, i = scene["spheres"][idx[s]], idx[s]
            ps = np.stack([fma32(t[s], d[s][:, c], o[s][:, c]) for c in range(3)], axis=1)
            p[s] = ps
            n[s] = ((ps - cr[:, :3]).astype(F) * (F(1.0) / cr[:, 3:4]).astype(F)).astype(F)
            m[s], mk[s] = device_record(scene["smats"][i]), scene["smats"]["kind"][i]
        if tex is not None:
            for sel, face, bind in ((f, True, tex.get("tri_tex")), (s, False, tex.get("sph_tex"))):
                if bind is None or not sel.any():
                    continue
                j = np.nonzero(sel)[0]
                slots = np.asarray(bind, np.uint32)[idx[j]]
                if face:
                    g, v = scene["faces"][idx[j]], np.asarray(scene["verts"], F)
                    uv6 = np.asarray(tex["tri_uv"], F).reshape(-1, 6)[idx[j]]
                    uv = texture_ref.face_uv(v[g["v1"], :3], v[g["v2"], :3], v[g["v3"], :3], uv6, p[j])
                else:
                    uv = texture_ref.sphere_uv(n[j])
                for slot in np.unique(slots):
                    if int(slot) not in tex["images"]:                  # (TEX_NONE among them)
                        continue
                    image, wrap = tex["images"][int(slot)]
                    w = (slots == slot) & (mk[j] != MAT_DIELECTRIC)
                    texel = texture_ref.lookup(image, uv[w], texture_ref.CLAMP if wrap in ("clamp", texture_ref.CLAMP) else texture_ref.REPEAT)
                    m[j[w], :3] = texture_ref.modulate(m[j[w], :3], texel)
    return p, n, mk, m


def chain_aov(rays, trace, scene, max_bounces, max_fuzz, spp, aov_dtype, ray_dtype, black=False):
    """rays: the spp * npix primary rays (sample-major, as rt3_camera_rays / rt3_lens_rays write them); trace(rays) -> hits, rt3_intersect's rule.
    scene: dict with spheres / smats / faces / verts / fmats / textures / env as the context holds them.
    -> (aov (npix,), info): info["casts"] valid rays traced over all bounces, and per item (spp * npix) "end" (END_*), "end_kind" (the material kind the
    chain ended on, -1 for a miss), "end_index", "end_hit" (RT3_HIT_* of the end) and "bounces" (bounces used)."""
    n_items = len(rays)
    npix = n_items // spp
    o = np.ascontiguousarray(rays["origin"], F).copy()
    d = np.ascontiguousarray(rays["direction"], F).copy()
    T = np.ones((n_items, 3), F)
    L = np.zeros(n_items, F)
    albedo = np.zeros((n_items, 3), F)
    normal = np.zeros((n_items, 3), F)
    active = np.ones(n_items, bool)
    end = np.full(n_items, END_INVALID, np.int32)
    end_kind = np.full(n_items, -1, np.int32)
    end_index = np.full(n_items, 0xFFFFFFFF, np.uint32)
    end_hit = np.zeros(n_items, np.uint32)
    bounces = np.zeros(n_items, np.uint32)
    first = None
    casts = 0
    env = scene.get("env")
    for b in range(max_bounces + 1):
        ids = np.nonzero(active)[0]
        if len(ids) == 0:
            break
        q = np.zeros(len(ids), ray_dtype)
        q["origin"], q["direction"], q["t_max"] = o[ids], d[ids], F(np.inf)
        if b == 0:
            q["t_max"] = rays["t_max"]
        hits = trace(q)
        if b == 0:
            first = hits.copy()
        kind, idx, t = hits["kind"], hits["index"], hits["t"]
        casts += int((kind != HIT_INVALID).sum())
        bounces[ids] = b
        end_hit[ids] = kind
        inv = kind == HIT_INVALID                                   # (a primary ray only: albedo 0, no hit)
        active[ids[inv]] = False
        miss = kind == HIT_NONE
        if miss.any():
            j = ids[miss]
            if black:
                c = np.zeros((len(j), 3), F)
            else:
                c = environment_ref.lookup(env, d[j]) if env is not None else sky(d[j])
            with np.errstate(all="ignore"):
                albedo[j] = (T[j] * c).astype(F)
            end[j] = END_MISS
            active[j] = False
        hit = (kind == HIT_FACE) | (kind == HIT_SPHERE)
        if hit.any():
            j = ids[hit]
            p, n, mk, m = surface(scene, o[j], d[j], kind[hit], idx[hit], t[hit])
            with np.errstate(all="ignore"):
                L[j] = (L[j] + t[hit]).astype(F)
            follow, rgb, nf, nd = step(d[j], p, n, mk, m, T[j], b, max_bounces, max_fuzz)
            normal[j] = nf
            done = j[~follow]
            albedo[done] = rgb[~follow]
            end[done] = END_SURFACE
            end_kind[done] = mk[~follow]
            end_index[done] = idx[hit][~follow]
            active[done] = False
            go = j[follow]
            T[go], o[go], d[go] = rgb[follow], p[follow], nd[follow]
    assert not active.any()
    a = np.zeros((npix, 3), F)
    ns = np.zeros((npix, 3), F)
    ls = np.zeros(npix, F)
    nh = np.zeros(npix, np.uint32)
    with np.errstate(all="ignore"):
        for s in range(spp):
            sl = slice(s * npix, (s + 1) * npix)
            a = (a + albedo[sl]).astype(F)
            ns = (ns + normal[sl]).astype(F)
            ph = (first["kind"][sl] == HIT_FACE) | (first["kind"][sl] == HIT_SPHERE)
            ls = np.where(ph, (ls + L[sl]).astype(F), ls)
            nh += ph
        out = np.zeros(npix, aov_dtype)
        fs = F(spp)
        out["albedo"] = a / fs
        out["normal"] = ns / fs
        out["coverage"] = nh.astype(F) / fs
        out["depth"] = np.where(nh > 0, ls / nh.astype(F), F(np.inf))
    out["kind"], out["index"] = first["kind"][:npix], first["index"][:npix]
    info = dict(casts=casts, end=end, end_kind=end_kind, end_index=end_index, end_hit=end_hit, bounces=bounces)
    return out, info
