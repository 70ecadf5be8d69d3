// rt3_path.hpp — per-wave path bookkeeping of Mode X: refill (plain and through the ray stock) and shade_lane()
// Part of rt3_device.hip (one translation unit, gfx950 only); included from there, in this order.
#pragma once

namespace {

// Batched ray queries: the QUERY form of a trace kernel takes its rays from the caller's buffer instead of the camera
// and stores the nearest hit (or the occlusion word) instead of shading.  One result per ray, written with one vector store.
__device__ __forceinline__ void query_store(const TraceArgs& A, uint32_t slot, uint32_t kind, uint32_t idx, float t) {
    if (A.q_occluded) reinterpret_cast<uint32_t*>(A.q_out)[slot] = kind == RT3_HIT_INVALID ? 0xFFFFFFFFu : (kind != RT3_HIT_NONE ? 1u : 0u);
    else reinterpret_cast<uint4*>(A.q_out)[slot] = make_uint4(__float_as_uint(t), kind, idx, 0u);
}
// Ray `item` of the caller's buffer (two 16-byte loads).  An invalid ray — non-finite origin or direction, |d.d - 1| > 2^-20 (the sphere test's
// a = 1 and the filter's bound of DESIGN.md 5.2c need a unit direction), t_max NaN or <= t_min — gets RT3_HIT_INVALID here and is never traced.
__device__ __forceinline__ bool query_ray(const TraceArgs& A, uint32_t item, Path& P) {
    const float4* r = A.q_rays + 2 * (size_t)item;
    const float4 a = r[0], b = r[1];
    P.ox = a.x; P.oy = a.y; P.oz = a.z; P.tmax = a.w;
    P.dx = b.x; P.dy = b.y; P.dz = b.z;
    P.slot = item; P.depth = 0;
    const float dd = dotf(b.x, b.y, b.z, b.x, b.y, b.z);
    const bool finite = __builtin_isfinite(a.x) & __builtin_isfinite(a.y) & __builtin_isfinite(a.z) &
                        __builtin_isfinite(b.x) & __builtin_isfinite(b.y) & __builtin_isfinite(b.z);
    const bool ok = finite && __builtin_fabsf(dd - 1.0f) <= 0x1p-20f && a.w > A.t_min;      // (a NaN t_max fails the last test)
    if (!ok) query_store(A, item, RT3_HIT_INVALID, 0xFFFFFFFFu, __builtin_nanf(""));
    return ok;
}

// The rays form of a path kernel (rt3_radiance*): item `item` is sample A.s0 + item / n of ray item % n of the caller's buffer
// (n = A.npix).  The loader fills the whole Path as start_path() does — origin and direction as they stand in the buffer, throughput 1, light 0, depth 0,
// base = hash2(key, hash2(s, seed)) with the ray's key in the pixel index's place — so that everything behind the refill is the render's.  Valid rays:
// query_ray's rule and t_max == +inf (a finite t_max is reserved); an invalid one gets a NaN record in the sample storage and is never traced.
__device__ __forceinline__ bool rays_path(const TraceArgs& A, uint32_t item, Path& P) {
    const uint32_t sb = fdiv(item, A.div_npix), ray = item - sb * A.npix;
    const float4* r = A.q_rays + 2 * (size_t)ray;
    const float4 a = r[0], b = r[1];
    const uint32_t key = A.ray_keys ? A.ray_keys[ray] : ray;
    P.ox = a.x; P.oy = a.y; P.oz = a.z;
    P.dx = b.x; P.dy = b.y; P.dz = b.z;
    P.tr = P.tg = P.tb = 1.0f;
    P.lr = P.lg = P.lb = 0.0f;
    P.slot = item; P.base = hash2(key, hash2(A.s0 + sb, A.seed)); P.depth = 0;
    const float dd = dotf(b.x, b.y, b.z, b.x, b.y, b.z);
    const bool finite = __builtin_isfinite(a.x) & __builtin_isfinite(a.y) & __builtin_isfinite(a.z) &
                        __builtin_isfinite(b.x) & __builtin_isfinite(b.y) & __builtin_isfinite(b.z);
    const bool ok = finite && __builtin_fabsf(dd - 1.0f) <= 0x1p-20f && a.w == __builtin_inff();       // (a NaN t_max fails the last test)
    if (!ok) { const float nan = __builtin_nanf(""); A.rad[item] = Rgb{ nan, nan, nan }; }
    return ok;
}

// HAS_TRI / HAS_SPH compile the face loop / sphere loop (and the matching shading) in or out, so that a sphere-only
// scene does not pay registers or code for the triangle path.
// Refill: lanes whose path ended take the next samples of the wave's chunk (ballot + prefix count); a chunk of
// kWorkChunk samples is fetched from the global queue with one atomic when the wave runs dry.
// Form::Query: the items are the caller's rays (query_ray); an invalid one leaves its lane empty (refill_queries fills it again).  Form::Rays: the same
// with rays_path.
template <Form F>
__device__ __forceinline__ void refill_lanes(const TraceArgs& A, uint32_t lane, bool& alive, Path& P, uint32_t& chunk_next,
                                             uint32_t& chunk_end, bool& exhausted) {
    const unsigned long long need = __ballot(!alive);
    if (need != 0ull && !exhausted) {
        const uint32_t n_need = (uint32_t)__popcll(need);
        const uint32_t rank = prefix_count(need);
        uint32_t item = 0xFFFFFFFFu, taken = 0;
        while (taken < n_need) {
            if (chunk_next == chunk_end) {
                uint32_t b = 0;
                if (lane == 0) b = atomicAdd(A.work_counter, kWorkChunk);
                b = __builtin_amdgcn_readfirstlane(b);
                if (b >= A.total) { exhausted = true; break; }
                chunk_next = b;
                chunk_end = min(b + kWorkChunk, A.total);
            }
            const uint32_t k = min(n_need - taken, chunk_end - chunk_next);
            if (!alive && rank >= taken && rank < taken + k) item = chunk_next + (rank - taken);
            chunk_next += k;
            taken += k;
        }
        if (item != 0xFFFFFFFFu) {
            if constexpr (F == Form::Query) alive = query_ray(A, item, P);
            else if constexpr (F == Form::Rays) alive = rays_path(A, item, P);
            else { start_path<F>(A, item, P); alive = true; }
        }
    }
}
// The query forms' refill: until every lane holds a valid ray or the queue is dry, so that invalid rays neither end a wave early (a wave leaves
// when no lane is alive after a refill) nor leave holes in it.  The rays forms' refill is the same loop around rays_path.
template <Form F>
__device__ __forceinline__ void refill_queries(const TraceArgs& A, uint32_t lane, bool& alive, Path& P, uint32_t& chunk_next, uint32_t& chunk_end,
                                               bool& exhausted) {
    static_assert(F == Form::Query || F == Form::Rays, "refill_queries: the forms whose items are the caller's rays");
    do refill_lanes<F>(A, lane, alive, P, chunk_next, chunk_end, exhausted);
    while (__ballot(!alive) != 0ull && !exhausted);
}
// The refill of every kernel without a ray stock: the one its form takes.
template <Form F>
__device__ __forceinline__ void refill(const TraceArgs& A, uint32_t lane, bool& alive, Path& P, uint32_t& chunk_next, uint32_t& chunk_end, bool& exhausted) {
    if constexpr (F == Form::Query || F == Form::Rays) refill_queries<F>(A, lane, alive, P, chunk_next, chunk_end, exhausted);
    else refill_lanes<F>(A, lane, alive, P, chunk_next, chunk_end, exhausted);
}

// Refill through a wave-wide stock of primary rays: start_path() runs for all 64 lanes at once (lane k of the stock holds sample
// chunk_next + k) and lanes whose path ended pop entries off the top with ds_bpermute — the ~250 instructions of start_path are
// then paid per 64 new paths instead of per loop iteration (in which about a third of the lanes end).
struct RayStock { float ox, oy, oz, dx, dy, dz; uint32_t slot, base; uint32_t n; };   // n: wave-uniform count, entries in lanes [0, n)
__device__ __forceinline__ void stock_pop(const RayStock& Q, uint32_t src, bool take, Path& P, bool& alive) {
    const int s = (int)src;
    const float ox = __shfl(Q.ox, s), oy = __shfl(Q.oy, s), oz = __shfl(Q.oz, s), dx = __shfl(Q.dx, s), dy = __shfl(Q.dy, s), dz = __shfl(Q.dz, s);
    const uint32_t slot = (uint32_t)__shfl((int)Q.slot, s), base = (uint32_t)__shfl((int)Q.base, s);
    if (take) {
        P.ox = ox; P.oy = oy; P.oz = oz; P.dx = dx; P.dy = dy; P.dz = dz; P.slot = slot; P.base = base;
        P.tr = P.tg = P.tb = 1.0f; P.lr = P.lg = P.lb = 0.0f; P.depth = 0;
        alive = true;
    }
}
template <Form F>
__device__ __forceinline__ void refill_from_stock(const TraceArgs& A, uint32_t lane, bool& alive, Path& P, RayStock& Q, uint32_t& chunk_next,
                                                  uint32_t& chunk_end, bool& exhausted) {
    const unsigned long long need = __ballot(!alive);
    if (need == 0ull) return;
    const uint32_t n_need = (uint32_t)__popcll(need), rank = prefix_count(need);
    uint32_t served = 0;
    for (;;) {
        const uint32_t k = min(Q.n, n_need - served);
        if (k != 0) {
            const bool take = !alive && rank >= served && rank < served + k;
            stock_pop(Q, Q.n - 1u - (rank - served), take, P, alive);       // (the index only matters where take is set)
            Q.n -= k;
            served += k;
        }
        if (served == n_need || exhausted) return;
        // the stock is empty: restock from the wave's chunk (one atomic per kWorkChunk samples)
        if (chunk_next == chunk_end) {
            uint32_t b = 0;
            if (lane == 0) b = atomicAdd(A.work_counter, kWorkChunk);
            b = __builtin_amdgcn_readfirstlane(b);
            if (b >= A.total) { exhausted = true; return; }
            chunk_next = b;
            chunk_end = min(b + kWorkChunk, A.total);
        }
        const uint32_t n_new = min(64u, chunk_end - chunk_next);
        Path T;
        start_path<F>(A, min(chunk_next + lane, chunk_end - 1u), T);
        Q.ox = T.ox; Q.oy = T.oy; Q.oz = T.oz; Q.dx = T.dx; Q.dy = T.dy; Q.dz = T.dz; Q.slot = T.slot; Q.base = T.base;
        Q.n = n_new;
        chunk_next += n_new;
    }
}

// The stock of k_trace_mfma32's render form (refill_from_traced_stock, rt3_matrix_filter.hpp): its entries are paths whose primary ray may already have
// been traced and shaded when the stock was filled, so an entry carries throughput and depth too (an untraced one: throughput 1, depth 0).
struct TracedStock { float ox, oy, oz, dx, dy, dz, tr, tg, tb; uint32_t slot, base, depth; uint32_t n; };   // n: wave-uniform count, entries in lanes [0, n)
__device__ __forceinline__ void stock_pop(const TracedStock& Q, uint32_t src, bool take, Path& P, bool& alive) {
    const int s = (int)src;
    const float ox = __shfl(Q.ox, s), oy = __shfl(Q.oy, s), oz = __shfl(Q.oz, s), dx = __shfl(Q.dx, s), dy = __shfl(Q.dy, s), dz = __shfl(Q.dz, s);
    const float tr = __shfl(Q.tr, s), tg = __shfl(Q.tg, s), tb = __shfl(Q.tb, s);
    const uint32_t slot = (uint32_t)__shfl((int)Q.slot, s), base = (uint32_t)__shfl((int)Q.base, s), depth = (uint32_t)__shfl((int)Q.depth, s);
    if (take) {
        P.ox = ox; P.oy = oy; P.oz = oz; P.dx = dx; P.dy = dy; P.dz = dz; P.slot = slot; P.base = base;
        P.tr = tr; P.tg = tg; P.tb = tb; P.lr = P.lg = P.lb = 0.0f; P.depth = depth;        // (a path that goes on has gathered no light yet: shade_lane)
        alive = true;
    }
}

// Shade / scatter one ray cast of every live lane (book materials).  kind: 0 miss, 1 face, 2 sphere.
// The four per-sphere arrays read at a hit are parameters: global memory in k_trace, LDS copies in k_trace_mfma.
// Form::RenderRef (RT3_FLAG_REFERENCE_PRIMARY): at ray cast 0 the direction is the reference's unnormalised one — the sky and the hit point use
// it as it is (SequentialRenderer.cpp:77,105-107); the scatter formulas then get the unit direction.
// CTR: ctr_tab is the counter-hash table (rt3_kernel_common.hpp, kCtrDepthCap rows in LDS): the inner hash of rnd(base, ctr + k) depends on the
// depth alone, so a lane below the cap reads its row instead of computing three hashes; at or beyond the cap it computes them as rnd() does.
// Environment forms (is_env(F); A is then an EnvTraceArgs): a miss adds throughput x env_lookup(direction) where the twin adds throughput x sky — the one
// difference between an environment form and its twin.
// Texture forms (is_tex(F); A is then a TexTraceArgs): where the material has just been fetched, its rgb is multiplied by the texel of the
// texture the hit primitive is bound to (tex_modulate) — the one difference between a texture form and its twin; a miss reads the map if one is set.
// Sampling forms (is_nee(F), RT3_FLAG_ENV_SAMPLING; A is a NeeTraceArgs, P a NeePath): a Lambert scatter also draws a direction w from the
// map's table (rt3env::sample, counters 3..6 of the scatter's block).  With c = n.w > 0 the shadow ray (p, w) takes the lane's next cast — the
// continuation waits in the NeePath — and THAT cast's shade_lane is the first block below: a miss adds T' (c / (pi pdf)) env(w), a hit adds nothing, and
// the lane goes on with the continuation.  The scatter itself draws what it always drew, so the continuation rays are the plain render's.  A miss
// behind such a scatter adds nothing: the shadow ray has accounted for the map.
template <bool HAS_TRI, bool HAS_SPH, Form F, bool CTR = false>
__device__ __forceinline__ void shade_lane(const TraceArgs& A, Path& P, bool& alive, uint32_t kind, uint32_t ibest, float tbest,
                                           const float4* sph, const float* sph_invr, const float4* sph_mat, const uint32_t* sph_kind,
                                           const uint4* ctr_tab = nullptr) {
    constexpr bool REF = F == Form::RenderRef;
    const float ox = P.ox, oy = P.oy, oz = P.oz;
    float dx = P.dx, dy = P.dy, dz = P.dz;
    if constexpr (is_nee(F)) {
        NeePath& N = nee_path(P);
        if (alive && (N.nee & kNeeShadow)) {                            // this cast was the shadow ray of the lane's last Lambert scatter
            if (kind == 0) {
                float r, g, b;
                env_lookup(env_of(A).env, env_of(A).env_n, dx, dy, dz, r, g, b);
                P.lr = fma_(N.er, r, P.lr); P.lg = fma_(N.eg, g, P.lg); P.lb = fma_(N.eb, b, P.lb);
            }
            P.dx = N.cx; P.dy = N.cy; P.dz = N.cz;                      // on with the continuation (origin, throughput and depth are already its)
            N.nee = kNeeLambert;
            return;
        }
    }
    if constexpr (is_light(F)) {
        LightPath& N = light_path(P);
        if (alive && (N.nee & kNeeShadow)) {                            // this cast was the shadow ray of the lane's last Lambert scatter
            const bool face_hit = HAS_TRI && (!HAS_SPH || kind == 1);
            const uint32_t entry = face_hit ? ibest : A.n_tri + ibest;  // the table's order: faces first, then spheres, each by rt3_hit.index
            if (kind != 0 && entry == N.light) {                        // the nearest hit IS the chosen light: nothing hides it
                const float4 m = face_hit ? A.tri_mat[ibest] : sph_mat[ibest];
                P.lr = fma_(N.er, m.x, P.lr); P.lg = fma_(N.eg, m.y, P.lg); P.lb = fma_(N.eb, m.z, P.lb);
            }
            P.dx = N.cx; P.dy = N.cy; P.dz = N.cz;                      // on with the continuation (origin, throughput and depth are already its)
            N.nee = kNeeLambert;
            return;
        }
    }
    if (alive) {
        bool done = false;
        if (kind == 0) {
            if constexpr (is_light(F)) {                                // the plain render's miss: black, the map's plain lookup, or the sky
                if (!(A.flags & RT3_FLAG_BLACK_BACKGROUND)) {
                    float r, g, b;
                    if (env_of(A).env_n != 0u) env_lookup(env_of(A).env, env_of(A).env_n, dx, dy, dz, r, g, b);
                    else sky(dx, dy, dz, r, g, b);
                    P.lr = fma_(P.tr, r, P.lr); P.lg = fma_(P.tg, g, P.lg); P.lb = fma_(P.tb, b, P.lb);
                }
            } else if constexpr (is_nee(F)) {                                 // (RT3_FLAG_BLACK_BACKGROUND is refused with the flag)
                if (!(nee_path(P).nee & kNeeLambert)) {
                    float r, g, b;
                    env_lookup(env_of(A).env, env_of(A).env_n, dx, dy, dz, r, g, b);
                    P.lr = fma_(P.tr, r, P.lr); P.lg = fma_(P.tg, g, P.lg); P.lb = fma_(P.tb, b, P.lb);
                }
            } else if (!(A.flags & RT3_FLAG_BLACK_BACKGROUND)) {
                float r, g, b;
                if constexpr (is_tex(F)) {                          // with or without a map, as the light forms
                    if (env_of(A).env_n != 0u) env_lookup(env_of(A).env, env_of(A).env_n, dx, dy, dz, r, g, b);
                    else sky(dx, dy, dz, r, g, b);
                }
                else if constexpr (is_env(F)) env_lookup(env_of(A).env, env_of(A).env_n, dx, dy, dz, r, g, b);
                else sky(dx, dy, dz, r, g, b);
                P.lr = fma_(P.tr, r, P.lr); P.lg = fma_(P.tg, g, P.lg); P.lb = fma_(P.tb, b, P.lb);
            }
            done = true;
        } else {
            float4 m; uint32_t mk;
            float px, py, pz, nx, ny, nz;
            if (HAS_TRI && (!HAS_SPH || kind == 1)) {
                m = A.tri_mat[ibest]; mk = A.tri_kind[ibest];
                const float4 n = A.tri[(size_t)ibest * 4];
                px = ox + tbest * dx; py = oy + tbest * dy; pz = oz + tbest * dz;
                nx = n.x; ny = n.y; nz = n.z;
            } else {
                m = sph_mat[ibest]; mk = sph_kind[ibest];
                const float4 s = sph[ibest];
                const float invr = sph_invr[ibest];
                px = fma_(tbest, dx, ox); py = fma_(tbest, dy, oy); pz = fma_(tbest, dz, oz);
                nx = (px - s.x) * invr; ny = (py - s.y) * invr; nz = (pz - s.z) * invr;
            }
            if constexpr (is_tex(F))                                // the one difference from the twin: rgb x the bound texture's texel
                tex_modulate(tex_of(A).tex, HAS_TRI && (!HAS_SPH || kind == 1), ibest, A.tri, px, py, pz, nx, ny, nz, mk, m);
            if (mk == RT3_MAT_FLAT) {
                bool adds = true;
                if constexpr (is_light(F)) {                            // behind a Lambert scatter the shadow ray has accounted for every light of the table
                    if (light_path(P).nee & kNeeLambert)
                        adds = light_of(A).lt_q[HAS_TRI && (!HAS_SPH || kind == 1) ? ibest : A.n_tri + ibest] == 0u;
                }
                if (adds) { P.lr = fma_(P.tr, m.x, P.lr); P.lg = fma_(P.tg, m.y, P.lg); P.lb = fma_(P.tb, m.z, P.lb); }
                done = true;
            } else if (P.depth + 1 == A.max_depth) {
                done = true;
            } else {
                if (REF && P.depth == 0) {
                    const float inv = 1.0f / __builtin_sqrtf(dot3(dx, dy, dz, dx, dy, dz));
                    dx = dx * inv; dy = dy * inv; dz = dz * inv;
                }
                const bool front = dotf(dx, dy, dz, nx, ny, nz) < 0.0f;
                if (!front) { nx = -nx; ny = -ny; nz = -nz; }           // (the dot product is recomputed with the flipped normal below:
                const uint32_t ctr = 1u + 8u * (P.depth + 1u);
                uint32_t h0 = 0, h1 = 0, h2 = 0;                // CTR: hash_u32(ctr + k)
                if constexpr (CTR) {
                    if (P.depth < kCtrDepthCap) { const uint4 row = ctr_tab[P.depth]; h0 = row.x; h1 = row.y; h2 = row.z; }
                    else { h0 = hash_u32(ctr); h1 = hash_u32(ctr + 1u); h2 = hash_u32(ctr + 2u); }
                }
                auto xi = [&](uint32_t k, uint32_t h) { return CTR ? u01(hash_u32(P.base ^ h)) : rnd(P.base, ctr + k); };
                float sx, sy, sz;                               // scattered direction before normalisation
                float ar = m.x, ag = m.y, ab = m.z;
                // work shared between material branches is done once for all lanes that need it: the random unit vector
                // (Lambert, fuzzy metal) and the mirror direction (metal, dielectric) — the wave executes every branch
                // that any lane takes, so merging them shortens the serialised shading
                const float dn = dotf(dx, dy, dz, nx, ny, nz);
                float vx = 0.0f, vy = 0.0f, vz = 0.0f;
                if ((mk == RT3_MAT_LAMBERT) | ((mk == RT3_MAT_METAL) & (m.w > 0.0f)))
                    unit_vector(xi(0, h0), xi(1, h1), vx, vy, vz);
                const float k2 = 2.0f * dn;
                const float mx = fma_(-k2, nx, dx), my = fma_(-k2, ny, dy), mz = fma_(-k2, nz, dz);   // reflect(d, n)
                if (mk == RT3_MAT_LAMBERT) {
                    sx = nx + vx; sy = ny + vy; sz = nz + vz;
                    if (__builtin_fabsf(sx) < 1e-8f && __builtin_fabsf(sy) < 1e-8f && __builtin_fabsf(sz) < 1e-8f) { sx = nx; sy = ny; sz = nz; }
                } else if (mk == RT3_MAT_METAL) {
                    const float inv = 1.0f / __builtin_sqrtf(dotf(mx, my, mz, mx, my, mz));
                    const float rx = mx * inv, ry = my * inv, rz = mz * inv;
                    sx = rx; sy = ry; sz = rz;
                    if (m.w > 0.0f) { sx = fma_(m.w, vx, rx); sy = fma_(m.w, vy, ry); sz = fma_(m.w, vz, rz); }
                    if (!(dotf(sx, sy, sz, nx, ny, nz) > 0.0f)) done = true;       // absorbed
                } else {                                        // dielectric: m = (1/ior, r0(1/ior), r0(ior), ior), see rt3_set_spheres
                    const float ri = front ? m.x : m.w;
                    float cosv = -dn;
                    if (cosv > 1.0f) cosv = 1.0f;
                    const float s2 = fma_(-cosv, cosv, 1.0f);
                    const float sinv = __builtin_sqrtf(s2 > 0.0f ? s2 : 0.0f);
                    const bool cannot = ri * sinv > 1.0f;
                    const float r0 = front ? m.y : m.z;
                    const float xx = 1.0f - cosv, x2 = xx * xx, x5 = x2 * x2 * xx;
                    const float R = fma_(1.0f - r0, x5, r0);
                    if (cannot || R > xi(2, h2)) {
                        sx = mx; sy = my; sz = mz;
                    } else {
                        const float ex = fma_(cosv, nx, dx) * ri, ey = fma_(cosv, ny, dy) * ri, ez = fma_(cosv, nz, dz) * ri;
                        const float par = -__builtin_sqrtf(__builtin_fabsf(1.0f - dotf(ex, ey, ez, ex, ey, ez)));
                        sx = fma_(par, nx, ex); sy = fma_(par, ny, ey); sz = fma_(par, nz, ez);
                    }
                    ar = ag = ab = 1.0f;
                }
                if (!done) {
                    const float inv = 1.0f / __builtin_sqrtf(dotf(sx, sy, sz, sx, sy, sz));
                    P.dx = sx * inv; P.dy = sy * inv; P.dz = sz * inv;
                    P.ox = px; P.oy = py; P.oz = pz;
                    P.tr *= ar; P.tg *= ag; P.tb *= ab;
                    P.depth += 1;
                    if constexpr (is_light(F)) {
                        LightPath& N = light_path(P);
                        N.nee = mk == RT3_MAT_LAMBERT ? kNeeLambert : 0u;
                        if (mk == RT3_MAT_LAMBERT) {
                            const LightTraceArgs& E = light_of(A);
                            const uint64_t total = E.lt_cdf[E.lt_n - 1u];
                            if (total != 0ull) {
                                float ua, ub;
                                const uint32_t li = rt3light::pick(E.lt_cdf, E.lt_n, total, P.base, P.depth - 1u, ua, ub);
                                const bool is_sph = !HAS_TRI || (HAS_SPH && li >= A.n_tri);
                                rt3light::Point Y;
                                float4 cr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                                if (is_sph) {
                                    cr = E.lt_sph_cr[li - A.n_tri];
                                    rt3light::point_on_sphere(cr.x, cr.y, cr.z, cr.w, ua, ub, Y);
                                } else {
                                    const float4 a = A.tri[(size_t)li * 4 + 1], b = A.tri[(size_t)li * 4 + 2], c = A.tri[(size_t)li * 4 + 3];
                                    const float p1[3] = { a.x, a.y, a.z }, p2[3] = { b.x, b.y, b.z }, p3[3] = { c.x, c.y, c.z };
                                    rt3light::Face f;
                                    rt3light::face_of(p1, p2, p3, f);
                                    rt3light::point_on_face(f, ua, ub, Y);
                                }
                                float wx, wy, wz, k;
                                if (rt3light::connect(Y, is_sph, cr.x, cr.y, cr.z, cr.w, px, py, pz, nx, ny, nz, E.lt_q[li], total, wx, wy, wz, k)) {
                                    N.er = P.tr * k; N.eg = P.tg * k; N.eb = P.tb * k;
                                    N.cx = P.dx; N.cy = P.dy; N.cz = P.dz;
                                    P.dx = wx; P.dy = wy; P.dz = wz;
                                    N.light = li;
                                    N.nee = kNeeLambert | kNeeShadow;
                                }
                            }
                        }
                    }
                    if constexpr (is_nee(F)) {
                        NeePath& N = nee_path(P);
                        N.nee = mk == RT3_MAT_LAMBERT ? kNeeLambert : 0u;
                        if (mk == RT3_MAT_LAMBERT) {
                            const NeeTraceArgs& E = nee_of(A);
                            const uint64_t total = E.nee_cdf[E.nee_cells - 1u];
                            if (total != 0ull) {
                                rt3env::Sample S;
                                rt3env::sample(E.nee_q, E.nee_cdf, E.nee_m, total, P.base, P.depth - 1u, S);
                                const float c = dotf(nx, ny, nz, S.dx, S.dy, S.dz);
                                if (c > 0.0f) {
                                    const float k = c / (3.14159274f * S.pdf);
                                    N.er = P.tr * k; N.eg = P.tg * k; N.eb = P.tb * k;
                                    N.cx = P.dx; N.cy = P.dy; N.cz = P.dz;
                                    P.dx = S.dx; P.dy = S.dy; P.dz = S.dz;
                                    N.nee = kNeeLambert | kNeeShadow;
                                }
                            }
                        }
                    }
                }
            }
        }
        if (done) {
            A.rad[P.slot] = Rgb{ P.lr, P.lg, P.lb };
            alive = false;
            if constexpr (has_shadow(F)) nee_path(P).nee = 0u;              // the lane's next path starts without a scatter behind it
        }
    }
}

}  // namespace
