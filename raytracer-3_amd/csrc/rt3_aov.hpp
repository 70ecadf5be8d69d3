// rt3_aov.hpp — first-hit AOVs (rt3_render_aov*), Mode X's camera rays as rt3_ray records (rt3_camera_rays*) and the
// linear float resolve of the accumulation (rt3_accum_resolve*), and the specular-chain AOVs (rt3_render_aov_specular*).  None of these kernels traces: the AOV pass runs k_camera_rays, then the
// query form of the trace kernel Mode X would take (plan_trace with Form::Query) on that buffer, then k_aov_accumulate.
// Part of rt3_device.hip (one translation unit, gfx950 only); included from there, in this order.
#pragma once

namespace {

// Item k of the batch (sample s0 + k / npix, owned pixel k % npix) -> its primary ray, bit for bit the ray Mode X casts first
// (start_path<Form::Render>): rays[2 k] = (origin, +inf), rays[2 k + 1] = (unit direction, 0).  Two 16-byte stores per ray.
__global__ __launch_bounds__(kBlock) void k_camera_rays(const TraceArgs A, float4* __restrict__ rays) {
    const uint32_t item = blockIdx.x * kBlock + threadIdx.x;
    if (item >= A.total) return;
    Path P;
    start_path<Form::Render>(A, item, P);
    float4* r = rays + 2 * (size_t)item;
    r[0] = make_float4(P.ox, P.oy, P.oz, __builtin_inff());
    r[1] = make_float4(P.dx, P.dy, P.dz, 0.0f);
}

// Running sums of one pixel's AOVs, three planes of npix float4 each:
//   acc[pix]            albedo sum (rgb), sum of t over the samples that hit
//   acc[npix + pix]     normal sum (xyz), 0
//   acc[2 npix + pix]   as uint4: kind and index of sample 0's hit, samples that hit, 0
// One thread per pixel; the samples of the batch are added in sample order, as k_accumulate adds radiance.  `first`: the batch
// starts at sample 0 (the sums start from zero and sample 0's hit is recorded).  Material and sphere records are read in the caller's primitive
// order — the order of a hit's index — through the fields scene_args() fills in; hit point and normal are computed as shade_lane() does.
// env_n != 0: an environment map is set and a miss's albedo is its lookup, where it is the sky otherwise — a run-time test, this is no
// trace kernel.  X.slots != null: the context is textured and a hit's albedo is rgb x the bound texel (tex_modulate), again at run time.
// The lookup's registers would take the kernel from 8 waves per SIMD to 6 (78 VGPRs); bounded to 7 it keeps 72 and no scratch, bounded to 8 it spills.
__global__ __launch_bounds__(kBlock, 7) void k_aov_accumulate(const TraceArgs A, const float4* __restrict__ rays, const uint4* __restrict__ hits,
                                                          float4* __restrict__ acc, uint32_t npix, uint32_t ns, int first,
                                                          const float4* __restrict__ env, uint32_t env_n, const TexTable X) {
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 a = first ? zero : acc[pix];
    float4 n = first ? zero : acc[(size_t)npix + pix];
    uint4* const acc_u = reinterpret_cast<uint4*>(acc) + 2 * (size_t)npix + pix;
    uint4 k = first ? make_uint4(0u, 0u, 0u, 0u) : *acc_u;
    for (uint32_t s = 0; s < ns; s++) {
        const size_t item = (size_t)s * npix + pix;
        const uint4 h = hits[item];
        const float4 ro = rays[2 * item], rd = rays[2 * item + 1];
        const uint32_t kind = h.y, idx = h.z;
        const float t = __uint_as_float(h.x);
        float ar = 0.0f, ag = 0.0f, ab = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (kind == RT3_HIT_NONE) {
            if (!(A.flags & RT3_FLAG_BLACK_BACKGROUND)) {
                if (env_n != 0u) env_lookup(env, env_n, rd.x, rd.y, rd.z, ar, ag, ab);
                else sky(rd.x, rd.y, rd.z, ar, ag, ab);
            }
        } else if (kind == RT3_HIT_FACE || kind == RT3_HIT_SPHERE) {
            float4 m; uint32_t mk;
            float px, py, pz;
            if (kind == RT3_HIT_FACE) {
                m = A.tri_mat[idx]; mk = A.tri_kind[idx];
                const float4 fn = A.tri[(size_t)idx * 4];
                px = ro.x + t * rd.x; py = ro.y + t * rd.y; pz = ro.z + t * rd.z;
                nx = fn.x; ny = fn.y; nz = fn.z;
            } else {
                m = A.sph_mat[idx]; mk = A.sph_kind[idx];
                const float4 c = A.sph[idx];
                const float invr = A.sph_invr[idx];
                px = fma_(t, rd.x, ro.x); py = fma_(t, rd.y, ro.y); pz = fma_(t, rd.z, ro.z);
                nx = (px - c.x) * invr; ny = (py - c.y) * invr; nz = (pz - c.z) * invr;
            }
            if (X.slots != nullptr) tex_modulate(X, kind == RT3_HIT_FACE, idx, A.tri, px, py, pz, nx, ny, nz, mk, m);     // textured: the modulated albedo
            if (!(dotf(rd.x, rd.y, rd.z, nx, ny, nz) < 0.0f)) { nx = -nx; ny = -ny; nz = -nz; }
            // a dielectric's device record holds (1/ior, r0, r0', ior), not a colour: its albedo is its attenuation, 1
            if (mk == RT3_MAT_DIELECTRIC) { ar = ag = ab = 1.0f; }
            else { ar = m.x; ag = m.y; ab = m.z; }
            a.w = a.w + t;
            k.z += 1u;
        }                                                           // (RT3_HIT_INVALID: a miss with albedo 0)
        a.x = a.x + ar; a.y = a.y + ag; a.z = a.z + ab;
        n.x = n.x + nx; n.y = n.y + ny; n.z = n.z + nz;
        if (first && s == 0) { k.x = kind; k.y = idx; }
    }
    acc[pix] = a;
    acc[(size_t)npix + pix] = n;
    *acc_u = k;
}

// The sums -> rt3_aov records (48 bytes: three 16-byte stores), spp samples per pixel.
__global__ __launch_bounds__(kBlock) void k_aov_resolve(const float4* __restrict__ acc, uint32_t npix, uint32_t spp, float4* __restrict__ out) {
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float4 a = acc[pix], n = acc[(size_t)npix + pix];
    const uint4 k = reinterpret_cast<const uint4*>(acc)[2 * (size_t)npix + pix];
    const float fs = (float)spp;
    const uint32_t n_hit = k.z;
    const float depth = n_hit ? a.w / (float)n_hit : __builtin_inff();
    float4* o = out + 3 * (size_t)pix;
    o[0] = make_float4(a.x / fs, a.y / fs, a.z / fs, (float)n_hit / fs);
    o[1] = make_float4(n.x / fs, n.y / fs, n.z / fs, depth);
    reinterpret_cast<uint4*>(o)[2] = make_uint4(k.x, k.y, 0u, 0u);
}

// ---- Specular-chain AOVs (rt3_render_aov_specular*).  Per item of a batch, beside its ray and the hit of the query just run:
//   state[item]   running: (T, L), the chain's throughput and length; finished: (albedo, L) of its end
//   endn[item]    (normal of the last surface the chain hit, 0)
// A finished item's ray keeps its origin and direction and gets t_max = NaN: the query engine calls such a ray INVALID, does not trace it and does not
// count it.  The engine still stores RT3_HIT_INVALID for it, so the bounce queries write to a buffer of their own and the primary hits — what kind /
// index and the coverage are taken from — stay where the first query put them.
// k_aov_bounce: one thread per item, after query number b (b bounces used).  Hit point, normal, material and texture are k_aov_accumulate's, operation
// for operation; the decision and the next direction are rt3chain::step's.  16-byte loads and stores throughout: the ray's two halves, the hit, the
// state.  COUNT: the items that go on are counted into *alive (one atomic per wave), for the host's early exit.  A streaming kernel:
// bounded to 7 waves per SIMD as k_aov_accumulate is (the same texture lookup is live here), it takes 66 VGPRs and no scratch.
template <bool COUNT>
__global__ __launch_bounds__(kBlock, 7) void k_aov_bounce(const TraceArgs A, float4* __restrict__ rays, const uint4* __restrict__ hits,
                                                      float4* __restrict__ state, float4* __restrict__ endn, uint32_t b, uint32_t max_bounces,
                                                      float max_fuzz, const float4* __restrict__ env, uint32_t env_n, const TexTable X,
                                                      uint32_t* __restrict__ alive) {
    const uint32_t item = blockIdx.x * kBlock + threadIdx.x;
    bool follow = false;
    if (item < A.total) {
        float4* const r = rays + 2 * (size_t)item;
        const float4 ro = r[0];
        if (ro.w == ro.w) {                                         // (NaN: the chain ended at an earlier bounce)
            const float4 rd = r[1];
            const uint4 h = hits[item];
            const float4 st = b ? state[item] : make_float4(1.0f, 1.0f, 1.0f, 0.0f);
            const uint32_t kind = h.y, idx = h.z;
            const float t = __uint_as_float(h.x);
            float4 out = make_float4(0.0f, 0.0f, 0.0f, st.w);       // (RT3_HIT_INVALID, a primary ray only: a miss with albedo 0)
            bool new_normal = b == 0;                               // a miss behind a surface keeps that surface's normal
            float nx = 0.0f, ny = 0.0f, nz = 0.0f;
            float4 next_o = ro, next_d = rd;
            if (kind == RT3_HIT_NONE) {
                float cr = 0.0f, cg = 0.0f, cb = 0.0f;
                if (!(A.flags & RT3_FLAG_BLACK_BACKGROUND)) {
                    if (env_n != 0u) env_lookup(env, env_n, rd.x, rd.y, rd.z, cr, cg, cb);
                    else sky(rd.x, rd.y, rd.z, cr, cg, cb);
                }
                out.x = st.x * cr; out.y = st.y * cg; out.z = st.z * cb;
            } else if (kind == RT3_HIT_FACE || kind == RT3_HIT_SPHERE) {
                float4 m; uint32_t mk;
                float px, py, pz;
                if (kind == RT3_HIT_FACE) {
                    m = A.tri_mat[idx]; mk = A.tri_kind[idx];
                    const float4 fn = A.tri[(size_t)idx * 4];
                    px = ro.x + t * rd.x; py = ro.y + t * rd.y; pz = ro.z + t * rd.z;
                    nx = fn.x; ny = fn.y; nz = fn.z;
                } else {
                    m = A.sph_mat[idx]; mk = A.sph_kind[idx];
                    const float4 c = A.sph[idx];
                    const float invr = A.sph_invr[idx];
                    px = fma_(t, rd.x, ro.x); py = fma_(t, rd.y, ro.y); pz = fma_(t, rd.z, ro.z);
                    nx = (px - c.x) * invr; ny = (py - c.y) * invr; nz = (pz - c.z) * invr;
                }
                if (X.slots != nullptr) tex_modulate(X, kind == RT3_HIT_FACE, idx, A.tri, px, py, pz, nx, ny, nz, mk, m);
                const rt3chain::Step S = rt3chain::step(rd.x, rd.y, rd.z, px, py, pz, nx, ny, nz, mk, m.x, m.y, m.z, m.w, st.x, st.y, st.z, b,
                                                        max_bounces, max_fuzz);
                out = make_float4(S.ax, S.ay, S.az, st.w + t);
                nx = S.nx; ny = S.ny; nz = S.nz;
                new_normal = true;
                follow = S.follow != 0u;
                next_o = make_float4(px, py, pz, __builtin_inff());
                next_d = make_float4(S.dx, S.dy, S.dz, 0.0f);
            }
            state[item] = out;
            if (new_normal) endn[item] = make_float4(nx, ny, nz, 0.0f);
            if (follow) { r[0] = next_o; r[1] = next_d; }
            else r[0] = make_float4(ro.x, ro.y, ro.z, __builtin_nanf(""));
        }
    }
    if constexpr (COUNT) {
        const unsigned long long going = __ballot(follow);
        if (going != 0ull && lane_id() == 0u) atomicAdd(alive, (uint32_t)__popcll(going));
    }
}

// k_aov_accumulate for the chains' ends: the same three planes, the same order of additions.  hits: the PRIMARY hits (sample 0's names the pixel's
// object; L is summed and counted over the samples whose primary ray hit), state / endn: as k_aov_bounce left them, every chain finished.
__global__ __launch_bounds__(kBlock) void k_aov_accumulate_chain(const uint4* __restrict__ hits, const float4* __restrict__ state,
                                                                 const float4* __restrict__ endn, float4* __restrict__ acc, uint32_t npix, uint32_t ns,
                                                                 int first) {
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 a = first ? zero : acc[pix];
    float4 n = first ? zero : acc[(size_t)npix + pix];
    uint4* const acc_u = reinterpret_cast<uint4*>(acc) + 2 * (size_t)npix + pix;
    uint4 k = first ? make_uint4(0u, 0u, 0u, 0u) : *acc_u;
    for (uint32_t s = 0; s < ns; s++) {
        const size_t item = (size_t)s * npix + pix;
        const uint4 h = hits[item];
        const float4 e = state[item], en = endn[item];
        if (h.y == RT3_HIT_FACE || h.y == RT3_HIT_SPHERE) { a.w = a.w + e.w; k.z += 1u; }
        a.x = a.x + e.x; a.y = a.y + e.y; a.z = a.z + e.z;
        n.x = n.x + en.x; n.y = n.y + en.y; n.z = n.z + en.z;
        if (first && s == 0) { k.x = h.y; k.y = h.z; }
    }
    acc[pix] = a;
    acc[(size_t)npix + pix] = n;
    *acc_u = k;
}

// Linear resolve of the accumulation: (sum / n, 0) per owned pixel, n = samples accumulated — k_resolve's division, before any gamma.
__global__ __launch_bounds__(kBlock) void k_resolve_float(const float4* __restrict__ accum, uint32_t npix, uint32_t spp, float4* __restrict__ out) {
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float4 a = accum[pix];
    const float n = (float)spp;
    out[pix] = make_float4(a.x / n, a.y / n, a.z / n, 0.0f);
}
// The same division in place (rt3_radiance*: the caller's output is the sum buffer of its batches; k_resolve_float's __restrict__ forbids the aliasing).
__global__ __launch_bounds__(kBlock) void k_resolve_float_inplace(float4* sums, uint32_t n_items, uint32_t spp) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_items) return;
    const float4 a = sums[i];
    const float n = (float)spp;
    sums[i] = make_float4(a.x / n, a.y / n, a.z / n, 0.0f);
}

}  // namespace
