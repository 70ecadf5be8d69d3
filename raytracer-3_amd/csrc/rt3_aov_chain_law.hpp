// rt3_aov_chain_law.hpp — the specular-chain law (rt3.h "Specular-chain AOVs"): what one hit does to a chain that follows mirrors and
// glass to the first rough surface — end here, reflect, or refract — one statement for the device and the host.
// Included by rt3_device.hip (k_aov_bounce, rt3_aov.hpp) and by rt3_host.cpp (rt3_debug_aov_bounce: the serial restatement the tests compare with
// tests/aov_chain_ref.py).  Every float operation is an IEEE f32 operation rounded on its own (every file is compiled with -ffp-contract=off); each
// fused multiply-add is written out (fma).  The directions are shade_lane's (rt3_path.hpp): the mirror direction normalised twice, the refraction
// normalised once; the fuzz of a followed metal is ignored and Schlick's choice is not taken (the chain refracts whenever it can).
#pragma once
#include <cstdint>

#include "rt3.h"

#ifndef RT3_HD
#ifdef __HIP__
#define RT3_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RT3_HD inline
#endif
#endif

namespace rt3chain {

RT3_HD float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// Mode X's dot: z*z' + (y*y' + x*x') as two fused multiply-adds.
RT3_HD float dot(float ax, float ay, float az, float bx, float by, float bz) { return fma(az, bz, fma(ay, by, ax * bx)); }

// rt3_intersect's rule for a ray with t_max = +inf (t_min is finite, so the t_max test always passes).
RT3_HD bool ray_valid(float ox, float oy, float oz, float dx, float dy, float dz) {
    const bool finite = __builtin_isfinite(ox) & __builtin_isfinite(oy) & __builtin_isfinite(oz) &
                        __builtin_isfinite(dx) & __builtin_isfinite(dy) & __builtin_isfinite(dz);
    return finite && __builtin_fabsf(dot(dx, dy, dz, dx, dy, dz) - 1.0f) <= 0x1p-20f;
}

// Why the entry points refuse these chain params (each message names its argument), or nullptr.
inline const char* refusal(const rt3_aov_chain_params* c) {
    if (!c) return "chain is NULL";
    if (c->max_bounces > 16u) return "chain: max_bounces must be <= 16";
    if (!(c->max_fuzz >= 0.0f) || !(c->max_fuzz < __builtin_inff())) return "chain: max_fuzz must be finite and >= 0";
    if (c->flags != 0u) return "chain: flags must be 0";
    if (c->_pad != 0u) return "chain: _pad must be 0";
    return nullptr;
}

// What a hit leaves behind.  follow == 0: the chain ends at this surface, a* = T x the surface's colour.  follow == 1: the next ray leaves the hit point
// along d*, a* is the new throughput.  n*: the surface's normal, flipped to face the ray, either way.
struct Step { float ax, ay, az; float nx, ny, nz; float dx, dy, dz; uint32_t follow; };

// One hit of the chain.  d: the ray's unit direction; p: the hit point (the next origin); n: the surface's normal before the flip; mk, m: the
// material's kind and device record (metal: rgb, fuzz; dielectric: 1/ior, r0, r0', ior) after any texture; T: the throughput; b: bounces used so far.
RT3_HD Step step(float dx, float dy, float dz, float px, float py, float pz, float nx, float ny, float nz, uint32_t mk, float mx_, float my_, float mz_,
                 float mw_, float tr, float tg, float tb, uint32_t b, uint32_t max_bounces, float max_fuzz) {
    Step S;
    const bool front = dot(dx, dy, dz, nx, ny, nz) < 0.0f;
    if (!front) { nx = -nx; ny = -ny; nz = -nz; }
    S.nx = nx; S.ny = ny; S.nz = nz;
    S.dx = S.dy = S.dz = 0.0f;
    const bool glass = mk == RT3_MAT_DIELECTRIC;
    const float cr = glass ? 1.0f : mx_, cg = glass ? 1.0f : my_, cb = glass ? 1.0f : mz_;
    S.ax = tr * cr; S.ay = tg * cg; S.az = tb * cb;                 // the end's albedo, and a followed metal's new throughput
    S.follow = 0u;
    if (!(b < max_bounces) || !((mk == RT3_MAT_METAL && mw_ <= max_fuzz) || glass)) return S;
    const float dn = dot(dx, dy, dz, nx, ny, nz);
    const float k2 = 2.0f * dn;
    const float mx = fma(-k2, nx, dx), my = fma(-k2, ny, dy), mz = fma(-k2, nz, dz);       // reflect(d, n)
    float sx, sy, sz;
    if (!glass) {
        const float inv = 1.0f / __builtin_sqrtf(dot(mx, my, mz, mx, my, mz));
        sx = mx * inv; sy = my * inv; sz = mz * inv;
        if (!(dot(sx, sy, sz, nx, ny, nz) > 0.0f)) return S;        // the render's "absorbed"
    } else {
        const float ri = front ? mx_ : mw_;
        float cosv = -dn;
        if (cosv > 1.0f) cosv = 1.0f;
        const float s2 = fma(-cosv, cosv, 1.0f);
        const float sinv = __builtin_sqrtf(s2 > 0.0f ? s2 : 0.0f);
        const bool cannot = ri * sinv > 1.0f;
        if (cannot) {
            sx = mx; sy = my; sz = mz;
        } else {
            const float ex = fma(cosv, nx, dx) * ri, ey = fma(cosv, ny, dy) * ri, ez = fma(cosv, nz, dz) * ri;
            const float par = -__builtin_sqrtf(__builtin_fabsf(1.0f - dot(ex, ey, ez, ex, ey, ez)));
            sx = fma(par, nx, ex); sy = fma(par, ny, ey); sz = fma(par, nz, ez);
        }
    }
    const float inv = 1.0f / __builtin_sqrtf(dot(sx, sy, sz, sx, sy, sz));
    const float ox = sx * inv, oy = sy * inv, oz = sz * inv;
    if (!ray_valid(px, py, pz, ox, oy, oz)) return S;               // the query engine would not trace it: the chain ends at this surface
    S.dx = ox; S.dy = oy; S.dz = oz;
    S.follow = 1u;                                                  // (a dielectric: a* = T x 1 = T, unchanged)
    return S;
}

}  // namespace rt3chain
