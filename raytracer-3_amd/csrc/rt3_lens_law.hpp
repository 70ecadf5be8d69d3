// rt3_lens_law.hpp — the lens models' ray law (rt3.h "Lens models") and its inverse (rt3.h "Lens sequences"), one
// statement for the device and the host.
// Included by rt3_device.hip (k_lens_rays and the drivers' checks, rt3_lens.hpp), by rt3_denoise.hip (the lens forms of k_temporal_reproject and
// k_motion, their entry points' checks) and by rt3_host.cpp (rt3_debug_lens_ray, rt3_lens_look_at, rt3_debug_turns, rt3_debug_optic_pixel: the serial restatement the tests
// compare with tests/lens_ref.py and tests/optic_ref.py).  Every float operation is an IEEE f32 operation rounded on its own (every file is compiled with
// -ffp-contract=off); the fused multiply-adds of sincos2pi and of the validity rule's d.d are written out.  The hash, u01 and sincos2pi restate
// rt3_kernel_common.hpp's, which exist for the device only.
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

namespace rt3lens {

RT3_HD uint32_t hash_u32(uint32_t x) { x += x << 10; x ^= x >> 6; x += x << 3; x ^= x >> 11; x += x << 15; return x; }
RT3_HD uint32_t hash2(uint32_t a, uint32_t b) { return hash_u32(a ^ hash_u32(b)); }
RT3_HD float u01(uint32_t m) { const uint32_t b = (m & 0x007FFFFFu) | 0x3F800000u; float f; __builtin_memcpy(&f, &b, 4); return f - 1.0f; }
RT3_HD float rnd(uint32_t base, uint32_t ctr) { return u01(hash2(base, ctr)); }
RT3_HD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// Mode X's fused dot product (the ray validity rule's d.d) and the unfused one start_path_at normalises with.
RT3_HD float dotf(const float* a, const float* b) { return fma_(a[2], b[2], fma_(a[1], b[1], a[0] * b[0])); }
RT3_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }
RT3_HD bool finite(float x) { return x - x == 0.0f; }

// (cos, sin)(2 pi u): rt3_kernel_common.hpp's sincos2pi, operation for operation.
RT3_HD void sincos2pi(float u, float& c_out, float& s_out) {
    const float a = u * 4.0f;
    const int k = (int)a;
    const float f = a - (float)k;
    const float x = f * 1.57079637f;
    const float x2 = x * x;
    float p = fma_(x2, -2.50521084e-8f, 2.75573192e-6f);
    p = fma_(x2, p, -1.98412698e-4f);
    p = fma_(x2, p, 8.33333333e-3f);
    p = fma_(x2, p, -1.66666667e-1f);
    const float s = fma_(x * x2, p, x);
    float q = fma_(x2, 2.08767570e-9f, -2.75573192e-7f);
    q = fma_(x2, q, 2.48015873e-5f);
    q = fma_(x2, q, -1.38888889e-3f);
    q = fma_(x2, q, 4.16666667e-2f);
    q = fma_(x2, q, -0.5f);
    const float c = fma_(x2, q, 1.0f);
    const int kk = k & 3;
    c_out = kk == 0 ? c : kk == 1 ? -s : kk == 2 ? -c : s;
    s_out = kk == 0 ? s : kk == 1 ? c : kk == 2 ? -s : -c;
}

// The stratum edge of spp samples: e when spp = e * e > 1 (stratified), else 0 — what path_args() hands start_path_at.
inline uint32_t edge_of(uint32_t spp) {
    uint32_t e = 0;
    while ((uint64_t)(e + 1) * (e + 1) <= spp) e++;
    return (e * e == spp && spp > 1) ? e : 0;
}

// Which lens the entry points accept (rt3.h): nullptr, or what is wrong with it.  width / height: the frame's (RT3_LENS_CUBE needs H = 6 W).
inline const char* refusal(const rt3_lens* l, uint32_t width, uint32_t height) {
    if (l->model < RT3_LENS_EQUIRECT || l->model > RT3_LENS_CUBE) return "lens: unknown model";
    const float* ax[3] = { l->right, l->up, l->forward };
    for (int c = 0; c < 3; c++)
        if (!finite(l->origin[c]) || !finite(l->right[c]) || !finite(l->up[c]) || !finite(l->forward[c])) return "lens: origin and axes must be finite";
    for (int a = 0; a < 3; a++)
        if (!(__builtin_fabsf(dotf(ax[a], ax[a]) - 1.0f) <= 0x1p-20f)) return "lens: right, up and forward must be unit vectors (|d.d - 1| <= 2^-20)";
    for (int a = 0; a < 3; a++)
        if (!(__builtin_fabsf(dotf(ax[a], ax[(a + 1) % 3])) <= 0x1p-20f)) return "lens: right, up and forward must be orthogonal (|a.b| <= 2^-20)";
    if (l->model == RT3_LENS_FISHEYE && !(l->half_fov_turns > 0.0f && l->half_fov_turns <= 0.5f)) return "lens: half_fov_turns must lie in (0, 0.5]";
    if (l->model == RT3_LENS_ORTHO)
        for (int c = 0; c < 2; c++)
            if (!(l->half_extent[c] > 0.0f) || !finite(l->half_extent[c])) return "lens: half_extent must be finite and > 0";
    if (l->model == RT3_LENS_CUBE && (uint64_t)height != 6ull * width) return "lens: a cube frame has height == 6 * width";
    return nullptr;
}

// The frame of one call: what the law reads besides the lens.
struct Frame { uint32_t width, height, spp, seed, edge; };

// Sample s of frame pixel (x, y), row 0 on top -> origin o and unit direction d.  MODEL: the lens's model, a compile-time choice in the kernels.
template <uint32_t MODEL>
RT3_HD void ray(const rt3_lens& L, const Frame& F, uint32_t x, uint32_t y, uint32_t s, float o[3], float d[3]) {
    const uint32_t base = hash2(y * F.width + x, hash2(s, F.seed));
    float jx = 0.0f, jy = 0.0f;
    if (F.spp > 1) {                                                // start_path_at's jitter: counters 1 and 2, its strata
        const float xi0 = rnd(base, 1), xi1 = rnd(base, 2);
        if (F.edge != 0) {
            const uint32_t sy = s / F.edge, sx = s - sy * F.edge;
            jx = ((float)sx + xi0) / (float)F.edge - 0.5f;
            jy = ((float)sy + xi1) / (float)F.edge - 0.5f;
        } else { jx = xi0 - 0.5f; jy = xi1 - 0.5f; }
    }
    const float W = (float)F.width, H = (float)F.height;
    const float px = ((float)x + 0.5f) + jx;
    const float py = ((float)y + 0.5f) - jy;
    const float a = px / W;
    const float b = py / H;
    float lx, ly, lz;
    o[0] = L.origin[0]; o[1] = L.origin[1]; o[2] = L.origin[2];
    if (MODEL == RT3_LENS_EQUIRECT) {
        float ct, st, cp, sp;
        sincos2pi(b * 0.5f, ct, st);
        sincos2pi(a, cp, sp);
        lx = -sp * st; ly = ct; lz = -cp * st;
    } else if (MODEL == RT3_LENS_FISHEYE) {
        const float m = 0.5f * (float)(F.width < F.height ? F.width : F.height);
        const float nx = (px - 0.5f * W) / m;
        const float ny = (0.5f * H - py) / m;
        const float r = __builtin_sqrtf(nx * nx + ny * ny);
        const float tau = __builtin_fminf(r * L.half_fov_turns, 0.5f);
        float c, sn;
        sincos2pi(tau, c, sn);
        const float k = r > 0.0f ? sn / r : 0.0f;
        lx = nx * k; ly = ny * k; lz = c;
    } else if (MODEL == RT3_LENS_ORTHO) {
        const float nx = a * 2.0f - 1.0f;
        const float ny = 1.0f - b * 2.0f;
        const float e1 = nx * L.half_extent[0];
        const float e2 = ny * L.half_extent[1];
        for (int c = 0; c < 3; c++) o[c] = (L.origin[c] + e1 * L.right[c]) + e2 * L.up[c];
        lx = 0.0f; ly = 0.0f; lz = 1.0f;
    } else {                                                        // RT3_LENS_CUBE: the sampling law's face table (rt3.h "Environment map: sampling")
        const uint32_t N = F.width;
        const uint32_t f = y / N;
        const uint32_t j = y - f * N;
        const float sc = a * 2.0f - 1.0f;
        const float tc = ((((float)j + 0.5f) - jy) / (float)N) * 2.0f - 1.0f;
        float vx, vy, vz;
        switch (f) {
        case 0:  vx = 1.0f;  vy = -tc;   vz = -sc;   break;
        case 1:  vx = -1.0f; vy = -tc;   vz = sc;    break;
        case 2:  vx = sc;    vy = 1.0f;  vz = tc;    break;
        case 3:  vx = sc;    vy = -1.0f; vz = -tc;   break;
        case 4:  vx = sc;    vy = -tc;   vz = 1.0f;  break;
        default: vx = -sc;   vy = -tc;   vz = -1.0f; break;
        }
        lx = vx; ly = vy; lz = -vz;
    }
    float w[3];
    for (int c = 0; c < 3; c++) w[c] = (lx * L.right[c] + ly * L.up[c]) + lz * L.forward[c];
    const float inv = 1.0f / __builtin_sqrtf(dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
    d[0] = w[0] * inv; d[1] = w[1] * inv; d[2] = w[2] * inv;
}

// The same with the model taken from the lens (the host's form).
inline void ray_of(const rt3_lens& L, const Frame& F, uint32_t x, uint32_t y, uint32_t s, float o[3], float d[3]) {
    switch (L.model) {
    case RT3_LENS_EQUIRECT: ray<RT3_LENS_EQUIRECT>(L, F, x, y, s, o, d); break;
    case RT3_LENS_FISHEYE:  ray<RT3_LENS_FISHEYE>(L, F, x, y, s, o, d); break;
    case RT3_LENS_ORTHO:    ray<RT3_LENS_ORTHO>(L, F, x, y, s, o, d); break;
    default:                ray<RT3_LENS_CUBE>(L, F, x, y, s, o, d); break;
    }
}

// ---- The inverse law (rt3.h "Lens sequences"): from a world point back to a frame position.

// The angle of the vector (c, s) in turns, in [0, 1): plain f32 * + - / and comparisons (no fma), an odd degree-17 polynomial of atan on [0, 1]
// (Abramowitz & Stegun 4.4.49) and three reflections.  NaN for (0, 0) and for a component that is not finite.  Within 2^-23 turns of atan2.
RT3_HD float turns(float c, float s) {
    const float ac = __builtin_fabsf(c), as = __builtin_fabsf(s);
    const float hi = ac > as ? ac : as, lo = ac > as ? as : ac;
    if (!finite(ac) || !finite(as) || !(hi > 0.0f)) return __builtin_nanf("");
    const float t = lo / hi;
    const float z = t * t;
    float p = 0.0028662257f;
    p = p * z; p = p + -0.0161657367f;
    p = p * z; p = p + 0.0429096138f;
    p = p * z; p = p + -0.0752896400f;
    p = p * z; p = p + 0.1065626393f;
    p = p * z; p = p + -0.1420889944f;
    p = p * z; p = p + 0.1999355085f;
    p = p * z; p = p + -0.3333314528f;
    p = p * z; p = p + 1.0f;
    float u = (t * p) * 0.159154937f;
    if (as > ac) u = 0.25f - u;
    if (c < 0.0f) u = 0.5f - u;
    if (s < 0.0f) u = 1.0f - u;
    if (u >= 1.0f) u = 0.0f;
    return u;
}

// Bit equality of the fields the inverse law reads: the model, the origin, the three axes and the model's own parameter.
inline bool same_optic(const rt3_lens& a, const rt3_lens& b) {
    if (a.model != b.model) return false;
    bool same = __builtin_memcmp(a.origin, b.origin, 12) == 0 && __builtin_memcmp(a.right, b.right, 12) == 0 &&
                __builtin_memcmp(a.up, b.up, 12) == 0 && __builtin_memcmp(a.forward, b.forward, 12) == 0;
    if (a.model == RT3_LENS_FISHEYE) same = same && __builtin_memcmp(&a.half_fov_turns, &b.half_fov_turns, 4) == 0;
    if (a.model == RT3_LENS_ORTHO) same = same && __builtin_memcmp(a.half_extent, b.half_extent, 8) == 0;
    return same;
}

// r (the point relative to the lens's origin; for a miss of a central model the direction) -> the frame position (x', y') in the pixel-index
// coordinates of the taps (pixel centres at integers), the depth zhat the history's is compared with, and for CUBE the face the taps stay on.
// false: no history (the pole behind a fisheye, r = 0).  L is the PREVIOUS lens, W x H its frame.  An ORTHO miss is not projected: the caller
// keeps x' = x, y' = y.
template <uint32_t MODEL>
RT3_HD bool project(const rt3_lens& L, uint32_t width, uint32_t height, const float r[3], float& xp, float& yp, float& zhat, uint32_t& face) {
    const float W = (float)width, H = (float)height;
    const float lx = dot3(r[0], r[1], r[2], L.right[0], L.right[1], L.right[2]);
    const float ly = dot3(r[0], r[1], r[2], L.up[0], L.up[1], L.up[2]);
    const float lz = dot3(r[0], r[1], r[2], L.forward[0], L.forward[1], L.forward[2]);
    zhat = MODEL == RT3_LENS_ORTHO ? lz : __builtin_sqrtf(dot3(r[0], r[1], r[2], r[0], r[1], r[2]));
    face = 0;
    float px, py;
    if (MODEL == RT3_LENS_EQUIRECT) {
        const float hxz = __builtin_sqrtf(lx * lx + lz * lz);
        const float a = turns(-lz, -lx);
        const float b = 2.0f * turns(ly, hxz);
        px = a * W; py = b * H;
    } else if (MODEL == RT3_LENS_FISHEYE) {
        const float hxy = __builtin_sqrtf(lx * lx + ly * ly);
        const float tau = turns(lz, hxy);
        const float rr = tau / L.half_fov_turns;
        float nx, ny;
        if (hxy > 0.0f) { nx = rr * (lx / hxy); ny = rr * (ly / hxy); }
        else if (tau == 0.0f) { nx = 0.0f; ny = 0.0f; }
        else return false;
        const float m = 0.5f * (float)(width < height ? width : height);
        px = nx * m + 0.5f * W; py = 0.5f * H - ny * m;
    } else if (MODEL == RT3_LENS_ORTHO) {
        const float nx = lx / L.half_extent[0];
        const float ny = ly / L.half_extent[1];
        px = ((nx + 1.0f) * 0.5f) * W; py = ((1.0f - ny) * 0.5f) * H;
    } else {                                                        // RT3_LENS_CUBE: the lookup law's face cases (rt3.h "Environment map")
        const float vx = lx, vy = ly, vz = -lz;
        const float ax = __builtin_fabsf(vx), ay = __builtin_fabsf(vy), az = __builtin_fabsf(vz);
        float m, sc, tc;
        if (ax >= ay && ax >= az) { face = vx < 0.0f ? 1u : 0u; m = ax; sc = vx < 0.0f ? vz : -vz; tc = -vy; }
        else if (ay >= az)        { face = vy < 0.0f ? 3u : 2u; m = ay; sc = vx; tc = vy < 0.0f ? -vz : vz; }
        else                      { face = vz < 0.0f ? 5u : 4u; m = az; sc = vz < 0.0f ? -vx : vx; tc = -vy; }
        px = ((sc / m) * 0.5f + 0.5f) * W; py = (float)(face * width) + ((tc / m) * 0.5f + 0.5f) * W;
    }
    xp = px - 0.5f; yp = py - 0.5f;
    return xp == xp && yp == yp;
}

// The same with the model taken from the lens (the host's form).
inline bool project_of(const rt3_lens& L, uint32_t width, uint32_t height, const float r[3], float& xp, float& yp, float& zhat, uint32_t& face) {
    switch (L.model) {
    case RT3_LENS_EQUIRECT: return project<RT3_LENS_EQUIRECT>(L, width, height, r, xp, yp, zhat, face);
    case RT3_LENS_FISHEYE:  return project<RT3_LENS_FISHEYE>(L, width, height, r, xp, yp, zhat, face);
    case RT3_LENS_ORTHO:    return project<RT3_LENS_ORTHO>(L, width, height, r, xp, yp, zhat, face);
    default:                return project<RT3_LENS_CUBE>(L, width, height, r, xp, yp, zhat, face);
    }
}

}  // namespace rt3lens
