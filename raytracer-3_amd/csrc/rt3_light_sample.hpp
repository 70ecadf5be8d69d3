// rt3_light_sample.hpp — the emitters' sampling table and sampling law (rt3.h "Emitters: sampling"), one statement for the device and the host.
// Included by rt3_scene.hip (the table kernels of rt3_light_table.hpp), by rt3_device.hip (shade_lane of the light sampling forms) and by rt3_host.cpp
// (rt3_debug_light_sample, the serial restatement the tests compare with tests/light_sample_ref.py).  As in rt3_env_sample.hpp: integers wherever a sum
// is taken, every float operation an IEEE f32 operation rounded on its own (both files are compiled with -ffp-contract=off), every fused multiply-add
// written out.
#pragma once
#include <cstdint>

#include "rt3_env_sample.hpp"

namespace rt3light {

using rt3env::hash_u32;
using rt3env::u01;
using rt3env::mul_hi_u64;
using rt3env::quantise;
using rt3env::kFltMax;

constexpr uint32_t kMatFlat = 0u;                                   // RT3_MAT_FLAT (rt3.h; static_asserted where both are visible)
constexpr uint32_t kNoLight = 0xFFFFFFFFu;

RT3_HD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
RT3_HD float dotf(float ax, float ay, float az, float bx, float by, float bz) { return fma_(az, bz, fma_(ay, by, ax * bx)); }   // rt3_kernel_common.hpp's

// The scatter's own random unit vector (unit_vector and sincos2pi of rt3_kernel_common.hpp, operation for operation), here for both compilers.
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
RT3_HD void unit_vector(float xi0, float xi1, float& x, float& y, float& z) {
    z = fma_(-2.0f, xi0, 1.0f);
    const float rr = fma_(-z, z, 1.0f);
    const float r = __builtin_sqrtf(rr > 0.0f ? rr : 0.0f);
    float c, s;
    sincos2pi(xi1, c, s);
    x = r * c;
    y = r * s;
}

// A primitive's brightness: the positive parts of a FLAT material's rgb added (a NaN counts as 0, +inf is clamped to FLT_MAX); any other kind: 0.
RT3_HD float brightness(uint32_t kind, float r, float g, float b) { return kind == kMatFlat ? rt3env::texel_brightness(r, g, b) : 0.0f; }

// A face: its edges from p1, their cross product x (every product and difference rounded on its own) and g2 = |x|^2 as the fused chain.
struct Face { float p1x, p1y, p1z, e1x, e1y, e1z, e2x, e2y, e2z, xx, xy, xz, g2; };
RT3_HD void face_of(const float p1[3], const float p2[3], const float p3[3], Face& f) {
    f.p1x = p1[0]; f.p1y = p1[1]; f.p1z = p1[2];
    f.e1x = p2[0] - p1[0]; f.e1y = p2[1] - p1[1]; f.e1z = p2[2] - p1[2];
    f.e2x = p3[0] - p1[0]; f.e2y = p3[1] - p1[1]; f.e2z = p3[2] - p1[2];
    f.xx = f.e1y * f.e2z - f.e1z * f.e2y;
    f.xy = f.e1z * f.e2x - f.e1x * f.e2z;
    f.xz = f.e1x * f.e2y - f.e1y * f.e2x;
    f.g2 = fma_(f.xz, f.xz, fma_(f.xy, f.xy, f.xx * f.xx));
}
RT3_HD float face_area(const Face& f) { return 0.5f * __builtin_sqrtf(f.g2); }
RT3_HD float sphere_area(float r) { return 12.566371f * (r * r); }
// w = l a: 0 for a NaN product and for an area that is not finite and > 0 (a degenerate face, a sphere record nothing can hit); +inf clamped.
RT3_HD float weight(float l, float a) {
    if (!(a > 0.0f) || !(a < __builtin_inff())) return 0.0f;
    const float w = l * a;
    if (w != w) return 0.0f;
    return __builtin_fminf(w, kFltMax);
}

// What a Lambert scatter of a path with RNG base `base` at depth `depth` draws (counters 3..6 of the scatter's block 1 + 8 (depth + 1)): the light by
// binary search of a 64-bit draw scaled to [0, total) in the inclusive prefix sums cdf[0 .. n) (total = cdf[n - 1] != 0), and the two numbers of the point.
RT3_HD uint32_t pick(const uint64_t* cdf, uint32_t n, uint64_t total, uint32_t base, uint32_t depth, float& a, float& b) {
    const uint32_t ctr = 1u + 8u * (depth + 1u);
    const uint32_t w3 = hash_u32(base ^ hash_u32(ctr + 3u)), w4 = hash_u32(base ^ hash_u32(ctr + 4u));
    const uint32_t w5 = hash_u32(base ^ hash_u32(ctr + 5u)), w6 = hash_u32(base ^ hash_u32(ctr + 6u));
    const uint64_t x = ((uint64_t)w3 << 32) | w4;
    const uint64_t target = mul_hi_u64(x, total);                   // < total
    uint32_t lo = 0u, hi = n - 1u;                                  // the first entry with cdf > target: cdf[hi] = total > target
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1u;
    }
    a = u01(w5); b = u01(w6);
    return lo;
}

// The sampled point y, the light's normal there and the light's area.
struct Point { float x, y, z, nx, ny, nz, area; };
RT3_HD void point_on_face(const Face& f, float a, float b, Point& out) {
    if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
    out.x = fma_(b, f.e2x, fma_(a, f.e1x, f.p1x));
    out.y = fma_(b, f.e2y, fma_(a, f.e1y, f.p1y));
    out.z = fma_(b, f.e2z, fma_(a, f.e1z, f.p1z));
    const float inv = 1.0f / __builtin_sqrtf(f.g2);
    out.nx = f.xx * inv; out.ny = f.xy * inv; out.nz = f.xz * inv;
    out.area = face_area(f);
}
RT3_HD void point_on_sphere(float cx, float cy, float cz, float r, float a, float b, Point& out) {
    float vx, vy, vz;
    unit_vector(a, b, vx, vy, vz);
    out.x = fma_(r, vx, cx); out.y = fma_(r, vy, cy); out.z = fma_(r, vz, cz);
    out.nx = vx; out.ny = vy; out.nz = vz;
    out.area = sphere_area(r);
}

// The shadow ray from the hit point p (normal n turned towards the ray) to the sampled point: its unit direction w and the factor k that
// E = throughput x albedo x k is parked with.  false: the sample is dropped (rt3.h lists the cases).  sphere: the light is one, (cx, cy, cz, r).
RT3_HD bool connect(const Point& y, bool sphere, float cx, float cy, float cz, float r, float px, float py, float pz, float nx, float ny, float nz,
                    uint32_t q, uint64_t total, float& wx, float& wy, float& wz, float& k) {
    const float Dx = y.x - px, Dy = y.y - py, Dz = y.z - pz;
    const float d2 = dotf(Dx, Dy, Dz, Dx, Dy, Dz);
    if (!(d2 > 0.0f) || !(d2 < __builtin_inff())) return false;
    const float inv = 1.0f / __builtin_sqrtf(d2);
    wx = Dx * inv; wy = Dy * inv; wz = Dz * inv;
    const float dl = dotf(y.nx, y.ny, y.nz, wx, wy, wz);
    const float cl = __builtin_fabsf(dl);
    if (!(cl > 0.0f)) return false;
    const float c = dotf(nx, ny, nz, wx, wy, wz);
    if (!(c > 0.0f)) return false;
    if (sphere) {                                                   // from outside, the far half is hidden by the near one
        const float ux = px - cx, uy = py - cy, uz = pz - cz;
        if (dotf(ux, uy, uz, ux, uy, uz) > r * r && dl >= 0.0f) return false;
    }
    const float pl = (float)q / (float)total;
    k = ((c * cl) * y.area) / ((3.14159274f * d2) * pl);
    return true;
}

}  // namespace rt3light
