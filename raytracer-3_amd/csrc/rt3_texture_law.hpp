// rt3_texture_law.hpp — the image texture law (rt3.h "Image textures"): the bilinear lookup of (u, v), a sphere's (u, v) from its unit
// outward normal and a face's (u, v) from the hit point, one statement for the device and the host.
// Included by rt3_device.hip (shade_lane of the texture forms and k_aov_accumulate, through tex_modulate in rt3_kernel_common.hpp) and by rt3_host.cpp
// (rt3_debug_texture_lookup, rt3_debug_texture_sphere_uv, rt3_debug_texture_face_uv: the serial restatement the tests compare with
// tests/texture_ref.py).  Every float operation is an IEEE f32 operation rounded on its own (every file is compiled with -ffp-contract=off), nothing is
// fused; dot(a, b) = (ax bx + ay by) + az bz.
#pragma once
#include <cstdint>

#include "rt3.h"
#include "rt3_lens_law.hpp"                                          // rt3lens::turns: an angle in turns without a library transcendental

namespace rt3tex {

// One axis of a lookup: the coordinate u over n texels -> the two taps and the weight of the second.  REPEAT takes u - floor(u) first and wraps the taps
// (-1 -> n - 1, n -> 0); CLAMP keeps u and clamps them to [0, n - 1].  The floor is clamped to [-1, n - 1] in float with the NaN-dropping min / max
// BEFORE the conversion (a NaN becomes -1), as the environment law does: whatever u holds, both taps lie inside the image.
RT3_HD void axis(float u, uint32_t n, uint32_t wrap, uint32_t& i0, uint32_t& i1, float& w) {
    if (wrap == RT3_TEX_REPEAT) u = u - __builtin_floorf(u);
    const float f = u * (float)n - 0.5f;
    const float f0 = __builtin_floorf(f);
    w = f - f0;
    const int k = (int)__builtin_fminf(__builtin_fmaxf(f0, -1.0f), (float)n - 1.0f);
    const int last = (int)n - 1;
    if (wrap == RT3_TEX_REPEAT) { i0 = (uint32_t)(k < 0 ? last : k); i1 = (uint32_t)(k + 1 > last ? 0 : k + 1); }
    else                        { i0 = (uint32_t)(k > 0 ? k : 0);    i1 = (uint32_t)(k + 1 < last ? k + 1 : last); }
}

// The four taps' indices and the two weights of (u, v) in a w x h image (row 0 on top, texel (i, j) at j * w + i).
struct Taps { uint32_t i00, i10, i01, i11; float wx, wy; };
RT3_HD Taps taps(uint32_t w, uint32_t h, uint32_t wrap, float u, float v) {
    uint32_t i0, i1, j0, j1;
    Taps t;
    axis(u, w, wrap, i0, i1, t.wx);
    axis(v, h, wrap, j0, j1, t.wy);
    t.i00 = j0 * w + i0; t.i10 = j0 * w + i1; t.i01 = j1 * w + i0; t.i11 = j1 * w + i1;         // (w * h <= 2^26: no overflow)
    return t;
}
// The environment law's combination of the four texels: a one-colour texture returns that colour exactly (c + w * 0 = c for every finite weight; a
// weight that is not finite — a non-finite or overflowing u or v — gives NaN, from texels inside the image all the same).
RT3_HD float mix(float c00, float c10, float c01, float c11, float wx, float wy) {
    const float top = c00 + wx * (c10 - c00), bot = c01 + wx * (c11 - c01);
    return top + wy * (bot - top);
}
// T4: a texel with members x, y, z (the device's float4, the host's four floats).  The four loads are independent and stand together.
template <class T4>
RT3_HD void lookup(const T4* tex, uint32_t w, uint32_t h, uint32_t wrap, float u, float v, float& r, float& g, float& b) {
    const Taps t = taps(w, h, wrap, u, v);
    const T4 c00 = tex[t.i00], c10 = tex[t.i10], c01 = tex[t.i01], c11 = tex[t.i11];
    r = mix(c00.x, c10.x, c01.x, c11.x, t.wx, t.wy);
    g = mix(c00.y, c10.y, c01.y, c11.y, t.wx, t.wy);
    b = mix(c00.z, c10.z, c01.z, c11.z, t.wx, t.wy);
}

// A sphere's (u, v) from its unit outward normal n = (p - C) * (1 / r), before the flip towards the ray: the book's u = (atan2(-z, x) + pi) / 2 pi,
// and v = 0 at the north pole (+y), 1 at the south pole.  At a pole (hxz == 0) u is 0.
RT3_HD void sphere_uv(float nx, float ny, float nz, float& u, float& v) {
    const float hxz = __builtin_sqrtf(nx * nx + nz * nz);
    u = hxz > 0.0f ? rt3lens::turns(-nx, nz) : 0.0f;
    v = 2.0f * rt3lens::turns(ny, hxz);
}

// A face's (u, v) at the point p of its plane: the barycentric coordinates of p from the Gram matrix of the two edges at p1, then the vertices' own
// (u, v) weighted by them.  uv6 = (u1, v1, u2, v2, u3, v3).  A degenerate face (den == 0) takes b2 = b3 = 0: the first vertex's (u, v).
RT3_HD float dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RT3_HD void face_uv(const float p1[3], const float p2[3], const float p3[3], const float uv6[6], const float p[3], float& u, float& v) {
    const float e1[3] = { p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2] };
    const float e2[3] = { p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2] };
    const float q[3] = { p[0] - p1[0], p[1] - p1[1], p[2] - p1[2] };
    const float d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), q1 = dot(q, e1), q2 = dot(q, e2);
    const float den = d11 * d22 - d12 * d12;
    float b2 = 0.0f, b3 = 0.0f;
    if (!(den == 0.0f)) { b2 = (d22 * q1 - d12 * q2) / den; b3 = (d11 * q2 - d12 * q1) / den; }
    const float b1 = (1.0f - b2) - b3;
    u = (b1 * uv6[0] + b2 * uv6[2]) + b3 * uv6[4];
    v = (b1 * uv6[1] + b2 * uv6[3]) + b3 * uv6[5];
}

}  // namespace rt3tex
