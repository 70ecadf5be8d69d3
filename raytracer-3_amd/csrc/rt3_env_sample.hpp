// rt3_env_sample.hpp — the environment map's sampling table and sampling law (rt3.h), one statement for the device and the host.
// Included by rt3_scene.hip (the table kernels), by rt3_device.hip (shade_lane of the sampling forms) and by rt3_host.cpp (rt3_debug_environment_sample, the serial
// restatement the tests compare with tests/environment_sample_ref.py).  Integers wherever a sum is taken, so the table does not depend on the order
// it was built in; every float operation is an IEEE f32 operation rounded on its own (both files are compiled with -ffp-contract=off), the one fused
// multiply-add — the dot product under the normalisation, as shade_lane normalises a scattered direction — is written out.
#pragma once
#include <cstdint>

#ifdef __HIP__
#define RT3_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RT3_HD inline
#endif

namespace rt3env {

constexpr uint32_t kMaxCellsPerEdge = 256;
constexpr float kFltMax = 3.40282347e+38f;
constexpr float kQuantum = 16777216.0f;                             // the largest cell weight becomes 2^24

RT3_HD uint32_t hash_u32(uint32_t x) { x += x << 10; x ^= x >> 6; x += x << 3; x ^= x >> 11; x += x << 15; return x; }      // rt3_kernel_common.hpp's
RT3_HD float u01(uint32_t m) { const uint32_t b = (m & 0x007FFFFFu) | 0x3F800000u; float f; __builtin_memcpy(&f, &b, 4); return f - 1.0f; }

// M cells per face edge.  Cell c of an axis is the interval [c / M, (c + 1) / M) of the face coordinate u; inside it the bilinear lookup
// (fx = u N - 0.5, texels floor(fx) and floor(fx) + 1, clamped) reads the texels cell_lo(c) .. cell_hi(c) and no other: floor(c N / M - 0.5) and
// floor((c + 1) N / M - 0.5) + 1 in integers, clamped to the face.  For N <= 256 (M = N) that is the cell's own texel and a ring of one around it.
RT3_HD uint32_t cells_per_edge(uint32_t n) { return n < kMaxCellsPerEdge ? n : kMaxCellsPerEdge; }
RT3_HD uint32_t cell_lo(uint32_t c, uint32_t n, uint32_t m) { return c == 0u ? 0u : (2u * c * n - m) / (2u * m); }
RT3_HD uint32_t cell_hi(uint32_t c, uint32_t n, uint32_t m) { const uint32_t h = (2u * (c + 1u) * n - m) / (2u * m) + 1u; return h < n ? h : n - 1u; }
// The in-face coordinate of the point a in [0, 1) of cell idx, and the solid-angle factor g sqrt(g), g = (s s + t t) + 1: dA / d omega at (s, t).
RT3_HD float cell_coord(uint32_t idx, float a, uint32_t m) { return (((float)idx + a) / (float)m) * 2.0f - 1.0f; }
RT3_HD float solid_factor(float s, float t) { const float g = (s * s + t * t) + 1.0f; return g * __builtin_sqrtf(g); }
// A texel's brightness: the channels' positive parts added (fmax drops a NaN: it counts as 0), +inf clamped to FLT_MAX.
RT3_HD float texel_brightness(float r, float g, float b) {
    const float l = (__builtin_fmaxf(r, 0.0f) + __builtin_fmaxf(g, 0.0f)) + __builtin_fmaxf(b, 0.0f);
    return __builtin_fminf(l, kFltMax);
}
// The weight of cell (face, row, col): the largest brightness among the texels the bilinear lookup can read inside the cell (cell_lo .. cell_hi on
// both axes), times the solid angle factor 1 / (g sqrt(g)) at the cell's centre.  rgba: 4 floats per texel.
RT3_HD float cell_weight(const float* rgba, uint32_t n, uint32_t m, uint32_t face, uint32_t row, uint32_t col) {
    const uint32_t i0 = cell_lo(col, n, m), i1 = cell_hi(col, n, m), j0 = cell_lo(row, n, m), j1 = cell_hi(row, n, m);                     // inclusive
    float l = 0.0f;
    for (uint32_t j = j0; j <= j1; j++) {
        const float* t = rgba + 4u * (((size_t)face * n + j) * n + i0);
        for (uint32_t i = i0; i <= i1; i++, t += 4) l = __builtin_fmaxf(l, texel_brightness(t[0], t[1], t[2]));
    }
    const float sa = 1.0f / solid_factor(cell_coord(col, 0.5f, m), cell_coord(row, 0.5f, m));
    return l * sa;
}
// w, and the largest w of the map, to the integer the prefix sums add: 0 stays 0, everything else is at least 1.
RT3_HD uint32_t quantise(float w, float w_max) {
    if (w == 0.0f) return 0u;
    const uint32_t q = (uint32_t)__builtin_floorf(w / w_max * kQuantum);
    return q > 1u ? q : 1u;
}

// The high 64 bits of a * b, from 32-bit halves (the same integers on the device and on the host).
RT3_HD uint64_t mul_hi_u64(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t mid = a1 * b0 + ((a0 * b0) >> 32);              // < 2^64: (2^32 - 1)^2 + 2^32 - 1
    const uint64_t mid2 = a0 * b1 + (uint32_t)mid;
    return a1 * b1 + (mid >> 32) + (mid2 >> 32);
}

struct Sample { uint32_t cell; float dx, dy, dz, pdf; };
// The sampling law: the direction a Lambert scatter of a path with RNG base `base` at depth `depth` draws from the table (q, cdf, m; total =
// cdf[6 m m - 1] != 0).  Counters 3..6 of the scatter's block 1 + 8 (depth + 1): the cell by binary search of a 64-bit draw scaled to [0, total),
// the point inside it uniformly in (s, t), the direction by the lookup's face cases inverted, the density per solid angle.
RT3_HD void sample(const uint32_t* q, const uint64_t* cdf, uint32_t m, uint64_t total, uint32_t base, uint32_t depth, Sample& out) {
    const uint32_t ctr = 1u + 8u * (depth + 1u);
    const uint32_t w3 = hash_u32(base ^ hash_u32(ctr + 3u)), w4 = hash_u32(base ^ hash_u32(ctr + 4u));
    const uint32_t w5 = hash_u32(base ^ hash_u32(ctr + 5u)), w6 = hash_u32(base ^ hash_u32(ctr + 6u));
    const uint64_t x = ((uint64_t)w3 << 32) | w4;
    const uint64_t target = mul_hi_u64(x, total);                   // < total
    uint32_t lo = 0u, hi = 6u * m * m - 1u;                         // the first cell with cdf > target: cdf[hi] = total > target
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1u;
    }
    const uint32_t cell = lo, face = cell / (m * m), in = cell - face * (m * m), row = in / m, col = in - row * m;
    const float s = cell_coord(col, u01(w5), m), t = cell_coord(row, u01(w6), m);
    float vx, vy, vz;
    switch (face) {
    case 0u: vx = 1.0f; vy = -t; vz = -s; break;
    case 1u: vx = -1.0f; vy = -t; vz = s; break;
    case 2u: vx = s; vy = 1.0f; vz = t; break;
    case 3u: vx = s; vy = -1.0f; vz = -t; break;
    case 4u: vx = s; vy = -t; vz = 1.0f; break;
    default: vx = -s; vy = -t; vz = -1.0f; break;
    }
    const float inv = 1.0f / __builtin_sqrtf(__builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx)));
    out.cell = cell;
    out.dx = vx * inv; out.dy = vy * inv; out.dz = vz * inv;
    out.pdf = ((float)q[cell] / (float)total) * ((float)(m * m) * 0.25f) * solid_factor(s, t);
}

}  // namespace rt3env
