// rt3_light_table.hpp — the kernels that build the emitters' sampling table (RT3_FLAG_LIGHT_SAMPLING; rt3_light_sample.hpp)
// Part of rt3_scene.hip (one translation unit, gfx950 only); included from there, in this order.
#pragma once

namespace {

static_assert(rt3light::kMatFlat == RT3_MAT_FLAT, "rt3_light_sample.hpp: RT3_MAT_FLAT");

// One thread per entry, faces first and then spheres in the caller's order (the order of rt3_hit.index): the entry's weight (rt3light::weight of its
// brightness and its area) as a bit pattern into q[entry] — the place of the quantised weight, which needs the largest weight first — and the largest
// of all into *w_max.  Weights are >= 0, so their order is their bit patterns' order: a maximum of words, in any order (one atomic per wave).
// tri: the faces' records as k_commit_mesh wrote them (p1, p2, p3 in records 1..3); sph_cr: (C, r) as the caller gave them.
__global__ __launch_bounds__(kBlock) void k_light_weights(const float4* __restrict__ tri, const float4* __restrict__ tri_mat, const uint32_t* __restrict__ tri_kind,
                                                          uint32_t n_tri, const float4* __restrict__ sph_cr, const float4* __restrict__ sph_mat,
                                                          const uint32_t* __restrict__ sph_kind, uint32_t n_sph, uint32_t* __restrict__ q,
                                                          uint32_t* __restrict__ w_max) {
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bits = 0u;
    if (e < n_tri) {
        const float4 m = tri_mat[e];
        const float l = rt3light::brightness(tri_kind[e], m.x, m.y, m.z);
        const float4 a = tri[(size_t)e * 4 + 1], b = tri[(size_t)e * 4 + 2], c = tri[(size_t)e * 4 + 3];
        const float p1[3] = { a.x, a.y, a.z }, p2[3] = { b.x, b.y, b.z }, p3[3] = { c.x, c.y, c.z };
        rt3light::Face f;
        rt3light::face_of(p1, p2, p3, f);
        bits = __float_as_uint(rt3light::weight(l, rt3light::face_area(f)));
        q[e] = bits;
    } else if (e - n_tri < n_sph) {
        const uint32_t i = e - n_tri;
        const float4 m = sph_mat[i];
        const float l = rt3light::brightness(sph_kind[i], m.x, m.y, m.z);
        bits = __float_as_uint(rt3light::weight(l, rt3light::sphere_area(sph_cr[i].w)));
        q[e] = bits;
    }
    uint32_t top = bits;
    for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, d));
    if (lane_id() == 0 && top != 0u) atomicMax(w_max, top);
}
// One thread per entry: the weight's bit pattern in q[entry] becomes the quantised weight, and cdf[entry] the same number for the prefix sum that follows.
__global__ __launch_bounds__(kBlock) void k_light_quantise(uint32_t n, const uint32_t* __restrict__ w_max, uint32_t* __restrict__ q,
                                                           unsigned long long* __restrict__ cdf) {
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const uint32_t v = rt3light::quantise(__uint_as_float(q[e]), __uint_as_float(*w_max));
    q[e] = v;
    cdf[e] = v;
}

}  // namespace
