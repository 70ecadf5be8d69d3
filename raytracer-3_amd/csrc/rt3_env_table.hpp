// rt3_env_table.hpp — the kernels that build the environment map's sampling table (RT3_FLAG_ENV_SAMPLING; rt3_env_sample.hpp)
// Part of rt3_scene.hip (one translation unit, gfx950 only); included from there, in this order.
#pragma once

namespace {

// One thread per cell: its weight (rt3env::cell_weight) as a bit pattern into q[cell] — the place of the quantised weight, which needs the map's
// largest weight first — and the largest of all into *w_max.  Weights are >= 0, so their order is their bit patterns' order: a maximum of words, which
// does not depend on the order it is taken in (one atomic per wave).
__global__ __launch_bounds__(kBlock) void k_env_cell_weights(const float4* __restrict__ env, uint32_t n, uint32_t m, uint32_t cells,
                                                             uint32_t* __restrict__ q, uint32_t* __restrict__ w_max) {
    const uint32_t cell = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bits = 0u;
    if (cell < cells) {
        const uint32_t face = cell / (m * m), in = cell - face * (m * m), row = in / m, col = in - row * m;
        bits = __float_as_uint(rt3env::cell_weight(reinterpret_cast<const float*>(env), n, m, face, row, col));
        q[cell] = bits;
    }
    uint32_t top = bits;
    for (int d = 32; d >= 1; d >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, d));
    if (lane_id() == 0 && top != 0u) atomicMax(w_max, top);
}
// One thread per cell: the weight's bit pattern in q[cell] becomes the quantised weight, and cdf[cell] the same number for the prefix sum that follows.
__global__ __launch_bounds__(kBlock) void k_env_quantise(uint32_t cells, const uint32_t* __restrict__ w_max, uint32_t* __restrict__ q,
                                                         unsigned long long* __restrict__ cdf) {
    const uint32_t cell = blockIdx.x * kBlock + threadIdx.x;
    if (cell >= cells) return;
    const uint32_t v = rt3env::quantise(__uint_as_float(q[cell]), __uint_as_float(*w_max));
    q[cell] = v;
    cdf[cell] = v;
}

}  // namespace
