// rt3_shared_kernels.hpp — the device code both rt3_device.hip and rt3_scene.hip launch from, and nothing else: each unit compiles a copy of its own
// (DESIGN.md 5.6).  k_fill_words: the adaptive render's counts there, the slots and group orders of a device upload here.  block_sum: the ordered
// compactions of both (k_adaptive_count / k_adaptive_select, k_compact_count / k_compact_select).  Needs kBlock (rt3_kernel_common.hpp).
#pragma once

namespace {

__global__ __launch_bounds__(kBlock) void k_fill_words(uint32_t* __restrict__ out, uint32_t n, uint32_t value) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = value;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds) {       // sum over the block of kBlock threads, in every thread
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (uint32_t w = 0; w < kBlock / 64; w++) t += lds[w];
    __syncthreads();
    return t;
}

}  // namespace
