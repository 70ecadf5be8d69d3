// rt3_display_sequence.hip — display sequences (rt3_display_sequence*): rt3_display with an exposure that follows the
// sequence and a bloom pyramid added before the tone curve.  The law is rt3_display_sequence_law.hpp, shared with the host restatement; the
// histogram and the map without bloom are rt3_display.hip's own kernels, launched through rt3_display.hpp.  Here: the gain kernel with the
// adaptation step, the pyramid (bright pass fused into the first reduction, the reductions, the in-place up-sampling sums) and the map that
// composites the bloom on the fly.  Every plane is float4 texels, one thread per texel, a capped grid with a grid-stride loop: streaming passes.
// A translation unit of its own (gfx950 only), as rt3_display.hip is.  rt3_device.hip checks the arguments, owns the buffers and calls
// display_sequence_launch().
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt3_display_sequence_law.hpp"
#include "rt3_display.hpp"
#include "rt3_display_sequence.hpp"

static_assert(sizeof(rt3_exposure) == 16, "rt3.h: rt3_exposure");
static_assert(sizeof(rt3_display_sequence_params) == 64, "rt3.h: rt3_display_sequence_params");

namespace {

using namespace rt3dseq;

constexpr uint32_t kSeqBlock = 256;
constexpr uint32_t kSeqMaxGrid = 2048;                              // as rt3_display.hip: 256 CUs x 8 blocks, the rest by the grid-stride loop
constexpr uint32_t kCountSlot = kBins + 1, kGainSlot = kBins + 2;   // the state's words behind the histogram, where k_display_gain leaves them

uint32_t seq_grid(uint32_t n) {
    const uint32_t want = (n + kSeqBlock - 1) / kSeqBlock;
    return want < kSeqMaxGrid ? want : kSeqMaxGrid;
}

__device__ inline Rgb rgb_of(const float4& v) { return Rgb{ v.x, v.y, v.z }; }
__device__ inline float4 texel_of(const Rgb& c) { return make_float4(c.r, c.g, c.b, 0.0f); }
__device__ inline Plane plane_of(const float4* p, uint32_t w, uint32_t h) { return Plane{ reinterpret_cast<const float*>(p), w, h }; }

// k_display_gain with one more thread-0 tail: the frame's target P_t instead of its gain, then the step from prev's level towards it; the state after
// the frame goes to out (if any) and its gain behind the histogram, where k_display_map and the bloom kernels read it.  prev == out is allowed:
// thread 0 has read prev before it writes.
__global__ __launch_bounds__(kBins) void k_display_gain_step(uint32_t* __restrict__ state, uint32_t trim_low, uint32_t trim_high, float exposure, float key,
                                                             const rt3_exposure* prev, rt3_exposure* out, uint32_t brighter, uint32_t darker) {
    __shared__ uint32_t s_end[kBins];
    __shared__ uint64_t s_sum[kBins];
    const uint32_t k = threadIdx.x;
    const uint32_t h = state[k];
    s_end[k] = h;
    __syncthreads();
    for (uint32_t off = 1; off < kBins; off <<= 1) {
        const uint32_t v = k >= off ? s_end[k - off] : 0u;
        __syncthreads();
        s_end[k] += v;
        __syncthreads();
    }
    const uint64_t n = s_end[kBins - 1], end = s_end[k], begin = end - h;     // n <= 2^26: the scan fits 32 bits
    uint32_t target = 0u;
    if (n != 0) {                                                   // (the whole block takes the same side)
        const Trim t = trim_of(n, trim_low, trim_high);
        s_sum[k] = kept(t, begin, end) * k;
        __syncthreads();
        for (uint32_t off = kBins / 2; off > 0; off >>= 1) {
            if (k < off) s_sum[k] += s_sum[k + off];
            __syncthreads();
        }
        if (k == 0) target = level_from_sum(t, s_sum[0]);
    }
    if (k == 0) {
        const uint32_t prev_level = prev ? prev->level : 0u, prev_frames = prev ? prev->frames : 0u;
        const rt3_exposure next = exposure_next(prev_level, prev_frames, n, target, brighter, darker, exposure, key);
        state[kCountSlot] = (uint32_t)n;
        state[kGainSlot] = bits_of(next.gain);
        if (out) { out->level = next.level; out->frames = next.frames; out->gain = next.gain; out->_pad = 0u; }
    }
}

// Without auto-exposure: the record of a call with a given gain.
__global__ void k_exposure_given(rt3_exposure* out, float gain) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = rt3_exposure{ 0u, 0u, gain, 0u };
}

// D_1: the bright pass of the four input pixels under a texel, then the first reduction.  The frame is read once, 16 bytes per pixel (the clamped
// last column and row of an odd size twice).
template <bool AUTO>
__global__ __launch_bounds__(kSeqBlock) void k_bloom_down_first(const float4* __restrict__ in, uint32_t w0, uint32_t h0, float4* __restrict__ d1, uint32_t w1,
                                                               uint32_t h1, float exposure, const uint32_t* __restrict__ state, float threshold) {
    const float gain = AUTO ? float_of(state[kGainSlot]) : exposure;
    const uint32_t n = w1 * h1, stride = gridDim.x * kSeqBlock;     // n <= 2^25: no wrap
    for (uint32_t t = blockIdx.x * kSeqBlock + threadIdx.x; t < n; t += stride) {
        const uint32_t j = t / w1, i = t - j * w1;
        const uint32_t ia = down_a(i, w0), ib = down_b(i, w0), ja = down_a(j, h0), jb = down_b(j, h0);
        const float4 a = in[(size_t)ja * w0 + ia], b = in[(size_t)ja * w0 + ib], c = in[(size_t)jb * w0 + ia], d = in[(size_t)jb * w0 + ib];
        d1[t] = texel_of(down4(bright(exposed(a.x, a.y, a.z, gain), threshold), bright(exposed(b.x, b.y, b.z, gain), threshold),
                               bright(exposed(c.x, c.y, c.z, gain), threshold), bright(exposed(d.x, d.y, d.z, gain), threshold)));
    }
}

// D_l of D_{l-1}.
__global__ __launch_bounds__(kSeqBlock) void k_bloom_down(const float4* __restrict__ src, uint32_t ws, uint32_t hs, float4* __restrict__ dst, uint32_t wd,
                                                         uint32_t hd) {
    const Plane s = plane_of(src, ws, hs);
    const uint32_t n = wd * hd, stride = gridDim.x * kSeqBlock;
    for (uint32_t t = blockIdx.x * kSeqBlock + threadIdx.x; t < n; t += stride) {
        const uint32_t j = t / wd, i = t - j * wd;
        dst[t] = texel_of(down_texel(s, i, j));
    }
}

// U_l = D_l + up(U_{l+1}), in place on D_l: a thread reads and writes its own texel of D_l and reads four of the coarser plane.
__global__ __launch_bounds__(kSeqBlock) void k_bloom_up(const float4* __restrict__ coarse, uint32_t wc, uint32_t hc, float4* __restrict__ fine, uint32_t w,
                                                       uint32_t h) {
    const Plane u = plane_of(coarse, wc, hc);
    const uint32_t n = w * h, stride = gridDim.x * kSeqBlock;
    for (uint32_t t = blockIdx.x * kSeqBlock + threadIdx.x; t < n; t += stride) {
        const uint32_t j = t / w, i = t - j * w;
        fine[t] = texel_of(sum(rgb_of(fine[t]), up_texel(u, i, j)));
    }
}

// k_display_map with the bloom: the pixel and the four U_1 texels around it, B formed on the fly, the composite, the curve, the transfer, the word.
// SRGB: the table is staged in LDS as in k_display_map.
template <uint32_t CURVE, uint32_t TRANSFER, bool AUTO>
__global__ __launch_bounds__(kSeqBlock) void k_display_map_bloom(const float4* __restrict__ in, uint32_t* __restrict__ out, uint32_t w0, uint32_t h0,
                                                                const float4* __restrict__ u1, uint32_t w1, uint32_t h1, float exposure,
                                                                const uint32_t* __restrict__ state, float white, float intensity, float weight) {
    __shared__ __attribute__((aligned(16))) uint8_t s_table[TRANSFER == RT3_DISPLAY_SRGB ? 4096 : 16];
    if (TRANSFER == RT3_DISPLAY_SRGB) {
        static_assert(kSeqBlock * 16 == sizeof(kSrgbTable), "one uint4 of the table per thread");
        reinterpret_cast<uint4*>(s_table)[threadIdx.x] = reinterpret_cast<const uint4*>(kSrgbTable)[threadIdx.x];
        __syncthreads();
    }
    const float gain = AUTO ? float_of(state[kGainSlot]) : exposure;
    const Plane u = plane_of(u1, w1, h1);
    const uint32_t n = w0 * h0, stride = gridDim.x * kSeqBlock;
    for (uint32_t t = blockIdx.x * kSeqBlock + threadIdx.x; t < n; t += stride) {
        const uint32_t j = t / w0, i = t - j * w0;
        const float4 c = in[t];
        const Rgb x = composite(exposed(c.x, c.y, c.z, gain), bloom_texel(u, i, j, weight), intensity);
        out[t] = word_of(x.r, x.g, x.b, CURVE, TRANSFER, white, s_table);
    }
}

using BloomMapKernel = void (*)(const float4*, uint32_t*, uint32_t, uint32_t, const float4*, uint32_t, uint32_t, float, const uint32_t*, float, float, float);
template <uint32_t CURVE, bool AUTO>
BloomMapKernel bloom_map_of(uint32_t transfer) {
    return transfer == RT3_DISPLAY_LINEAR ? k_display_map_bloom<CURVE, RT3_DISPLAY_LINEAR, AUTO>
         : transfer == RT3_DISPLAY_GAMMA2 ? k_display_map_bloom<CURVE, RT3_DISPLAY_GAMMA2, AUTO> : k_display_map_bloom<CURVE, RT3_DISPLAY_SRGB, AUTO>;
}
template <bool AUTO>
BloomMapKernel bloom_map_of(uint32_t curve, uint32_t transfer) {
    return curve == RT3_DISPLAY_CLAMP ? bloom_map_of<RT3_DISPLAY_CLAMP, AUTO>(transfer)
         : curve == RT3_DISPLAY_REINHARD ? bloom_map_of<RT3_DISPLAY_REINHARD, AUTO>(transfer) : bloom_map_of<RT3_DISPLAY_FILMIC, AUTO>(transfer);
}

// Tests only: B stored at the frame's size, by the device function the composite calls.
__global__ __launch_bounds__(kSeqBlock) void k_bloom_plane(const float4* __restrict__ u1, uint32_t w1, uint32_t h1, float4* __restrict__ out, uint32_t w0,
                                                          uint32_t h0, float weight) {
    const Plane u = plane_of(u1, w1, h1);
    const uint32_t n = w0 * h0, stride = gridDim.x * kSeqBlock;
    for (uint32_t t = blockIdx.x * kSeqBlock + threadIdx.x; t < n; t += stride) {
        const uint32_t j = t / w0, i = t - j * w0;
        out[t] = texel_of(bloom_texel(u, i, j, weight));
    }
}

}  // namespace

hipError_t display_sequence_launch(const DisplaySequenceLaunch& S, hipStream_t stream) {
    const DisplayLaunch& L = S.display;
    hipError_t e;
    if (L.auto_exposure) {
        if ((e = display_histogram_launch(L, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_display_gain_step, dim3(1), dim3(kBins), 0, stream, L.state, L.trim_low, L.trim_high, L.exposure, L.key, S.prev, S.out_exposure,
                           S.adapt_brighter, S.adapt_darker);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    } else if (S.out_exposure) {
        hipLaunchKernelGGL(k_exposure_given, dim3(1), dim3(64), 0, stream, S.out_exposure, L.exposure);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (S.bloom_levels == 0) return display_map_launch(L, stream);

    const float4* in = (const float4*)L.rgba;
    float4* plane[kMaxBloomLevels];
    uint32_t w[kMaxBloomLevels + 1] = { S.width }, h[kMaxBloomLevels + 1] = { S.height };
    float4* next = (float4*)S.pyramid;
    for (uint32_t l = 1; l <= S.bloom_levels; l++) {
        w[l] = half_of(w[l - 1]); h[l] = half_of(h[l - 1]);
        plane[l - 1] = next;
        next += (size_t)w[l] * h[l];
    }
    const dim3 block(kSeqBlock);
    if (L.auto_exposure)
        hipLaunchKernelGGL(k_bloom_down_first<true>, dim3(seq_grid(w[1] * h[1])), block, 0, stream, in, w[0], h[0], plane[0], w[1], h[1], L.exposure,
                           (const uint32_t*)L.state, S.bloom_threshold);
    else
        hipLaunchKernelGGL(k_bloom_down_first<false>, dim3(seq_grid(w[1] * h[1])), block, 0, stream, in, w[0], h[0], plane[0], w[1], h[1], L.exposure,
                           (const uint32_t*)L.state, S.bloom_threshold);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (uint32_t l = 2; l <= S.bloom_levels; l++) {
        hipLaunchKernelGGL(k_bloom_down, dim3(seq_grid(w[l] * h[l])), block, 0, stream, (const float4*)plane[l - 2], w[l - 1], h[l - 1], plane[l - 1], w[l], h[l]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (uint32_t l = S.bloom_levels - 1; l >= 1; l--) {
        hipLaunchKernelGGL(k_bloom_up, dim3(seq_grid(w[l] * h[l])), block, 0, stream, (const float4*)plane[l], w[l + 1], h[l + 1], plane[l - 1], w[l], h[l]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const BloomMapKernel map = L.auto_exposure ? bloom_map_of<true>(L.curve, L.transfer) : bloom_map_of<false>(L.curve, L.transfer);
    hipLaunchKernelGGL(map, dim3(seq_grid(L.npix)), block, 0, stream, in, (uint32_t*)L.out, w[0], h[0], (const float4*)plane[0], w[1], h[1], L.exposure,
                       (const uint32_t*)L.state, L.white, S.bloom_intensity, level_weight(S.bloom_levels));
    return hipGetLastError();
}

hipError_t bloom_plane_launch(const void* u1, uint32_t w1, uint32_t h1, void* out, uint32_t w0, uint32_t h0, uint32_t levels, hipStream_t stream) {
    hipLaunchKernelGGL(k_bloom_plane, dim3(seq_grid(w0 * h0)), dim3(kSeqBlock), 0, stream, (const float4*)u1, w1, h1, (float4*)out, w0, h0, level_weight(levels));
    return hipGetLastError();
}
