// rt3_display_sequence.hip — display sequences (rt3_display_sequence*): rt3_display with an exposure that follows the
// sequence and a bloom pyramid added before the tone curve.  The law is rt3_display_sequence_law.hpp, shared with the host restatement; the
// histogram and the map without bloom are rt3_display.hip's own kernels, launched through rt3_display.hpp.  Here: the gain kernel with the
// adaptation step, the pyramid (bright pass fused into the first reduction, the reductions, the in-place up-sampling sums) and the map that
// composites the bloom on the fly.  Every plane is float4 texels, one thread per texel, a capped grid with a grid-stride loop: streaming passes.
// A translation unit of its own (gfx950 only), as rt3_display.hip is.  The entry points are below the kernels: they check the arguments, take the
// state and the pyramid from the context (rt3_ctx.hpp) and launch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt3_ctx.hpp"
#include "rt3_display_sequence_law.hpp"
#include "rt3_display.hpp"

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

// (rt3dseq::Rgb, the law's colour, spelled out: in this namespace a plain Rgb is the render path's radiance record, which rt3_ctx.hpp names)
__device__ inline rt3dseq::Rgb rgb_of(const float4& v) { return rt3dseq::Rgb{ v.x, v.y, v.z }; }
__device__ inline float4 texel_of(const rt3dseq::Rgb& c) { return make_float4(c.r, c.g, c.b, 0.0f); }
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
        const rt3dseq::Rgb x = composite(exposed(c.x, c.y, c.z, gain), bloom_texel(u, i, j, weight), intensity);
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

// ---- The entry points (rt3.h)
static int display_sequence_checks(rt3_ctx* ctx, uint32_t w, uint32_t h, const void* rgba, const rt3_display_sequence_params* p, const void* prev,
                                   const void* out_exposure, const void* out) {
    if (!p) return fail(ctx, RT3_E_ARG, "p is NULL");
    if (!rgba || !out) return fail(ctx, RT3_E_ARG, "rgba / out_pixels is NULL");
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 26)) return fail(ctx, RT3_E_ARG, "the frame must have 1 .. 2^26 pixels");
    if (const char* why = rt3dseq::refusal(*p)) return fail(ctx, RT3_E_ARG, why);
    if (prev && !(p->display.flags & RT3_DISPLAY_AUTO_EXPOSURE)) return fail(ctx, RT3_E_ARG, "prev_exposure needs RT3_DISPLAY_AUTO_EXPOSURE");
    const size_t npix = (size_t)w * h;
    const struct { const void* at; size_t bytes; } buf[4] = { { rgba, npix * sizeof(float4) }, { out, npix * sizeof(uint32_t) },
                                                              { prev, sizeof(rt3_exposure) }, { out_exposure, sizeof(rt3_exposure) } };
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++) {
            if (!buf[a].at || !buf[b].at || (a == 2 && buf[a].at == buf[b].at)) continue;      // prev == out_exposure: one record serves a sequence
            if (ranges_overlap(buf[a].at, buf[a].bytes, buf[b].at, buf[b].bytes)) return fail(ctx, RT3_E_ARG, "rgba, out_pixels and the exposure records must not overlap (prev_exposure == out_exposure apart)");
        }
    return 0;
}

extern "C" {

// Queued on the stream with no host wait, and nothing is timed: rt3_get_stats stays as it was.
//   the exposure: with auto-exposure the state zeroed, k_display_histogram and k_display_gain_step (d_prev -> d_out_exposure, the gain left in the
//   state); without it k_exposure_given if there is a d_out_exposure;
//   bloom_levels == 0: k_display_map, one launch;
//   bloom_levels == L: k_bloom_down_first, L - 1 x k_bloom_down, L - 1 x k_bloom_up, k_display_map_bloom: 2 L launches.
// The pyramid (ctx->d_bloom): pyramid_texels(w, h, L) float4 texels, D_1 .. D_L one behind the other; after the call plane 1 holds U_1.
int rt3_display_sequence_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const void* d_rgba, const rt3_display_sequence_params* p, const void* d_prev,
                                void* d_out_exposure, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = display_sequence_checks(ctx, w, h, d_rgba, p, d_prev, d_out_exposure, d_out);
    if (rc) return rc;
    if ((uintptr_t)d_rgba % 16u != 0 || (uintptr_t)d_out % 4u != 0 || (uintptr_t)d_prev % 4u != 0 || (uintptr_t)d_out_exposure % 4u != 0)
        return fail(ctx, RT3_E_ARG, "d_rgba must be 16-byte, d_out_pixels and the exposure records 4-byte aligned");
    const rt3_display_params& d = p->display;
    const bool auto_exposure = (d.flags & RT3_DISPLAY_AUTO_EXPOSURE) != 0;
    const uint32_t levels = p->bloom_levels;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    if (auto_exposure && (rc = ctx->d_display.ensure(ctx, rt3disp::kStateWords))) return rc;
    if (levels && (rc = ctx->d_bloom.ensure(ctx, pyramid_texels(w, h, levels)))) return rc;
    const DisplayLaunch L{ w * h, d.curve, d.transfer, auto_exposure, d.exposure, d.white, d_rgba, d_out, auto_exposure ? ctx->d_display.get() : nullptr };
    rt3_exposure* const out_exposure = (rt3_exposure*)d_out_exposure;
    if (auto_exposure) {
        RT3_HIP(display_histogram_launch(L, stream));
        hipLaunchKernelGGL(k_display_gain_step, dim3(1), dim3(kBins), 0, stream, L.state, d.trim_low, d.trim_high, d.exposure, d.key, (const rt3_exposure*)d_prev,
                           out_exposure, p->adapt_brighter, p->adapt_darker);
        RT3_HIP(hipGetLastError());
    } else if (out_exposure) {
        hipLaunchKernelGGL(k_exposure_given, dim3(1), dim3(64), 0, stream, out_exposure, d.exposure);
        RT3_HIP(hipGetLastError());
    }
    if (levels == 0) {
        RT3_HIP(display_map_launch(L, stream));
    } else {
        const float4* in = (const float4*)d_rgba;
        const uint32_t* state = L.state;
        float4* plane[kMaxBloomLevels];
        uint32_t pw[kMaxBloomLevels + 1] = { w }, ph[kMaxBloomLevels + 1] = { h };
        float4* next = ctx->d_bloom.get();
        for (uint32_t l = 1; l <= levels; l++) {
            pw[l] = half_of(pw[l - 1]); ph[l] = half_of(ph[l - 1]);
            plane[l - 1] = next;
            next += (size_t)pw[l] * ph[l];
        }
        const dim3 block(kSeqBlock);
        hipLaunchKernelGGL(auto_exposure ? k_bloom_down_first<true> : k_bloom_down_first<false>, dim3(seq_grid(pw[1] * ph[1])), block, 0, stream, in, pw[0], ph[0],
                           plane[0], pw[1], ph[1], d.exposure, state, p->bloom_threshold);
        RT3_HIP(hipGetLastError());
        for (uint32_t l = 2; l <= levels; l++) {
            hipLaunchKernelGGL(k_bloom_down, dim3(seq_grid(pw[l] * ph[l])), block, 0, stream, (const float4*)plane[l - 2], pw[l - 1], ph[l - 1], plane[l - 1], pw[l], ph[l]);
            RT3_HIP(hipGetLastError());
        }
        for (uint32_t l = levels - 1; l >= 1; l--) {
            hipLaunchKernelGGL(k_bloom_up, dim3(seq_grid(pw[l] * ph[l])), block, 0, stream, (const float4*)plane[l], pw[l + 1], ph[l + 1], plane[l - 1], pw[l], ph[l]);
            RT3_HIP(hipGetLastError());
        }
        const BloomMapKernel map = auto_exposure ? bloom_map_of<true>(d.curve, d.transfer) : bloom_map_of<false>(d.curve, d.transfer);
        hipLaunchKernelGGL(map, dim3(seq_grid(L.npix)), block, 0, stream, in, (uint32_t*)d_out, pw[0], ph[0], (const float4*)plane[0], pw[1], ph[1], d.exposure,
                           state, d.white, p->bloom_intensity, level_weight(levels));
        RT3_HIP(hipGetLastError());
    }
    if (auto_exposure) ctx->display_auto = true;
    if (levels) { ctx->bloom_w = w; ctx->bloom_h = h; ctx->bloom_levels = levels; }
    return leave(ctx, stream);
}

int rt3_display_sequence(rt3_ctx* ctx, uint32_t w, uint32_t h, const float* rgba, const rt3_display_sequence_params* p, const rt3_exposure* prev,
                         rt3_exposure* out_exposure, uint32_t* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = display_sequence_checks(ctx, w, h, rgba, p, prev, out_exposure, out);
    if (rc) return rc;
    if (prev && prev->level > kMaxLevel) return fail(ctx, RT3_E_ARG, "prev_exposure->level is above 511 << 19");
    const size_t npix = (size_t)w * h;
    return staged(ctx, { stage_in(rgba, npix * sizeof(float4)), stage_in(prev, sizeof(rt3_exposure)), stage_out(out_exposure, sizeof(rt3_exposure)),
                         stage_out(out, npix * sizeof(uint32_t)) },
                  [&](void* const* d) { return rt3_display_sequence_device(ctx, w, h, d[0], p, d[1], d[2], d[3], ctx->stream); });
}

// Tests only: U_1 of the last bloom call, and B = up(U_1) / levels stored at the frame's size.
int rt3_debug_display_bloom(rt3_ctx* ctx, float* out_u1, float* out_bloom, uint64_t capacity_pixels, uint32_t* w_out, uint32_t* h_out) {
    if (!ctx) return RT3_E_ARG;
    if (!w_out || !h_out) return fail(ctx, RT3_E_ARG, "w / h is NULL");
    if (ctx->bloom_levels == 0) return fail(ctx, RT3_E_STATE, "no rt3_display_sequence call with bloom_levels >= 1 on this context");
    const uint32_t w = ctx->bloom_w, h = ctx->bloom_h, w1 = half_of(w), h1 = half_of(h);
    const size_t npix = (size_t)w * h;
    *w_out = w; *h_out = h;
    if (capacity_pixels < npix) return fail(ctx, RT3_E_ARG, "capacity_pixels is smaller than the frame of the last bloom call");
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, nullptr, &stream))) return rc;            // behind the call that wrote the pyramid, whatever stream it ran on
    if (out_u1) RT3_HIP(hipMemcpyAsync(out_u1, ctx->d_bloom.get(), (size_t)w1 * h1 * sizeof(float4), hipMemcpyDeviceToHost, stream));
    if (out_bloom) {
        if ((rc = ctx->d_bloom_plane.ensure(ctx, npix))) return rc;
        hipLaunchKernelGGL(k_bloom_plane, dim3(seq_grid(w * h)), dim3(kSeqBlock), 0, stream, (const float4*)ctx->d_bloom.get(), w1, h1, ctx->d_bloom_plane.get(), w, h,
                           level_weight(ctx->bloom_levels));
        RT3_HIP(hipGetLastError());
        RT3_HIP(hipMemcpyAsync(out_bloom, ctx->d_bloom_plane.get(), npix * sizeof(float4), hipMemcpyDeviceToHost, stream));
    }
    if ((rc = leave(ctx, stream))) return rc;
    RT3_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
