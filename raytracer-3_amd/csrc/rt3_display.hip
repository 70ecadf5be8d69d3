// rt3_display.hip — the display transform (rt3_display*): a linear float frame to RGBA8 words — exposure (given, or from the
// frame's trimmed log-average luminance), a tone curve, a transfer function.  A streaming pass: 16 bytes in and 4 out per pixel, 16 more in with
// auto-exposure.  The law itself is rt3_display_law.hpp, shared with the host restatement; the auto-exposure adds up integers only (LDS and global
// integer atomics), so the gain does not depend on the order the pixels arrive in and tests/display_ref.py reproduces every word.
// A translation unit of its own (gfx950 only), as rt3_denoise.hip is: the kernels share nothing with the render path.  The entry points are below
// the kernels: they check the arguments, take the state from the context (rt3_ctx.hpp) and launch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rt3_ctx.hpp"
#include "rt3_display_law.hpp"
#include "rt3_display.hpp"

static_assert(sizeof(rt3_display_params) == 32, "rt3.h: rt3_display_params");

namespace {

using namespace rt3disp;

constexpr uint32_t kDispBlock = 256;
constexpr uint32_t kDispMaxGrid = 2048;                             // a memory-bound pass: 256 CUs x 8 blocks, the rest by the grid-stride loop
constexpr uint32_t kHistBlock = 1024, kHistMaxGrid = 256, kHistLoads = 2;      // k_display_histogram: 2^19 pixels per turn of its loop
constexpr uint32_t kDarkSlot = kBins, kCountSlot = kBins + 1, kGainSlot = kBins + 2;      // the state's words behind the histogram

uint32_t display_grid(uint32_t npix) {
    const uint32_t want = (npix + kDispBlock - 1) / kDispBlock;
    return want < kDispMaxGrid ? want : kDispMaxGrid;
}

// Every pixel's bin, counted in LDS; each block then adds its non-zero bins to the context's histogram.  Integer atomics only.  Few large blocks —
// one of 1024 threads per CU at most, two loads in flight per thread: every block ends with up to 513 global atomics on the same 513 words, and with
// the map's grid of 2048 blocks those serialised adds made a call about 30 us longer whatever the frame's size (measured: DESIGN.md 5.2q).
__global__ __launch_bounds__(kHistBlock) void k_display_histogram(const float4* __restrict__ in, uint32_t npix, uint32_t* __restrict__ state) {
    __shared__ uint32_t s_hist[kBins + 1];                          // [kBins]: the dark pixels
    for (uint32_t j = threadIdx.x; j <= kBins; j += kHistBlock) s_hist[j] = 0u;
    __syncthreads();
    const uint32_t stride = gridDim.x * kHistBlock;                 // npix + kHistLoads * stride <= 2^26 + 2^19: no wrap
    for (uint32_t i = blockIdx.x * kHistBlock + threadIdx.x; i < npix; i += kHistLoads * stride) {
        float4 c[kHistLoads];
#pragma unroll
        for (uint32_t u = 0; u < kHistLoads; u++)
            if (i + u * stride < npix) c[u] = in[i + u * stride];
#pragma unroll
        for (uint32_t u = 0; u < kHistLoads; u++) {
            if (i + u * stride >= npix) continue;
            const uint32_t b = bin(c[u].x, c[u].y, c[u].z);
            atomicAdd(&s_hist[b == kDark ? kDarkSlot : b], 1u);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j <= kBins; j += kHistBlock) {
        const uint32_t v = s_hist[j];
        if (v != 0u) atomicAdd(&state[j], v);
    }
}

// One block of kBins threads, one bin each: the ranks by an inclusive scan, the trim, S by a tree sum (integers: any order gives the same S), then
// thread 0 divides and leaves n and the gain behind the histogram.
__global__ __launch_bounds__(kBins) void k_display_gain(uint32_t* __restrict__ state, uint32_t trim_low, uint32_t trim_high, float exposure, float key) {
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
    if (n == 0) {                                                   // (the whole block: nothing waits behind this)
        if (k == 0) { state[kCountSlot] = 0u; state[kGainSlot] = bits_of(exposure); }
        return;
    }
    const Trim t = trim_of(n, trim_low, trim_high);
    s_sum[k] = kept(t, begin, end) * k;
    __syncthreads();
    for (uint32_t off = kBins / 2; off > 0; off >>= 1) {
        if (k < off) s_sum[k] += s_sum[k + off];
        __syncthreads();
    }
    if (k == 0) { state[kCountSlot] = (uint32_t)n; state[kGainSlot] = bits_of(gain_from_sum(t, s_sum[0], exposure, key)); }
}

// The gain (uniform, or the float k_display_gain left), the curve, the transfer, the word.  SRGB: the table is staged in LDS, 16 bytes per thread.
template <uint32_t CURVE, uint32_t TRANSFER, bool AUTO>
__global__ __launch_bounds__(kDispBlock) void k_display_map(const float4* __restrict__ in, uint32_t* __restrict__ out, uint32_t npix, float exposure,
                                                           const uint32_t* __restrict__ state, float white) {
    __shared__ __attribute__((aligned(16))) uint8_t s_table[TRANSFER == RT3_DISPLAY_SRGB ? 4096 : 16];
    if (TRANSFER == RT3_DISPLAY_SRGB) {
        static_assert(kDispBlock * 16 == sizeof(kSrgbTable), "one uint4 of the table per thread");
        reinterpret_cast<uint4*>(s_table)[threadIdx.x] = reinterpret_cast<const uint4*>(kSrgbTable)[threadIdx.x];
        __syncthreads();
    }
    const float gain = AUTO ? float_of(state[kGainSlot]) : exposure;
    const uint32_t stride = gridDim.x * kDispBlock;
    for (uint32_t i = blockIdx.x * kDispBlock + threadIdx.x; i < npix; i += stride) {
        const float4 c = in[i];
        out[i] = pixel(c.x, c.y, c.z, gain, CURVE, TRANSFER, white, s_table);
    }
}

using MapKernel = void (*)(const float4*, uint32_t*, uint32_t, float, const uint32_t*, float);
template <uint32_t CURVE, bool AUTO>
MapKernel map_of(uint32_t transfer) {
    return transfer == RT3_DISPLAY_LINEAR ? k_display_map<CURVE, RT3_DISPLAY_LINEAR, AUTO>
         : transfer == RT3_DISPLAY_GAMMA2 ? k_display_map<CURVE, RT3_DISPLAY_GAMMA2, AUTO> : k_display_map<CURVE, RT3_DISPLAY_SRGB, AUTO>;
}
template <bool AUTO>
MapKernel map_of(uint32_t curve, uint32_t transfer) {
    return curve == RT3_DISPLAY_CLAMP ? map_of<RT3_DISPLAY_CLAMP, AUTO>(transfer)
         : curve == RT3_DISPLAY_REINHARD ? map_of<RT3_DISPLAY_REINHARD, AUTO>(transfer) : map_of<RT3_DISPLAY_FILMIC, AUTO>(transfer);
}

}  // namespace

hipError_t display_histogram_launch(const DisplayLaunch& L, hipStream_t stream) {
    // zeroed at the start of the call, not at its end: rt3_debug_display_state reads what the call left
    const hipError_t e = hipMemsetAsync(L.state, 0, kStateWords * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t per_block = kHistBlock * kHistLoads, want = (L.npix + per_block - 1) / per_block;
    hipLaunchKernelGGL(k_display_histogram, dim3(want < kHistMaxGrid ? want : kHistMaxGrid), dim3(kHistBlock), 0, stream, (const float4*)L.rgba, L.npix,
                       L.state);
    return hipGetLastError();
}

hipError_t display_map_launch(const DisplayLaunch& L, hipStream_t stream) {
    const MapKernel map = L.auto_exposure ? map_of<true>(L.curve, L.transfer) : map_of<false>(L.curve, L.transfer);
    hipLaunchKernelGGL(map, dim3(display_grid(L.npix)), dim3(kDispBlock), 0, stream, (const float4*)L.rgba, (uint32_t*)L.out, L.npix, L.exposure,
                       (const uint32_t*)L.state, L.white);
    return hipGetLastError();
}

// ---- The entry points (rt3.h)
static int display_checks(rt3_ctx* ctx, uint32_t w, uint32_t h, const void* rgba, const rt3_display_params* p, const void* out) {
    if (!p) return fail(ctx, RT3_E_ARG, "p is NULL");
    if (!rgba || !out) return fail(ctx, RT3_E_ARG, "rgba / out_pixels is NULL");
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 26)) return fail(ctx, RT3_E_ARG, "the frame must have 1 .. 2^26 pixels");
    if (const char* why = rt3disp::refusal(*p)) return fail(ctx, RT3_E_ARG, why);
    const size_t npix = (size_t)w * h;
    if (ranges_overlap(out, npix * sizeof(uint32_t), rgba, npix * sizeof(float4))) return fail(ctx, RT3_E_ARG, "out_pixels overlaps rgba");
    return 0;
}

extern "C" {

// Without the flag one launch, k_display_map with the uniform gain; with it the state zeroed on the stream, k_display_histogram, k_display_gain and
// k_display_map reading the gain where k_display_gain left it.  Nothing here waits for the device, and nothing is timed: rt3_get_stats stays as it was.
int rt3_display_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const void* d_rgba, const rt3_display_params* p, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = display_checks(ctx, w, h, d_rgba, p, d_out);
    if (rc) return rc;
    if ((uintptr_t)d_rgba % 16u != 0 || (uintptr_t)d_out % 4u != 0) return fail(ctx, RT3_E_ARG, "d_rgba must be 16-byte and d_out_pixels 4-byte aligned");
    const bool auto_exposure = (p->flags & RT3_DISPLAY_AUTO_EXPOSURE) != 0;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    if (auto_exposure && (rc = ctx->d_display.ensure(ctx, kStateWords))) return rc;      // (the state is the context's: the first such call allocates it)
    const DisplayLaunch L{ w * h, p->curve, p->transfer, auto_exposure, p->exposure, p->white, d_rgba, d_out, auto_exposure ? ctx->d_display.get() : nullptr };
    if (auto_exposure) {
        RT3_HIP(display_histogram_launch(L, stream));
        hipLaunchKernelGGL(k_display_gain, dim3(1), dim3(kBins), 0, stream, L.state, p->trim_low, p->trim_high, p->exposure, p->key);
        RT3_HIP(hipGetLastError());
    }
    RT3_HIP(display_map_launch(L, stream));
    if (auto_exposure) ctx->display_auto = true;
    return leave(ctx, stream);
}

int rt3_display(rt3_ctx* ctx, uint32_t w, uint32_t h, const float* rgba, const rt3_display_params* p, uint32_t* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = display_checks(ctx, w, h, rgba, p, out);
    if (rc) return rc;
    const size_t npix = (size_t)w * h;
    return staged(ctx, { stage_in(rgba, npix * sizeof(float4)), stage_out(out, npix * sizeof(uint32_t)) },
                  [&](void* const* d) { return rt3_display_device(ctx, w, h, d[0], p, d[1], ctx->stream); });
}

int rt3_debug_display_state(rt3_ctx* ctx, uint32_t hist[512], uint32_t* dark, float* gain) {
    if (!ctx) return RT3_E_ARG;
    if (!ctx->display_auto) return fail(ctx, RT3_E_STATE, "no call with RT3_DISPLAY_AUTO_EXPOSURE on this context");
    uint32_t state[kStateWords];
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, nullptr, &stream))) return rc;            // behind the call that wrote the state, whatever stream it ran on
    RT3_HIP(hipMemcpyAsync(state, ctx->d_display.get(), sizeof state, hipMemcpyDeviceToHost, stream));
    if ((rc = leave(ctx, stream))) return rc;
    RT3_HIP(hipStreamSynchronize(stream));
    if (hist) std::memcpy(hist, state, kBins * sizeof(uint32_t));
    if (dark) *dark = state[kDarkSlot];
    if (gain) *gain = float_of(state[kGainSlot]);
    return 0;
}

}  // extern "C"
