// rt3_denoise.hip — the AOV-guided edge-avoiding a-trous denoiser (rt3_denoise*): the spatial part of SVGF (Schied et
// al. 2017) over the demodulated irradiance, built on the a-trous wavelet filter of Dammertz et al. 2010.  One call runs k_denoise_prepare,
// k_denoise_moments, then k_denoise_atrous once per pass; the last pass remodulates into the caller's frame.  Every sum runs in the tap order
// of DESIGN.md 4.11 with no contraction (the library builds with -ffp-contract=off), so tests/denoise_ref.py restates it in numpy.
// A translation unit of its own (gfx950 only): the kernels share nothing with the render path, and compiled apart they add about 2 s to the
// build instead of about 14 s inside rt3_device.hip.  rt3_device.hip checks the arguments, owns the scratch and calls denoise_launch().
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt3_denoise.hpp"

namespace {

constexpr int kDnTile = 16;                 // 16 x 16 pixel tiles (a wave covers 16 x 4): neighbouring taps of a wave share cache lines

// What every denoiser kernel reads besides its own planes.
struct DenoiseArgs {
    uint32_t width, height, tiles_x;
    uint32_t squarings;                     // log2(normal_power)
    float sigma_l, sigma_z;
    const float4* __restrict__ guide;       // per pixel (normal.xyz, depth)
    const float* __restrict__ gz;           // per pixel depth slope
};

// The pixel of this thread; false outside the frame.
__device__ __forceinline__ bool dn_pixel(const DenoiseArgs& D, int& x, int& y) {
    const uint32_t ty = blockIdx.x / D.tiles_x, tx = blockIdx.x - ty * D.tiles_x;
    x = (int)(tx * kDnTile + threadIdx.x);
    y = (int)(ty * kDnTile + threadIdx.y);
    return x < (int)D.width && y < (int)D.height;
}

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ float dn_demod(float c, float a) { return a > 0x1p-10f ? c / a : c; }

// exp(x) for the weights, written out in plain f32 steps so that the numpy restatement computes the same bits (tests/denoise_ref.py):
// x = k ln2 + r (k = rint(x log2 e), ln2 split so that k ln2_hi is exact), a degree-7 Taylor polynomial of exp(r) in Horner form with
// separate multiplies and adds, then ldexp.  About 2 ulp.  A library expf would do as well numerically, but its last bit differs from any
// host exp, and the filter amplifies such differences at ill-conditioned pixels far beyond a relative 1e-5.
__device__ __forceinline__ float dn_exp(float x) {
    if (x < -104.0f) return 0.0f;                                   // (also -inf); exp(-104) is below half the least denormal
    const float k = __builtin_rintf(x * 1.44269502f);
    const float r = (x - k * 0.693145751953125f) - k * 1.42860677e-6f;
    float p = 1.98412701e-4f;                                       // 1/5040, then 1/720 ... 1/1 (float-rounded)
    p = p * r + 1.38888892e-3f;
    p = p * r + 8.33333377e-3f;
    p = p * r + 4.16666679e-2f;
    p = p * r + 0.166666672f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return __builtin_ldexpf(p, (int)k);
}

// w_n of a pair: 1 when both normals are exactly zero, else max(0, n_p . n_q)^P by log2(P) squarings.
__device__ __forceinline__ float dn_wn(const DenoiseArgs& D, const float4& gp, const float4& gq) {
    if (gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f && gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f) return 1.0f;
    float w = fmaxf(0.0f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
    for (uint32_t i = 0; i < D.squarings; i++) w = w * w;
    return w;
}

// e_z of a pair whose depths are both finite or both infinite, at pixel distance d.
__device__ __forceinline__ float dn_ez(const DenoiseArgs& D, float zp, float zq, float gzp, float d) {
    return __builtin_isinf(zp) ? 0.0f : __builtin_fabsf(zp - zq) / (D.sigma_z * gzp * d + 1e-10f);
}

// w_g of a pair (p, q), q != p: 0 when exactly one depth is infinite.
__device__ __forceinline__ float dn_wg(const DenoiseArgs& D, const float4& gp, const float4& gq, float gzp, float d) {
    if (__builtin_isinf(gp.w) != __builtin_isinf(gq.w)) return 0.0f;
    return dn_wn(D, gp, gq) * dn_exp(-dn_ez(D, gp.w, gq.w, gzp, d));
}

// colour (r, g, b, .) and rt3_aov records (3 float4 each) -> il = (I.rgb, L(I)), guide = (normal, depth), gz = the depth slope.
__global__ __launch_bounds__(kDnTile * kDnTile) void k_denoise_prepare(const DenoiseArgs D, const float4* __restrict__ colour,
                                                                      const float4* __restrict__ aov, float4* __restrict__ il,
                                                                      float4* __restrict__ guide, float* __restrict__ gz) {
    int x, y;
    if (!dn_pixel(D, x, y)) return;
    const int W = (int)D.width, H = (int)D.height;
    const uint32_t p = (uint32_t)(y * W + x);
    const float4 c = colour[p], a = aov[3 * (size_t)p], n = aov[3 * (size_t)p + 1];
    const float ir = dn_demod(c.x, a.x), ig = dn_demod(c.y, a.y), ib = dn_demod(c.z, a.z);
    il[p] = make_float4(ir, ig, ib, dn_lum(ir, ig, ib));
    guide[p] = n;
    float g = 0.0f;
    if (!__builtin_isinf(n.w)) {
        const int nx[4] = { x - 1, x + 1, x, x }, ny[4] = { y, y, y - 1, y + 1 };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (nx[k] < 0 || nx[k] >= W || ny[k] < 0 || ny[k] >= H) continue;
            const float zq = aov[3 * (size_t)(ny[k] * W + nx[k]) + 1].w;
            if (!__builtin_isinf(zq)) g = fmaxf(g, __builtin_fabsf(zq - n.w));
        }
    }
    gz[p] = g;
}

// The spatial variance estimate: il (I, L) -> iv (I, v), v from the w_g-weighted moments of L over the 7 x 7 window.
__global__ __launch_bounds__(kDnTile * kDnTile) void k_denoise_moments(const DenoiseArgs D, const float4* __restrict__ il,
                                                                      float4* __restrict__ iv) {
    int x, y;
    if (!dn_pixel(D, x, y)) return;
    const int W = (int)D.width, H = (int)D.height;
    const uint32_t p = (uint32_t)(y * W + x);
    const float4 gp = D.guide[p];
    const float gzp = D.gz[p];
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -3; dx <= 3; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const uint32_t q = (uint32_t)(qy * W + qx);
            const float L = il[q].w;
            const int ady = dy < 0 ? -dy : dy, adx = dx < 0 ? -dx : dx;
            const float w = (dx == 0 && dy == 0) ? 1.0f : dn_wg(D, gp, D.guide[q], gzp, (float)(adx > ady ? adx : ady));
            sw = sw + w;
            s1 = s1 + w * L;
            s2 = s2 + w * (L * L);
        }
    }
    const float m1 = s1 / sw, m2 = s2 / sw;
    const float4 c = il[p];
    iv[p] = make_float4(c.x, c.y, c.z, fmaxf(0.0f, m2 - m1 * m1));
}

// One a-trous pass at step `step` over (I, v): the edge-stopped 3 x 3 blur of v, then the 25 taps.  LAST: remodulate with the albedo of
// the rt3_aov records and write (r, g, b, 0) to the caller's frame instead of (I', v').
template <bool LAST>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_denoise_atrous(const DenoiseArgs D, const float4* __restrict__ in,
                                                                     float4* __restrict__ out, int step, const float4* __restrict__ aov) {
    int x, y;
    if (!dn_pixel(D, x, y)) return;
    const int W = (int)D.width, H = (int)D.height;
    const uint32_t p = (uint32_t)(y * W + x);
    const float4 gp = D.guide[p], cp = in[p];
    const float gzp = D.gz[p];
    const bool pinf = __builtin_isinf(gp.w);

    const float k1[3] = { 0.25f, 0.5f, 0.25f };
    float gn = 0.0f, gd = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const uint32_t q = (uint32_t)(qy * W + qx);
            const float k = k1[dy + 1] * k1[dx + 1];
            const float w = (dx == 0 && dy == 0) ? k : k * dn_wg(D, gp, D.guide[q], gzp, 1.0f);
            gd = gd + w;
            gn = gn + w * in[q].w;
        }
    }
    const float sig = D.sigma_l * __builtin_sqrtf(gn / gd) + 1e-10f;
    const float lp = dn_lum(cp.x, cp.y, cp.z);

    const float h1[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= W) continue;
            const float h = h1[dy + 2] * h1[dx + 2];
            float w;
            float4 c;
            if (dx == 0 && dy == 0) {
                w = h;
                c = cp;
            } else {
                const uint32_t q = (uint32_t)(qy * W + qx);
                const float4 gq = D.guide[q];
                if (pinf != __builtin_isinf(gq.w)) continue;                       // w = 0: nothing of q is read
                const int ady = dy < 0 ? -dy : dy, adx = dx < 0 ? -dx : dx;
                const float ez = dn_ez(D, gp.w, gq.w, gzp, (float)(step * (adx > ady ? adx : ady)));
                const float wn = dn_wn(D, gp, gq);
                c = in[q];
                const float el = __builtin_fabsf(lp - dn_lum(c.x, c.y, c.z)) / sig;
                w = h * wn * dn_exp(-(ez + el));
            }
            sw = sw + w;
            sr = sr + w * c.x;
            sg = sg + w * c.y;
            sb = sb + w * c.z;
            sv = sv + (w * w) * c.w;
        }
    }
    const float ir = sr / sw, ig = sg / sw, ib = sb / sw;
    if (LAST) {
        const float4 a = aov[3 * (size_t)p];
        out[p] = make_float4(a.x > 0x1p-10f ? ir * a.x : ir, a.y > 0x1p-10f ? ig * a.y : ig, a.z > 0x1p-10f ? ib * a.z : ib, 0.0f);
    } else {
        out[p] = make_float4(ir, ig, ib, sv / (sw * sw));
    }
}

}  // namespace

hipError_t denoise_launch(const DenoiseLaunch& L, hipStream_t stream) {
    const uint32_t w = L.width, h = L.height;
    const size_t npix = (size_t)w * h;
    float4* const pa = L.scratch;
    float4* const pb = pa + npix;
    float4* const guide = pb + npix;
    float* const gz = reinterpret_cast<float*>(guide + npix);
    DenoiseArgs D;
    D.width = w; D.height = h;
    D.tiles_x = (w + kDnTile - 1) / kDnTile;
    D.squarings = 0;
    while ((1u << D.squarings) < L.normal_power) D.squarings++;
    D.sigma_l = L.sigma_l; D.sigma_z = L.sigma_z;
    D.guide = guide; D.gz = gz;
    const dim3 grid(D.tiles_x * ((h + kDnTile - 1) / kDnTile)), block(kDnTile, kDnTile);
    const float4* aov = (const float4*)L.aov;
    hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, stream, D, (const float4*)L.colour, aov, pa, guide, gz);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_denoise_moments, grid, block, 0, stream, D, (const float4*)pa, pb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    float4* src = pb;
    float4* dst = pa;
    for (uint32_t i = 0; i < L.iterations; i++) {
        if (i + 1 == L.iterations) hipLaunchKernelGGL(k_denoise_atrous<true>, grid, block, 0, stream, D, (const float4*)src, (float4*)L.out, 1 << i, aov);
        else hipLaunchKernelGGL(k_denoise_atrous<false>, grid, block, 0, stream, D, (const float4*)src, dst, 1 << i, aov);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        float4* t = src; src = dst; dst = t;
    }
    return hipSuccess;
}
