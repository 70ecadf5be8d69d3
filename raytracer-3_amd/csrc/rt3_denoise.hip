// rt3_denoise.hip — the AOV-guided edge-avoiding a-trous denoiser (rt3_denoise*): the spatial part of SVGF (Schied et
// al. 2017) over the demodulated irradiance, built on the a-trous wavelet filter of Dammertz et al. 2010.  One call runs k_denoise_prepare,
// k_denoise_moments, then k_denoise_atrous once per pass; the last pass remodulates into the caller's frame.  Every sum runs in the tap order
// of DESIGN.md 4.11 with no contraction (the library builds with -ffp-contract=off), so tests/denoise_ref.py restates it in numpy.
// A translation unit of its own (gfx950 only): the kernels share nothing with the render path, and compiled apart they add about 2 s to the
// build instead of about 14 s inside rt3_device.hip.  The entry points are below the kernels: they check the arguments, take the scratch from the
// context (rt3_ctx.hpp) and launch.
// k_temporal_reproject and k_motion take the view as a template parameter: the pinhole camera, or a lens model whose law is rt3_lens_law.hpp's
// (DESIGN.md 4.24, 5.2s).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>

#include "rt3_ctx.hpp"
#include "rt3_lens_law.hpp"

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

// The spatial variance estimate: il (I, L) -> iv (I, v), v from the w_g-weighted moments of L over the 7 x 7 window.  TEMPORAL (DESIGN.md
// 4.12 step 6): where the history record's length is at least 4, v = max(0, M2 - M1 * M1) of its moments instead.
template <bool TEMPORAL>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_denoise_moments(const DenoiseArgs D, const float4* __restrict__ il,
                                                                      float4* __restrict__ iv, const float4* __restrict__ hist) {
    int x, y;
    if (!dn_pixel(D, x, y)) return;
    const int W = (int)D.width, H = (int)D.height;
    const uint32_t p = (uint32_t)(y * W + x);
    if (TEMPORAL && hist[3 * (size_t)p].w >= 4.0f) {
        const float4 m = hist[3 * (size_t)p + 1], c = il[p];
        iv[p] = make_float4(c.x, c.y, c.z, fmaxf(0.0f, m.y - m.x * m.x));
        return;
    }
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
// the rt3_aov records and write (r, g, b, 0) to the caller's frame instead of (I', v').  HIST (pass 0 of the temporal call): also write
// (I'.rgb, length) to the first float4 of the pixel's history record, whose length k_temporal_reproject left there.
template <bool LAST, bool HIST>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_denoise_atrous(const DenoiseArgs D, const float4* __restrict__ in,
                                                                     float4* __restrict__ out, int step, const float4* __restrict__ aov,
                                                                     float4* __restrict__ hist) {
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
    if (HIST) hist[3 * (size_t)p] = make_float4(ir, ig, ib, hist[3 * (size_t)p].w);
    if (LAST) {
        const float4 a = aov[3 * (size_t)p];
        out[p] = make_float4(a.x > 0x1p-10f ? ir * a.x : ir, a.y > 0x1p-10f ? ig * a.y : ig, a.z > 0x1p-10f ? ib * a.z : ib, 0.0f);
    } else {
        out[p] = make_float4(ir, ig, ib, sv / (sw * sw));
    }
}

// The view a frame was rendered through, a compile-time choice of k_temporal_reproject and k_motion: the pinhole camera, or one of the lens
// models (RT3_LENS_*).  The model is the same for every pixel of a launch, so it is a template parameter, not a per-lane switch.
constexpr uint32_t kViewCamera = 0;

// The camera's part of k_temporal_reproject's arguments: this frame's camera and the previous camera's constants.
struct CameraReproject {
    float ox, oy, oz, hx, hy, hz, vx, vy, vz, lx, ly, lz;      // this frame's camera
    float pox, poy, poz, plx, ply, plz;                        // o' and L = llc' - o'
    float nx, ny, nz, aux, auy, auz, avx, avy, avz, ln;        // n = h x v, a_u, a_v, L . n
};
// The camera's part of k_motion's arguments: this frame's camera.
struct CameraRays { float ox, oy, oz, hx, hy, hz, vx, vy, vz, lx, ly, lz; };
// A lens frame's part of either: this frame's lens, the previous one (k_motion does not read it), the frame, and whether the two
// lenses are equal in every bit the inverse law reads.
struct LensArgs { rt3_lens lens, prev; uint32_t width, height, same; };

// What k_temporal_reproject reads besides DenoiseArgs: the view, then the parameters.
template <class View>
struct TemporalArgs {
    View view;
    uint32_t has_prev, same_cam;
    float alpha, moments_alpha, depth_tolerance, normal_tolerance;
};
template <uint32_t VIEW> using TemporalArgsOf = TemporalArgs<std::conditional_t<VIEW == kViewCamera, CameraReproject, LensArgs>>;

__device__ __forceinline__ float dn_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// DESIGN.md 4.12 steps 1-5 (in place of k_denoise_prepare): colour, rt3_aov records and the previous history -> il = (I.rgb, L(I)) of the
// blended I, the guide and gz planes as k_denoise_prepare writes them, and the history record of the pixel with (I, length) in its first
// float4 (pass 0 replaces I), (M1, M2, depth, 0) and (normal, 0).  MOTION: a pixel that hit and whose motion record
// (m, moved) has moved != 0 adds m to its world point and is projected even under a byte-equal camera; every other pixel takes the
// operations of the MOTION = false kernel.  VIEW: kViewCamera, or the lens model of both lenses: steps 2 and 3 are then the
// lens's centre ray and rt3lens::project, and step 4 wraps an equirectangular frame's columns and keeps a cube frame's taps on the face.
template <uint32_t VIEW, bool MOTION>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_temporal_reproject(const DenoiseArgs D, const TemporalArgsOf<VIEW> T,
                                                                         const float4* __restrict__ colour, const float4* __restrict__ aov,
                                                                         const float4* __restrict__ prev, float4* __restrict__ il,
                                                                         float4* __restrict__ guide, float* __restrict__ gz,
                                                                         float4* __restrict__ hist, const float4* __restrict__ motion) {
    int x, y;
    if (!dn_pixel(D, x, y)) return;
    const int W = (int)D.width, H = (int)D.height;
    const uint32_t p = (uint32_t)(y * W + x);
    // 1: demodulate, guides and depth slope exactly as k_denoise_prepare
    const float4 c = colour[p], a = aov[3 * (size_t)p], n = aov[3 * (size_t)p + 1];
    const float ir = dn_demod(c.x, a.x), ig = dn_demod(c.y, a.y), ib = dn_demod(c.z, a.z);
    const float lc = dn_lum(ir, ig, ib);
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

    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f, nmin = __builtin_inff();
    if (T.has_prev) {
        const bool hit = !__builtin_isinf(n.w);
        float rx, ry, rz, xp, yp;
        bool ok = true;
        uint32_t face = 0;                                          // RT3_LENS_CUBE: the face the taps stay on
        if constexpr (VIEW == kViewCamera) {
            const CameraReproject& V = T.view;
            // 2: the world point of the pixel-centre ray, relative to the previous origin (the sky: the direction)
            const float u = (float)x / ((float)W - 1.0f), v = (float)(H - 1 - y) / ((float)H - 1.0f);
            const float dx = ((V.lx + u * V.hx) + v * V.vx) - V.ox;
            const float dy = ((V.ly + u * V.hy) + v * V.vy) - V.oy;
            const float dz = ((V.lz + u * V.hz) + v * V.vz) - V.oz;
            const float inv = 1.0f / __builtin_sqrtf(dn_dot(dx, dy, dz, dx, dy, dz));
            const float ux = dx * inv, uy = dy * inv, uz = dz * inv;
            rx = hit ? (V.ox + n.w * ux) - V.pox : ux;
            ry = hit ? (V.oy + n.w * uy) - V.poy : uy;
            rz = hit ? (V.oz + n.w * uz) - V.poz : uz;
            bool moved = false;
            if (MOTION && hit) {
                const float4 m = motion[p];
                moved = m.w != 0.0f;
                if (moved) {
                    rx = ((V.ox + n.w * ux) + m.x) - V.pox;
                    ry = ((V.oy + n.w * uy) + m.y) - V.poy;
                    rz = ((V.oz + n.w * uz) + m.z) - V.poz;
                }
            }
            // 3: project into the previous camera (skipped for a byte-equal camera: every pixel that has not moved maps to itself)
            xp = (float)x; yp = (float)y;
            if (!T.same_cam || moved) {
                const float sc = V.ln / dn_dot(rx, ry, rz, V.nx, V.ny, V.nz);
                ok = __builtin_isfinite(sc) && sc > 0.0f;
                const float px = sc * rx - V.plx, py = sc * ry - V.ply, pz = sc * rz - V.plz;
                xp = dn_dot(px, py, pz, V.aux, V.auy, V.auz) * ((float)W - 1.0f);
                yp = ((float)H - 1.0f) - dn_dot(px, py, pz, V.avx, V.avy, V.avz) * ((float)H - 1.0f);
            }
        } else {
            const LensArgs& V = T.view;
            // 2 (4.24): the shown point on the lens's centre ray (spp 1: no jitter), relative to the previous origin (a miss: the direction)
            const rt3lens::Frame F{ V.width, V.height, 1u, 0u, 0u };
            float o[3], d[3];
            rt3lens::ray<VIEW>(V.lens, F, (uint32_t)x, (uint32_t)y, 0u, o, d);
            rx = hit ? (o[0] + n.w * d[0]) - V.prev.origin[0] : d[0];
            ry = hit ? (o[1] + n.w * d[1]) - V.prev.origin[1] : d[1];
            rz = hit ? (o[2] + n.w * d[2]) - V.prev.origin[2] : d[2];
            bool moved = false;
            if (MOTION && hit) {
                const float4 m = motion[p];
                moved = m.w != 0.0f;
                if (moved) {
                    rx = ((o[0] + n.w * d[0]) + m.x) - V.prev.origin[0];
                    ry = ((o[1] + n.w * d[1]) + m.y) - V.prev.origin[1];
                    rz = ((o[2] + n.w * d[2]) + m.z) - V.prev.origin[2];
                }
            }
            // 3 (4.24): the inverse law of the previous lens (skipped for an equal lens and a pixel that has not moved, and for an orthographic
            // miss, whose direction says nothing about where it was)
            xp = (float)x; yp = (float)y;
            if (VIEW == RT3_LENS_CUBE) face = (uint32_t)y / V.width;
            if ((!V.same || moved) && !(VIEW == RT3_LENS_ORTHO && !hit)) {
                const float r[3] = { rx, ry, rz };
                float zunused;
                ok = rt3lens::project<VIEW>(V.prev, V.width, V.height, r, xp, yp, zunused, face);
            }
        }
        // 4: the bilinear taps that lie in the frame and are consistent (no tap can when x' or y' is outside (-1, W) x (-1, H), or NaN)
        if (ok && xp > -1.0f && xp < (float)W && yp > -1.0f && yp < (float)H) {
            float zhat;
            if constexpr (VIEW == RT3_LENS_ORTHO) zhat = dn_dot(rx, ry, rz, T.view.prev.forward[0], T.view.prev.forward[1], T.view.prev.forward[2]);
            else zhat = __builtin_sqrtf(dn_dot(rx, ry, rz, rx, ry, rz));
            const float bound = T.depth_tolerance * (g + 1e-3f * zhat);
            const float x0 = __builtin_floorf(xp), y0 = __builtin_floorf(yp);
            const float fx = xp - x0, fy = yp - y0;
            const int ix = (int)x0, iy = (int)y0;
            const float wt[4] = { (1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int qx = ix + (k & 1);
                const int qy = iy + (k >> 1);
                if (VIEW == RT3_LENS_EQUIRECT) qx = qx < 0 ? qx + W : qx >= W ? qx - W : qx;           // the columns wrap: -1 -> W - 1, W -> 0
                if (VIEW == RT3_LENS_CUBE && (qy < (int)(face * (uint32_t)W) || qy >= (int)((face + 1u) * (uint32_t)W))) continue;   // no tap across faces
                if (wt[k] == 0.0f || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                const size_t q = 3 * (size_t)(qy * W + qx);
                const float4 hm = prev[q + 1], hn = prev[q + 2];
                bool consistent;
                if (!hit || __builtin_isinf(hm.z)) consistent = !hit && __builtin_isinf(hm.z);
                else consistent = __builtin_fabsf(hm.z - zhat) <= bound && dn_dot(n.x, n.y, n.z, hn.x, hn.y, hn.z) >= T.normal_tolerance;
                if (!consistent) continue;
                const float4 hc = prev[q];
                const float w = wt[k];
                sw = sw + w;
                sr = sr + w * hc.x;
                sg = sg + w * hc.y;
                sb = sb + w * hc.z;
                s1 = s1 + w * hm.x;
                s2 = s2 + w * hm.y;
                nmin = fminf(nmin, hc.w);
            }
        }
    }
    // 5: blend, or start afresh
    float4 o;
    float len, m1, m2;
    if (sw >= 0.01f) {
        len = fminf(nmin + 1.0f, 65535.0f);
        const float a1 = fmaxf(T.alpha, 1.0f / len), a2 = fmaxf(T.moments_alpha, 1.0f / len);
        const float r = (1.0f - a1) * (sr / sw) + a1 * ir, gg = (1.0f - a1) * (sg / sw) + a1 * ig, b = (1.0f - a1) * (sb / sw) + a1 * ib;
        o = make_float4(r, gg, b, dn_lum(r, gg, b));
        m1 = (1.0f - a2) * (s1 / sw) + a2 * lc;
        m2 = (1.0f - a2) * (s2 / sw) + a2 * (lc * lc);
    } else {
        len = 1.0f;
        o = make_float4(ir, ig, ib, lc);
        m1 = lc;
        m2 = lc * lc;
    }
    il[p] = o;
    hist[3 * (size_t)p] = make_float4(o.x, o.y, o.z, len);
    hist[3 * (size_t)p + 1] = make_float4(m1, m2, n.w, 0.0f);
    hist[3 * (size_t)p + 2] = make_float4(n.x, n.y, n.z, 0.0f);
}

// What k_motion reads: this frame's camera, the context's current primitives in the caller's order and the caller's
// previous ones (nullptr: that class did not move).
template <class View>
struct MotionArgs {
    uint32_t width, height, tiles_x;
    uint32_t n_sph, n_faces, n_verts;
    using view_type = View;
    View view;                                                 // this frame's camera, or its lens
    const float4* __restrict__ aov;                            // rt3_aov records (3 float4 each)
    const float4* __restrict__ sph;                            // (C, r) as rt3_set_spheres took them
    const float* __restrict__ sph_invr;                        // 1 / r
    const float4* __restrict__ prev_sph;                       // (C', r'), or nullptr
    const uint4* __restrict__ gfaces;                          // rt3_gface records (3 x 16 bytes each; the first holds v1, v2, v3)
    const float4* __restrict__ verts;                          // the merged vertices
    const float4* __restrict__ prev_verts;                     // the previous vertices, or nullptr
};

// per pixel the world-space displacement from the point it shows to where that surface point was in the previous frame,
// (mx, my, mz, 1), or (0, 0, 0, 0) where nothing moved or nothing is known.  Every gather index is checked against its buffer first.
// VIEW: kViewCamera, or the lens model: step 2's point then lies on the lens's centre ray.
template <uint32_t VIEW> using MotionArgsOf = MotionArgs<std::conditional_t<VIEW == kViewCamera, CameraRays, LensArgs>>;
template <uint32_t VIEW>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_motion(const MotionArgsOf<VIEW> M, float4* __restrict__ out) {
    const uint32_t ty = blockIdx.x / M.tiles_x, tx = blockIdx.x - ty * M.tiles_x;
    const int x = (int)(tx * kDnTile + threadIdx.x), y = (int)(ty * kDnTile + threadIdx.y);
    const int W = (int)M.width, H = (int)M.height;
    if (x >= W || y >= H) return;
    const uint32_t p = (uint32_t)(y * W + x);
    const float z = M.aov[3 * (size_t)p + 1].w;
    const float4 ki = M.aov[3 * (size_t)p + 2];
    const uint32_t kind = __float_as_uint(ki.x), index = __float_as_uint(ki.y);
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool sphere = kind == 2u && M.prev_sph && index < M.n_sph;            // RT3_HIT_SPHERE
    const bool face = kind == 1u && M.prev_verts && index < M.n_faces;          // RT3_HIT_FACE
    if (!__builtin_isinf(z) && (sphere || face)) {
        // 2: the shown point on the pixel-centre ray (4.12 step 2)
        float px, py, pz;
        if constexpr (VIEW == kViewCamera) {
            const CameraRays& V = M.view;
            const float u = (float)x / ((float)W - 1.0f), v = (float)(H - 1 - y) / ((float)H - 1.0f);
            const float dx = ((V.lx + u * V.hx) + v * V.vx) - V.ox;
            const float dy = ((V.ly + u * V.hy) + v * V.vy) - V.oy;
            const float dz = ((V.lz + u * V.hz) + v * V.vz) - V.oz;
            const float inv = 1.0f / __builtin_sqrtf(dn_dot(dx, dy, dz, dx, dy, dz));
            px = V.ox + z * (dx * inv); py = V.oy + z * (dy * inv); pz = V.oz + z * (dz * inv);
        } else {
            const rt3lens::Frame F{ M.view.width, M.view.height, 1u, 0u, 0u };
            float o[3], d[3];
            rt3lens::ray<VIEW>(M.view.lens, F, (uint32_t)x, (uint32_t)y, 0u, o, d);
            px = o[0] + z * d[0]; py = o[1] + z * d[1]; pz = o[2] + z * d[2];
        }
        if (sphere) {
            // 3: translation and uniform scaling about the centre
            const float4 c = M.sph[index], q = M.prev_sph[index];
            const bool same = __float_as_uint(c.x) == __float_as_uint(q.x) && __float_as_uint(c.y) == __float_as_uint(q.y) &&
                              __float_as_uint(c.z) == __float_as_uint(q.z) && __float_as_uint(c.w) == __float_as_uint(q.w);
            if (!same) {
                const float k = q.w * M.sph_invr[index];
                const float qx = q.x + (px - c.x) * k, qy = q.y + (py - c.y) * k, qz = q.z + (pz - c.z) * k;
                o = make_float4(qx - px, qy - py, qz - pz, 1.0f);
            }
        } else {
            // 4: the barycentrics of P in the current triangle, applied to the previous one
            const uint4 f = M.gfaces[3 * (size_t)index];
            if (f.x < M.n_verts && f.y < M.n_verts && f.z < M.n_verts) {
                const float4 a = M.verts[f.x], b = M.verts[f.y], c = M.verts[f.z];
                const float4 a1 = M.prev_verts[f.x], b1 = M.prev_verts[f.y], c1 = M.prev_verts[f.z];
                const bool same = __float_as_uint(a.x) == __float_as_uint(a1.x) && __float_as_uint(a.y) == __float_as_uint(a1.y) &&
                                  __float_as_uint(a.z) == __float_as_uint(a1.z) && __float_as_uint(b.x) == __float_as_uint(b1.x) &&
                                  __float_as_uint(b.y) == __float_as_uint(b1.y) && __float_as_uint(b.z) == __float_as_uint(b1.z) &&
                                  __float_as_uint(c.x) == __float_as_uint(c1.x) && __float_as_uint(c.y) == __float_as_uint(c1.y) &&
                                  __float_as_uint(c.z) == __float_as_uint(c1.z);
                if (!same) {
                    const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
                    const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
                    const float wx = px - a.x, wy = py - a.y, wz = pz - a.z;
                    const float d00 = dn_dot(e1x, e1y, e1z, e1x, e1y, e1z), d01 = dn_dot(e1x, e1y, e1z, e2x, e2y, e2z);
                    const float d11 = dn_dot(e2x, e2y, e2z, e2x, e2y, e2z);
                    const float d20 = dn_dot(wx, wy, wz, e1x, e1y, e1z), d21 = dn_dot(wx, wy, wz, e2x, e2y, e2z);
                    const float den = d00 * d11 - d01 * d01;
                    if (den != 0.0f) {
                        const float b2 = (d11 * d20 - d01 * d21) / den, b3 = (d00 * d21 - d01 * d20) / den;
                        const float qx = (a1.x + b2 * (b1.x - a1.x)) + b3 * (c1.x - a1.x);
                        const float qy = (a1.y + b2 * (b1.y - a1.y)) + b3 * (c1.y - a1.y);
                        const float qz = (a1.z + b2 * (b1.z - a1.z)) + b3 * (c1.z - a1.z);
                        o = make_float4(qx - px, qy - py, qz - pz, 1.0f);
                    }
                }
            }
        }
    }
    out[p] = o;
}

}  // namespace

// ======================================================================================================
// The entry points (rt3.h): the checks, the context's scratch, the launches
// ======================================================================================================
static_assert(sizeof(rt3_denoise_params) == 16, "rt3.h: rt3_denoise_params");
static_assert(sizeof(rt3_history) == 48, "rt3.h: rt3_history");
static_assert(sizeof(rt3_temporal_params) == 32, "rt3.h: rt3_temporal_params");

// ---- The denoiser
static int denoise_checks(rt3_ctx* ctx, uint32_t w, uint32_t h, const void* colour, const void* aov, const rt3_denoise_params* p,
                          const void* out) {
    if (!p) return fail(ctx, RT3_E_ARG, "p is NULL");
    if (!colour || !aov || !out) return fail(ctx, RT3_E_ARG, "colour / aov / out is NULL");
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 26)) return fail(ctx, RT3_E_ARG, "the frame must have 1 .. 2^26 pixels");
    if (p->iterations < 1 || p->iterations > 8) return fail(ctx, RT3_E_ARG, "iterations must be 1 .. 8");
    if (p->normal_power < 1 || p->normal_power > 1024 || (p->normal_power & (p->normal_power - 1)))
        return fail(ctx, RT3_E_ARG, "normal_power must be a power of two in 1 .. 1024");
    if (!std::isfinite(p->sigma_luminance) || !(p->sigma_luminance > 0.0f) || !std::isfinite(p->sigma_depth) || !(p->sigma_depth > 0.0f))
        return fail(ctx, RT3_E_ARG, "sigma_luminance and sigma_depth must be finite and > 0");
    return 0;
}

// The scratch of a call over n = w * h pixels (ctx->d_dn, the context's): scratch_quads(n) float4 entries, [0, n) and [n, 2n) the two (I, v)
// planes the passes ping-pong, [2n, 3n) the guide, then n floats of depth slope.  With it what every kernel of the call reads and the launch
// geometry: one thread per pixel, 16 x 16 tiles.
static size_t scratch_quads(size_t npix) { return 3 * npix + (npix + 3) / 4; }
struct DenoisePlan {
    DenoiseArgs D;
    float4 *pa, *pb, *guide;
    float* gz;
    dim3 grid, block;
    DenoisePlan(uint32_t w, uint32_t h, const rt3_denoise_params& p, float4* scratch) : block(kDnTile, kDnTile) {
        const size_t npix = (size_t)w * h;
        pa = scratch; pb = pa + npix; guide = pb + npix;
        gz = reinterpret_cast<float*>(guide + npix);
        D.width = w; D.height = h;
        D.tiles_x = (w + kDnTile - 1) / kDnTile;
        D.squarings = 0;
        while ((1u << D.squarings) < p.normal_power) D.squarings++;
        D.sigma_l = p.sigma_luminance; D.sigma_z = p.sigma_depth;
        D.guide = guide; D.gz = gz;
        grid = dim3(D.tiles_x * ((h + kDnTile - 1) / kDnTile));
    }
};

// k_denoise_atrous once per pass from plane pb, ping-ponging the two (I, v) planes; the last pass remodulates into `out`.  hist (the temporal
// call): pass 0 also writes the history colour.
static int atrous_passes(rt3_ctx* ctx, const DenoisePlan& P, uint32_t iterations, const float4* aov, float4* out, float4* hist, hipStream_t stream) {
    float4* src = P.pb;
    float4* dst = P.pa;
    for (uint32_t i = 0; i < iterations; i++) {
        const bool last = i + 1 == iterations, history = hist && i == 0;
        const auto pass = last ? (history ? k_denoise_atrous<true, true> : k_denoise_atrous<true, false>)
                               : (history ? k_denoise_atrous<false, true> : k_denoise_atrous<false, false>);
        hipLaunchKernelGGL(pass, P.grid, P.block, 0, stream, P.D, (const float4*)src, last ? out : dst, 1 << i, aov, history ? hist : (float4*)nullptr);
        RT3_HIP(hipGetLastError());
        float4* t = src; src = dst; dst = t;
    }
    return 0;
}

extern "C" int rt3_denoise_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const void* d_colour, const void* d_aov, const rt3_denoise_params* p, void* d_out,
                                  void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = denoise_checks(ctx, w, h, d_colour, d_aov, p, d_out);
    if (rc) return rc;
    if (((uintptr_t)d_colour | (uintptr_t)d_aov | (uintptr_t)d_out) % 16u != 0)
        return fail(ctx, RT3_E_ARG, "d_colour_rgba, d_aov and d_out_rgba must be 16-byte aligned");
    const size_t npix = (size_t)w * h;
    const uintptr_t o = (uintptr_t)d_out, oe = o + npix * sizeof(float4);
    const uintptr_t c = (uintptr_t)d_colour, a = (uintptr_t)d_aov;
    if ((o < c + npix * sizeof(float4) && c < oe) || (o < a + npix * sizeof(rt3_aov) && a < oe))
        return fail(ctx, RT3_E_ARG, "d_out_rgba overlaps an input");
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream)) || (rc = ctx->d_dn.ensure(ctx, scratch_quads(npix)))) return rc;
    const DenoisePlan P(w, h, *p, ctx->d_dn);
    const float4* const aov = (const float4*)d_aov;
    hipLaunchKernelGGL(k_denoise_prepare, P.grid, P.block, 0, stream, P.D, (const float4*)d_colour, aov, P.pa, P.guide, P.gz);
    RT3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_denoise_moments<false>, P.grid, P.block, 0, stream, P.D, (const float4*)P.pa, P.pb, (const float4*)nullptr);
    RT3_HIP(hipGetLastError());
    if ((rc = atrous_passes(ctx, P, p->iterations, aov, (float4*)d_out, nullptr, stream))) return rc;
    return leave(ctx, stream);
}

extern "C" int rt3_denoise(rt3_ctx* ctx, uint32_t w, uint32_t h, const float* colour, const rt3_aov* aov, const rt3_denoise_params* p, float* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = denoise_checks(ctx, w, h, colour, aov, p, out);
    if (rc) return rc;
    const size_t npix = (size_t)w * h;
    return staged(ctx, { stage_in(colour, npix * sizeof(float4)), stage_in(aov, npix * sizeof(rt3_aov)), stage_out(out, npix * sizeof(float4)) },
                  [&](void* const* d) { return rt3_denoise_device(ctx, w, h, d[0], d[1], p, d[2], ctx->stream); });
}

// ---- The views of the temporal denoiser and of the motion plane: the pinhole camera, or a lens
// h x v, written out: (hy vz - hz vy, hz vx - hx vz, hx vy - hy vx)
static void cross3(const float* h, const float* v, float* out) {
    out[0] = h[1] * v[2] - h[2] * v[1];
    out[1] = h[2] * v[0] - h[0] * v[2];
    out[2] = h[0] * v[1] - h[1] * v[0];
}

static float dot3h(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// A camera the reprojection can use: finite fields, horizontal x vertical != 0, and an image plane that misses the origin.
static bool camera_ok(const rt3_camera* c) {
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(c->origin[i]) || !std::isfinite(c->horizontal[i]) || !std::isfinite(c->vertical[i]) || !std::isfinite(c->lower_left_corner[i]))
            return false;
    float n[3], l[3];
    cross3(c->horizontal, c->vertical, n);
    if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return false;
    for (int i = 0; i < 3; i++) l[i] = c->lower_left_corner[i] - c->origin[i];
    return dot3h(l, n) != 0.0f;
}

// This frame's camera, the first twelve floats of CameraReproject and of CameraRays.
template <class V>
static void set_camera(V& v, const rt3_camera* c) {
    v.ox = c->origin[0]; v.oy = c->origin[1]; v.oz = c->origin[2];
    v.hx = c->horizontal[0]; v.hy = c->horizontal[1]; v.hz = c->horizontal[2];
    v.vx = c->vertical[0]; v.vy = c->vertical[1]; v.vz = c->vertical[2];
    v.lx = c->lower_left_corner[0]; v.ly = c->lower_left_corner[1]; v.lz = c->lower_left_corner[2];
}

// The launch argument of the lens forms: both lenses by value, the frame, and whether the inverse law may take the shortcut.
static LensArgs lens_args(const rt3_lens* lens, const rt3_lens* prev, uint32_t w, uint32_t h) {
    LensArgs A;
    A.lens = *lens; A.prev = *prev;
    A.width = w; A.height = h;
    A.same = rt3lens::same_optic(*lens, *prev) ? 1u : 0u;
    return A;
}

// fn(the view as a compile-time constant): kViewCamera, or the lens's model.
template <uint32_t VIEW> using ViewConstant = std::integral_constant<uint32_t, VIEW>;
template <class Fn>
static void with_view(const rt3_camera*, Fn fn) { fn(ViewConstant<kViewCamera>{}); }
template <class Fn>
static void with_view(const rt3_lens* lens, Fn fn) {
    switch (lens->model) {
    case RT3_LENS_EQUIRECT: fn(ViewConstant<RT3_LENS_EQUIRECT>{}); break;
    case RT3_LENS_FISHEYE:  fn(ViewConstant<RT3_LENS_FISHEYE>{}); break;
    case RT3_LENS_ORTHO:    fn(ViewConstant<RT3_LENS_ORTHO>{}); break;
    default:                fn(ViewConstant<RT3_LENS_CUBE>{}); break;
    }
}

// ---- The temporal denoiser, for a frame rendered through a camera or through a lens: View is rt3_camera or rt3_lens,
// view / prev_view this frame's and the previous frame's.  What follows is overloaded on it: its name in the refusals, what refuses a pair of
// views, and the view's part of k_temporal_reproject's arguments.
static const char* view_name(const rt3_camera*) { return "cam"; }
static const char* view_name(const rt3_lens*) { return "lens"; }

static int views_ok(rt3_ctx* ctx, uint32_t, uint32_t, const rt3_camera* cam, const rt3_camera* prev_cam) {
    if (!camera_ok(cam) || (prev_cam && !camera_ok(prev_cam)))
        return fail(ctx, RT3_E_ARG, "a camera has a non-finite field, horizontal x vertical = 0, or an image plane through its origin");
    return 0;
}
static int views_ok(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_lens* lens, const rt3_lens* prev_lens) {
    if (const char* why = rt3lens::refusal(lens, w, h)) return fail(ctx, RT3_E_ARG, why);
    if (prev_lens) {
        if (const char* why = rt3lens::refusal(prev_lens, w, h)) return fail(ctx, RT3_E_ARG, std::string("prev_") + why);
        if (prev_lens->model != lens->model) return fail(ctx, RT3_E_ARG, "prev_lens must have the model of lens");
    }
    return 0;
}

// The projection constants of DESIGN.md 4.12 step 3, in f32 in this order: L = llc' - o', n = h x v, a_u = (v x n) / (h . (v x n)),
// a_v = (n x h) / (v . (n x h)) component by component, then L . n.  Without a previous camera they stay zero and are not read.
static TemporalArgs<CameraReproject> reproject_args(const rt3_camera* cam, const rt3_camera* prev_cam, uint32_t, uint32_t) {
    TemporalArgs<CameraReproject> A{};
    CameraReproject& V = A.view;
    set_camera(V, cam);
    if (prev_cam) {
        const float* hh = prev_cam->horizontal;
        const float* vv = prev_cam->vertical;
        float l[3], n[3], vn[3], nh[3];
        for (int i = 0; i < 3; i++) l[i] = prev_cam->lower_left_corner[i] - prev_cam->origin[i];
        cross3(hh, vv, n);
        cross3(vv, n, vn);
        const float du = dot3h(hh, vn);
        cross3(n, hh, nh);
        const float dv = dot3h(vv, nh);
        V.pox = prev_cam->origin[0]; V.poy = prev_cam->origin[1]; V.poz = prev_cam->origin[2];
        V.plx = l[0]; V.ply = l[1]; V.plz = l[2];
        V.nx = n[0]; V.ny = n[1]; V.nz = n[2];
        V.aux = vn[0] / du; V.auy = vn[1] / du; V.auz = vn[2] / du;
        V.avx = nh[0] / dv; V.avy = nh[1] / dv; V.avz = nh[2] / dv;
        V.ln = dot3h(l, n);
        A.has_prev = 1;
        A.same_cam = std::memcmp(prev_cam, cam, sizeof(rt3_camera)) == 0;
    }
    return A;
}
// The lens forms of k_temporal_reproject take the lenses by value; nothing is worked out here.
static TemporalArgs<LensArgs> reproject_args(const rt3_lens* lens, const rt3_lens* prev_lens, uint32_t w, uint32_t h) {
    TemporalArgs<LensArgs> A{};
    A.view = lens_args(lens, prev_lens ? prev_lens : lens, w, h);
    A.has_prev = prev_lens ? 1u : 0u;
    A.same_cam = A.view.same;
    return A;
}

// What every form checks.
template <class View>
static int temporal_checks_of(rt3_ctx* ctx, uint32_t w, uint32_t h, const View* view, const void* colour, const void* aov, const View* prev_view,
                              const void* prev_history, const void* motion, const rt3_temporal_params* p, const void* out, const void* out_history) {
    const char* const what = view_name(view);
    if (!p || !view) return fail(ctx, RT3_E_ARG, std::string("p / ") + what + " is NULL");
    if (!colour || !aov || !out || !out_history) return fail(ctx, RT3_E_ARG, "colour / aov / out / out_history is NULL");
    if (!prev_view != !prev_history) return fail(ctx, RT3_E_ARG, std::string("prev_") + what + " and prev_history must both be NULL or both be non-NULL");
    if (w < 2 || h < 2 || (uint64_t)w * h > (1ull << 26)) return fail(ctx, RT3_E_ARG, "the frame must be at least 2 x 2 and have at most 2^26 pixels");
    int rc = denoise_checks(ctx, w, h, colour, aov, &p->spatial, out);
    if (rc) return rc;
    if (!(p->alpha > 0.0f && p->alpha <= 1.0f) || !(p->moments_alpha > 0.0f && p->moments_alpha <= 1.0f))
        return fail(ctx, RT3_E_ARG, "alpha and moments_alpha must be in (0, 1]");
    if (!std::isfinite(p->depth_tolerance) || !(p->depth_tolerance > 0.0f)) return fail(ctx, RT3_E_ARG, "depth_tolerance must be finite and > 0");
    if (!(p->normal_tolerance >= -1.0f && p->normal_tolerance <= 1.0f)) return fail(ctx, RT3_E_ARG, "normal_tolerance must be in [-1, 1]");
    if ((rc = views_ok(ctx, w, h, view, prev_view))) return rc;
    const size_t npix = (size_t)w * h, nf = npix * sizeof(float4), nh = npix * sizeof(rt3_history);
    const struct { const void* ptr; size_t n; } in[4] = { { colour, nf }, { aov, npix * sizeof(rt3_aov) }, { prev_history, nh }, { motion, nf } };
    for (const auto& i : in)
        if (i.ptr && (ranges_overlap(out, nf, i.ptr, i.n) || ranges_overlap(out_history, nh, i.ptr, i.n)))
            return fail(ctx, RT3_E_ARG, "an output overlaps an input");
    if (ranges_overlap(out, nf, out_history, nh)) return fail(ctx, RT3_E_ARG, "out_rgba and out_history overlap");
    return 0;
}

// The device form for either view: k_temporal_reproject -> k_denoise_moments<true> -> the passes (pass 0 also writes the history colour); the
// same scratch as rt3_denoise.  d_motion: the plane rt3_motion wrote, or NULL; without a previous frame it is checked and not read.
template <class View>
static int temporal_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const View* view, const void* d_colour, const void* d_aov, const View* prev_view,
                           const void* d_prev_history, const void* d_motion, const rt3_temporal_params* p, void* d_out, void* d_out_history,
                           void* stream_) {
    int rc = temporal_checks_of(ctx, w, h, view, d_colour, d_aov, prev_view, d_prev_history, d_motion, p, d_out, d_out_history);
    if (rc) return rc;
    if (((uintptr_t)d_colour | (uintptr_t)d_aov | (uintptr_t)d_prev_history | (uintptr_t)d_motion | (uintptr_t)d_out | (uintptr_t)d_out_history) % 16u != 0)
        return fail(ctx, RT3_E_ARG, "device buffers must be 16-byte aligned");
    auto A = reproject_args(view, prev_view, w, h);
    A.alpha = p->alpha; A.moments_alpha = p->moments_alpha; A.depth_tolerance = p->depth_tolerance; A.normal_tolerance = p->normal_tolerance;
    const float4* const colour = (const float4*)d_colour;
    const float4* const aov = (const float4*)d_aov;
    const float4* const prev = (const float4*)d_prev_history;
    const float4* const motion = prev_view ? (const float4*)d_motion : nullptr;
    float4* const hist = (float4*)d_out_history;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream)) || (rc = ctx->d_dn.ensure(ctx, scratch_quads((size_t)w * h)))) return rc;
    const DenoisePlan P(w, h, p->spatial, ctx->d_dn);
    with_view(view, [&](auto model) {
        constexpr uint32_t VIEW = decltype(model)::value;
        if (motion) hipLaunchKernelGGL((k_temporal_reproject<VIEW, true>), P.grid, P.block, 0, stream, P.D, A, colour, aov, prev, P.pa, P.guide, P.gz, hist, motion);
        else hipLaunchKernelGGL((k_temporal_reproject<VIEW, false>), P.grid, P.block, 0, stream, P.D, A, colour, aov, prev, P.pa, P.guide, P.gz, hist, motion);
    });
    RT3_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_denoise_moments<true>, P.grid, P.block, 0, stream, P.D, (const float4*)P.pa, P.pb, (const float4*)hist);
    RT3_HIP(hipGetLastError());
    if ((rc = atrous_passes(ctx, P, p->spatial.iterations, aov, (float4*)d_out, hist, stream))) return rc;
    return leave(ctx, stream);
}

// The host form for either view.
template <class View>
static int temporal_host(rt3_ctx* ctx, uint32_t w, uint32_t h, const View* view, const float* colour, const rt3_aov* aov, const View* prev_view,
                         const rt3_history* prev_history, const float* motion, const rt3_temporal_params* p, float* out, rt3_history* out_history) {
    int rc = temporal_checks_of(ctx, w, h, view, colour, aov, prev_view, prev_history, motion, p, out, out_history);
    if (rc) return rc;
    const size_t npix = (size_t)w * h;
    return staged(ctx, { stage_in(colour, npix * sizeof(float4)), stage_in(aov, npix * sizeof(rt3_aov)),
                         stage_in(prev_history, npix * sizeof(rt3_history)), stage_in(motion, npix * sizeof(float4)),
                         stage_out(out, npix * sizeof(float4)), stage_out(out_history, npix * sizeof(rt3_history)) },
                  [&](void* const* d) { return temporal_device(ctx, w, h, view, d[0], d[1], prev_view, d[2], d[3], p, d[4], d[5], ctx->stream); });
}

extern "C" {

int rt3_denoise_temporal_motion_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const void* d_colour, const void* d_aov,
                                       const rt3_camera* prev_cam, const void* d_prev_history, const void* d_motion,
                                       const rt3_temporal_params* p, void* d_out, void* d_out_history, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    return temporal_device(ctx, w, h, cam, d_colour, d_aov, prev_cam, d_prev_history, d_motion, p, d_out, d_out_history, stream_);
}

int rt3_denoise_temporal_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const void* d_colour, const void* d_aov,
                                const rt3_camera* prev_cam, const void* d_prev_history, const rt3_temporal_params* p, void* d_out,
                                void* d_out_history, void* stream_) {
    return rt3_denoise_temporal_motion_device(ctx, w, h, cam, d_colour, d_aov, prev_cam, d_prev_history, nullptr, p, d_out, d_out_history, stream_);
}

int rt3_denoise_temporal_motion(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const float* colour, const rt3_aov* aov,
                                const rt3_camera* prev_cam, const rt3_history* prev_history, const float* motion,
                                const rt3_temporal_params* p, float* out, rt3_history* out_history) {
    if (!ctx) return RT3_E_ARG;
    return temporal_host(ctx, w, h, cam, colour, aov, prev_cam, prev_history, motion, p, out, out_history);
}

int rt3_denoise_temporal(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const float* colour, const rt3_aov* aov,
                         const rt3_camera* prev_cam, const rt3_history* prev_history, const rt3_temporal_params* p, float* out,
                         rt3_history* out_history) {
    return rt3_denoise_temporal_motion(ctx, w, h, cam, colour, aov, prev_cam, prev_history, nullptr, p, out, out_history);
}

// Lens sequences: the same for a frame rendered through a lens.
int rt3_denoise_temporal_optic_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_lens* lens, const void* d_colour, const void* d_aov,
                                      const rt3_lens* prev_lens, const void* d_prev_history, const void* d_motion,
                                      const rt3_temporal_params* p, void* d_out, void* d_out_history, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    return temporal_device(ctx, w, h, lens, d_colour, d_aov, prev_lens, d_prev_history, d_motion, p, d_out, d_out_history, stream_);
}

int rt3_denoise_temporal_optic(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_lens* lens, const float* colour, const rt3_aov* aov,
                               const rt3_lens* prev_lens, const rt3_history* prev_history, const float* motion,
                               const rt3_temporal_params* p, float* out, rt3_history* out_history) {
    if (!ctx) return RT3_E_ARG;
    return temporal_host(ctx, w, h, lens, colour, aov, prev_lens, prev_history, motion, p, out, out_history);
}

}  // extern "C"

// ---- The motion plane
// What both forms check: the frame, the view, and the previous arrays against the scene on the context.
// cam or lens: the frame's view, exactly one of them.
static int motion_checks(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const rt3_lens* lens, const void* aov, const void* prev_sph,
                         uint32_t n_prev_sph, const void* prev_verts, uint32_t n_prev_verts, const void* out) {
    if ((!cam && !lens) || !aov || !out) return fail(ctx, RT3_E_ARG, "cam / lens / aov / out_motion is NULL");
    if (w < 2 || h < 2 || (uint64_t)w * h > (1ull << 26)) return fail(ctx, RT3_E_ARG, "the frame must be at least 2 x 2 and have at most 2^26 pixels");
    if (cam && !camera_ok(cam))
        return fail(ctx, RT3_E_ARG, "the camera has a non-finite field, horizontal x vertical = 0, or an image plane through its origin");
    if (lens)
        if (const char* why = rt3lens::refusal(lens, w, h)) return fail(ctx, RT3_E_ARG, why);
    if ((!prev_sph && n_prev_sph) || (!prev_verts && n_prev_verts)) return fail(ctx, RT3_E_ARG, "a NULL previous array must have a count of 0");
    if (prev_sph && ctx->n_sph == 0) return fail(ctx, RT3_E_STATE, "previous spheres were given, but the context has no spheres");
    if (prev_verts && ctx->n_faces == 0) return fail(ctx, RT3_E_STATE, "previous vertices were given, but the context has no committed mesh");
    if (prev_verts && !ctx->mesh_in_sync)
        return fail(ctx, RT3_E_STATE, "the merged entity buffers were changed after the last rt3_mesh_commit (rt3_mesh_begin / rt3_mesh_put without a commit)");
    if (prev_sph && n_prev_sph != ctx->n_sph) return fail(ctx, RT3_E_ARG, "n_prev_spheres must equal the context's sphere count");
    if (prev_verts && n_prev_verts != ctx->d_verts.size()) return fail(ctx, RT3_E_ARG, "n_prev_vertices must equal the vertex count of the merged entity buffers");
    const size_t npix = (size_t)w * h, no = npix * sizeof(float4);
    const struct { const void* ptr; size_t n; } in[3] = { { aov, npix * sizeof(rt3_aov) }, { prev_sph, (size_t)n_prev_sph * sizeof(float4) },
                                                          { prev_verts, (size_t)n_prev_verts * sizeof(float4) } };
    for (const auto& i : in)
        if (i.ptr && ranges_overlap(out, no, i.ptr, i.n)) return fail(ctx, RT3_E_ARG, "out_motion overlaps an input");
    return 0;
}

// The device form for either view (cam or lens, exactly one): k_motion, one launch.  A class whose previous array is NULL did not move and is
// never gathered: its buffers and counts stay out of the launch; the counts bound every gather of the other.
static int motion_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const rt3_lens* lens, const void* d_aov, const void* d_prev_sph,
                         uint32_t n_prev_sph, const void* d_prev_verts, uint32_t n_prev_verts, void* d_out, void* stream_) {
    int rc = motion_checks(ctx, w, h, cam, lens, d_aov, d_prev_sph, n_prev_sph, d_prev_verts, n_prev_verts, d_out);
    if (rc) return rc;
    if (((uintptr_t)d_aov | (uintptr_t)d_prev_sph | (uintptr_t)d_prev_verts | (uintptr_t)d_out) % 16u != 0)
        return fail(ctx, RT3_E_ARG, "device buffers must be 16-byte aligned");
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    const auto launch = [&](auto model) {
        constexpr uint32_t VIEW = decltype(model)::value;
        MotionArgsOf<VIEW> M{};
        M.width = w; M.height = h;
        M.tiles_x = (w + kDnTile - 1) / kDnTile;
        if constexpr (VIEW == kViewCamera) set_camera(M.view, cam);
        else M.view = lens_args(lens, lens, w, h);
        M.aov = (const float4*)d_aov;
        if (d_prev_sph) { M.sph = ctx->d_sph_cr; M.sph_invr = ctx->d_sph_invr; M.prev_sph = (const float4*)d_prev_sph; M.n_sph = ctx->n_sph; }
        if (d_prev_verts) {
            M.gfaces = (const uint4*)ctx->d_gfaces.get(); M.verts = ctx->d_verts; M.prev_verts = (const float4*)d_prev_verts;
            M.n_faces = ctx->n_faces; M.n_verts = (uint32_t)ctx->d_verts.size();
        }
        const dim3 grid(M.tiles_x * ((h + kDnTile - 1) / kDnTile)), block(kDnTile, kDnTile);
        hipLaunchKernelGGL(k_motion<VIEW>, grid, block, 0, stream, M, (float4*)d_out);
    };
    if (lens) with_view(lens, launch);
    else with_view(cam, launch);
    RT3_HIP(hipGetLastError());
    return leave(ctx, stream);
}

// The host form for either view.
static int motion_host(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const rt3_lens* lens, const rt3_aov* aov, const float* prev_sph,
                       uint32_t n_prev_sph, const float* prev_verts, uint32_t n_prev_verts, float* out) {
    int rc = motion_checks(ctx, w, h, cam, lens, aov, prev_sph, n_prev_sph, prev_verts, n_prev_verts, out);
    if (rc) return rc;
    const size_t npix = (size_t)w * h;
    return staged(ctx, { stage_in(aov, npix * sizeof(rt3_aov)), stage_in(prev_sph, (size_t)n_prev_sph * sizeof(float4)),
                         stage_in(prev_verts, (size_t)n_prev_verts * sizeof(float4)), stage_out(out, npix * sizeof(float4)) },
                  [&](void* const* d) { return motion_device(ctx, w, h, cam, lens, d[0], d[1], n_prev_sph, d[2], n_prev_verts, d[3], ctx->stream); });
}

extern "C" {

int rt3_motion_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const void* d_aov, const void* d_prev_sph, uint32_t n_prev_sph,
                      const void* d_prev_verts, uint32_t n_prev_verts, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    return motion_device(ctx, w, h, cam, nullptr, d_aov, d_prev_sph, n_prev_sph, d_prev_verts, n_prev_verts, d_out, stream_);
}

int rt3_motion(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_camera* cam, const rt3_aov* aov, const float* prev_sph, uint32_t n_prev_sph,
               const float* prev_verts, uint32_t n_prev_verts, float* out) {
    if (!ctx) return RT3_E_ARG;
    return motion_host(ctx, w, h, cam, nullptr, aov, prev_sph, n_prev_sph, prev_verts, n_prev_verts, out);
}

int rt3_motion_optic_device(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_lens* lens, const void* d_aov, const void* d_prev_sph, uint32_t n_prev_sph,
                            const void* d_prev_verts, uint32_t n_prev_verts, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    if (!lens) return fail(ctx, RT3_E_ARG, "lens / aov / out_motion is NULL");
    return motion_device(ctx, w, h, nullptr, lens, d_aov, d_prev_sph, n_prev_sph, d_prev_verts, n_prev_verts, d_out, stream_);
}

int rt3_motion_optic(rt3_ctx* ctx, uint32_t w, uint32_t h, const rt3_lens* lens, const rt3_aov* aov, const float* prev_sph, uint32_t n_prev_sph,
                     const float* prev_verts, uint32_t n_prev_verts, float* out) {
    if (!ctx) return RT3_E_ARG;
    if (!lens) return fail(ctx, RT3_E_ARG, "lens / aov / out_motion is NULL");
    return motion_host(ctx, w, h, nullptr, lens, aov, prev_sph, n_prev_sph, prev_verts, n_prev_verts, out);
}

}  // extern "C"
