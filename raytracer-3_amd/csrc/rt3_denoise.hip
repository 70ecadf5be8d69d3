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

// What k_temporal_reproject reads besides DenoiseArgs: this frame's camera, the previous camera's constants, the parameters.
struct TemporalArgs {
    float ox, oy, oz, hx, hy, hz, vx, vy, vz, lx, ly, lz;      // this frame's camera
    float pox, poy, poz, plx, ply, plz;                        // o' and L = llc' - o'
    float nx, ny, nz, aux, auy, auz, avx, avy, avz, ln;        // n = h x v, a_u, a_v, L . n
    uint32_t has_prev, same_cam;
    float alpha, moments_alpha, depth_tolerance, normal_tolerance;
};

__device__ __forceinline__ float dn_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// DESIGN.md 4.12 steps 1-5 (in place of k_denoise_prepare): colour, rt3_aov records and the previous history -> il = (I.rgb, L(I)) of the
// blended I, the guide and gz planes as k_denoise_prepare writes them, and the history record of the pixel with (I, length) in its first
// float4 (pass 0 replaces I), (M1, M2, depth, 0) and (normal, 0).  MOTION: a pixel that hit and whose motion record
// (m, moved) has moved != 0 adds m to its world point and is projected even under a byte-equal camera; every other pixel takes the
// operations of the MOTION = false kernel.
template <bool MOTION>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_temporal_reproject(const DenoiseArgs D, const TemporalArgs T,
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
        // 2: the world point of the pixel-centre ray, relative to the previous origin (the sky: the direction)
        const float u = (float)x / ((float)W - 1.0f), v = (float)(H - 1 - y) / ((float)H - 1.0f);
        const float dx = ((T.lx + u * T.hx) + v * T.vx) - T.ox;
        const float dy = ((T.ly + u * T.hy) + v * T.vy) - T.oy;
        const float dz = ((T.lz + u * T.hz) + v * T.vz) - T.oz;
        const float inv = 1.0f / __builtin_sqrtf(dn_dot(dx, dy, dz, dx, dy, dz));
        const float ux = dx * inv, uy = dy * inv, uz = dz * inv;
        const bool hit = !__builtin_isinf(n.w);
        float rx = hit ? (T.ox + n.w * ux) - T.pox : ux;
        float ry = hit ? (T.oy + n.w * uy) - T.poy : uy;
        float rz = hit ? (T.oz + n.w * uz) - T.poz : uz;
        bool moved = false;
        if (MOTION && hit) {
            const float4 m = motion[p];
            moved = m.w != 0.0f;
            if (moved) {
                rx = ((T.ox + n.w * ux) + m.x) - T.pox;
                ry = ((T.oy + n.w * uy) + m.y) - T.poy;
                rz = ((T.oz + n.w * uz) + m.z) - T.poz;
            }
        }
        // 3: project into the previous camera (skipped for a byte-equal camera: every pixel that has not moved maps to itself)
        float xp = (float)x, yp = (float)y;
        bool ok = true;
        if (!T.same_cam || moved) {
            const float sc = T.ln / dn_dot(rx, ry, rz, T.nx, T.ny, T.nz);
            ok = __builtin_isfinite(sc) && sc > 0.0f;
            const float px = sc * rx - T.plx, py = sc * ry - T.ply, pz = sc * rz - T.plz;
            xp = dn_dot(px, py, pz, T.aux, T.auy, T.auz) * ((float)W - 1.0f);
            yp = ((float)H - 1.0f) - dn_dot(px, py, pz, T.avx, T.avy, T.avz) * ((float)H - 1.0f);
        }
        // 4: the bilinear taps that lie in the frame and are consistent (no tap can when x' or y' is outside (-1, W) x (-1, H), or NaN)
        if (ok && xp > -1.0f && xp < (float)W && yp > -1.0f && yp < (float)H) {
            const float zhat = __builtin_sqrtf(dn_dot(rx, ry, rz, rx, ry, rz));
            const float bound = T.depth_tolerance * (g + 1e-3f * zhat);
            const float x0 = __builtin_floorf(xp), y0 = __builtin_floorf(yp);
            const float fx = xp - x0, fy = yp - y0;
            const int ix = (int)x0, iy = (int)y0;
            const float wt[4] = { (1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int qx = ix + (k & 1), qy = iy + (k >> 1);
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
struct MotionArgs {
    uint32_t width, height, tiles_x;
    uint32_t n_sph, n_faces, n_verts;
    float ox, oy, oz, hx, hy, hz, vx, vy, vz, lx, ly, lz;      // this frame's camera
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
__global__ __launch_bounds__(kDnTile * kDnTile) void k_motion(const MotionArgs M, float4* __restrict__ out) {
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
        const float u = (float)x / ((float)W - 1.0f), v = (float)(H - 1 - y) / ((float)H - 1.0f);
        const float dx = ((M.lx + u * M.hx) + v * M.vx) - M.ox;
        const float dy = ((M.ly + u * M.hy) + v * M.vy) - M.oy;
        const float dz = ((M.lz + u * M.hz) + v * M.vz) - M.oz;
        const float inv = 1.0f / __builtin_sqrtf(dn_dot(dx, dy, dz, dx, dy, dz));
        const float px = M.ox + z * (dx * inv), py = M.oy + z * (dy * inv), pz = M.oz + z * (dz * inv);
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
    hipLaunchKernelGGL(k_denoise_moments<false>, grid, block, 0, stream, D, (const float4*)pa, pb, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    float4* src = pb;
    float4* dst = pa;
    for (uint32_t i = 0; i < L.iterations; i++) {
        if (i + 1 == L.iterations) hipLaunchKernelGGL((k_denoise_atrous<true, false>), grid, block, 0, stream, D, (const float4*)src, (float4*)L.out, 1 << i, aov, nullptr);
        else hipLaunchKernelGGL((k_denoise_atrous<false, false>), grid, block, 0, stream, D, (const float4*)src, dst, 1 << i, aov, nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        float4* t = src; src = dst; dst = t;
    }
    return hipSuccess;
}

hipError_t temporal_launch(const TemporalLaunch& T, hipStream_t stream) {
    const DenoiseLaunch& L = T.base;
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
    TemporalArgs A;
    A.ox = T.cam[0]; A.oy = T.cam[1]; A.oz = T.cam[2];
    A.hx = T.cam[3]; A.hy = T.cam[4]; A.hz = T.cam[5];
    A.vx = T.cam[6]; A.vy = T.cam[7]; A.vz = T.cam[8];
    A.lx = T.cam[9]; A.ly = T.cam[10]; A.lz = T.cam[11];
    A.pox = T.prev_o[0]; A.poy = T.prev_o[1]; A.poz = T.prev_o[2];
    A.plx = T.prev_l[0]; A.ply = T.prev_l[1]; A.plz = T.prev_l[2];
    A.nx = T.prev_n[0]; A.ny = T.prev_n[1]; A.nz = T.prev_n[2];
    A.aux = T.a_u[0]; A.auy = T.a_u[1]; A.auz = T.a_u[2];
    A.avx = T.a_v[0]; A.avy = T.a_v[1]; A.avz = T.a_v[2];
    A.ln = T.ln;
    A.has_prev = T.has_prev; A.same_cam = T.same_cam;
    A.alpha = T.alpha; A.moments_alpha = T.moments_alpha; A.depth_tolerance = T.depth_tolerance; A.normal_tolerance = T.normal_tolerance;
    const dim3 grid(D.tiles_x * ((h + kDnTile - 1) / kDnTile)), block(kDnTile, kDnTile);
    const float4* aov = (const float4*)L.aov;
    float4* const hist = (float4*)T.out_history;
    if (T.motion) hipLaunchKernelGGL(k_temporal_reproject<true>, grid, block, 0, stream, D, A, (const float4*)L.colour, aov,
                                     (const float4*)T.prev_history, pa, guide, gz, hist, (const float4*)T.motion);
    else hipLaunchKernelGGL(k_temporal_reproject<false>, grid, block, 0, stream, D, A, (const float4*)L.colour, aov,
                            (const float4*)T.prev_history, pa, guide, gz, hist, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_denoise_moments<true>, grid, block, 0, stream, D, (const float4*)pa, pb, (const float4*)hist);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    float4* src = pb;
    float4* dst = pa;
    for (uint32_t i = 0; i < L.iterations; i++) {
        const bool last = i + 1 == L.iterations;
        if (i == 0 && last) hipLaunchKernelGGL((k_denoise_atrous<true, true>), grid, block, 0, stream, D, (const float4*)src, (float4*)L.out, 1, aov, hist);
        else if (i == 0) hipLaunchKernelGGL((k_denoise_atrous<false, true>), grid, block, 0, stream, D, (const float4*)src, dst, 1, aov, hist);
        else if (last) hipLaunchKernelGGL((k_denoise_atrous<true, false>), grid, block, 0, stream, D, (const float4*)src, (float4*)L.out, 1 << i, aov, nullptr);
        else hipLaunchKernelGGL((k_denoise_atrous<false, false>), grid, block, 0, stream, D, (const float4*)src, dst, 1 << i, aov, nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        float4* t = src; src = dst; dst = t;
    }
    return hipSuccess;
}

hipError_t motion_launch(const MotionLaunch& L, hipStream_t stream) {
    MotionArgs M;
    M.width = L.width; M.height = L.height;
    M.tiles_x = (L.width + kDnTile - 1) / kDnTile;
    M.n_sph = L.n_sph; M.n_faces = L.n_faces; M.n_verts = L.n_verts;
    M.ox = L.cam[0]; M.oy = L.cam[1]; M.oz = L.cam[2];
    M.hx = L.cam[3]; M.hy = L.cam[4]; M.hz = L.cam[5];
    M.vx = L.cam[6]; M.vy = L.cam[7]; M.vz = L.cam[8];
    M.lx = L.cam[9]; M.ly = L.cam[10]; M.lz = L.cam[11];
    M.aov = (const float4*)L.aov;
    M.sph = (const float4*)L.sph; M.sph_invr = L.sph_invr; M.prev_sph = (const float4*)L.prev_sph;
    M.gfaces = (const uint4*)L.gfaces; M.verts = (const float4*)L.verts; M.prev_verts = (const float4*)L.prev_verts;
    const dim3 grid(M.tiles_x * ((L.height + kDnTile - 1) / kDnTile)), block(kDnTile, kDnTile);
    hipLaunchKernelGGL(k_motion, grid, block, 0, stream, M, (float4*)L.out);
    return hipGetLastError();
}
