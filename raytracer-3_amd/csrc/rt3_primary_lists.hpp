// rt3_primary_lists.hpp — k_primary_lists: which spheres the primary rays of a group of 64 owned pixels can meet (the strip lists that
// k_trace_mfma32's render form traces its primary rays against when it refills its stock: refill_from_traced_stock, rt3_matrix_filter.hpp).
// Part of rt3_device.hip (one translation unit, gfx950 only); included from there, in this order.
#pragma once

namespace {

// For every aligned group of 64 consecutive owned-pixel indices (start_path's `pix`; frame_row() maps its row to the frame, so shards work
// unchanged) one bit per sphere row, n_blocks dwords: bit set = "some primary ray of some sample of a pixel of the group may pass sphere_root's
// candidate rule for this sphere".  The test is CONSERVATIVE for every jitter in [-1/2, 1/2] pixel, every lens point, both roots, any t_min:
//   A ray of the piece of a frame row that the group covers starts at o0 + f, |f| <= R, and passes through T0 + e, |e| <= rho, where T0 is the
//   centre of the piece's footprint on the focus plane and rho its half-extent (triangle inequality over `horizontal` and `vertical`).  Its point
//   at parameter lambda lies within dev(lambda) = |1 - lambda| R + |lambda| rho of the point q(lambda) of the central line o0 -> T0, and dev is
//   Lipschitz in the distance s = lambda L along that line with constant k = (R + rho) / L.  For a sphere (C, r) at distance d from the line, foot
//   at s_c: the ray can reach it only if sqrt(d^2 + x^2) <= r + dev(s_c / L) + k |x| for some x, and the minimum of sqrt(d^2 + x^2) - k |x| is
//   d sqrt(1 - k^2).  So the sphere is a candidate unless  d^2 (1 - k^2) > (r + dev(s_c / L))^2.
// The geometry runs in f64; what f32 does to the rays and to sphere_root is added to the radii:
//   delta  start_path builds origin and target from camera vectors of magnitude M with a few roundings of size 2^-24 M each and normalises the
//          direction (2^-23 relative): the ray it makes is an ideal ray of a lens and a footprint wider by delta = 2^-18 M (64 roundings' worth);
//   eps    sphere_root's discriminant carries a rounding error below 20 x 2^-24 (|C - o|^2 + r^2), so a ray passes its rule only if its line comes
//          within sqrt(r^2 + eps (r^2 + |C - o|^2)) of C, eps = 4e-6 (three times that bound); |C - o| <= |C - o0| + R.
// The lens axes are unit vectors but need not be orthogonal: |a lu + b lv|^2 <= (a^2 + b^2)(1 + |lu.lv|).
// A comparison that meets a NaN makes a candidate; a piece with k >= 1, L = 0 or non-finite values marks the whole group "no list" (every bit of
// its n_blocks words set: more than any threshold below 32 n_blocks, and still exact for a larger one — the list is then every row).
// A group may straddle frame rows (width not a multiple of 64): its list is the union over its row pieces.  The direct spheres are not listed:
// every ray is tested against them anyway.  One wave per group; lane l owns spheres l, l + 64, ...; the words are written by lane 0 with
// ordinary vector stores (the ballot goes through a VGPR).
constexpr double kListEps = 4e-6, kListDelta = 0x1p-18, kListSlack = 1e-6;
__global__ __launch_bounds__(kBlock) void k_primary_lists(const TraceArgs A, uint32_t n_groups, uint32_t n_blocks, uint32_t* __restrict__ masks) {
    const uint32_t lane = lane_id();
    const uint32_t g = blockIdx.x * (uint32_t)(kBlock / 64) + threadIdx.x / 64u;
    if (g >= n_groups) return;                                          // (wave-uniform)
    const CamDev& c = A.cam;
    const double o0x = c.ox, o0y = c.oy, o0z = c.oz;
    const double lh = sqrt((double)c.hx * c.hx + (double)c.hy * c.hy + (double)c.hz * c.hz);
    const double lv = sqrt((double)c.vx * c.vx + (double)c.vy * c.vy + (double)c.vz * c.vz);
    const double mag = fmax(fmax(fmax(fabs(o0x), fabs(o0y)), fabs(o0z)),
                            fmax(fmax(fabs((double)c.lx) + fabs((double)c.hx) + fabs((double)c.vx), fabs((double)c.ly) + fabs((double)c.hy) + fabs((double)c.vy)),
                                 fabs((double)c.lz) + fabs((double)c.hz) + fabs((double)c.vz)));
    const double delta = kListDelta * mag;
    double R = delta;
    if (A.lens_radius > 0.0f) {
        const double uv = fabs((double)A.lux * A.lvx + (double)A.luy * A.lvy + (double)A.luz * A.lvz);
        R += (double)A.lens_radius * sqrt(1.0 + uv) * (1.0 + 1e-5);      // (1e-5: sincos2pi's cos^2 + sin^2 is 1 only to 1e-6)
    }
    const double wm1 = (double)A.width - 1.0, hm1 = (double)A.height - 1.0;
    bool no_list = !(mag < 1e300) || !(R < 1e300);                      // (false for a NaN too)
    uint32_t cand = 0;                                                  // bit i: sphere 64 i + lane
    const uint32_t n_chunks = (n_blocks + 1u) / 2u;
    const uint32_t p_end = min(g * 64u + 64u, A.npix);
    for (uint32_t p = g * 64u; p < p_end && !no_list;) {                // the group's pieces of frame rows
        const uint32_t lrow = fdiv(p, A.div_width), x0 = p - lrow * A.width;
        const uint32_t nx = min(A.width - x0, p_end - p);               // pixels x0 .. x0 + nx - 1 of the row
        const uint32_t y = frame_row(A, lrow);
        p += nx;
        const double uc = ((double)x0 + 0.5 * (double)(nx - 1u)) / wm1, du = 0.5 * (double)nx / wm1;
        const double vc = (double)(A.height - 1u - y) / hm1, dv = 0.5 / hm1;
        const double ax = ((double)c.lx + uc * c.hx + vc * c.vx) - o0x, ay = ((double)c.ly + uc * c.hy + vc * c.vy) - o0y,
                     az = ((double)c.lz + uc * c.hz + vc * c.vz) - o0z;
        const double L = sqrt(ax * ax + ay * ay + az * az);
        const double rho = du * lh + dv * lv + delta;
        const double k = (R + rho) / L;
        if (!(L > 0.0) || !(k < 1.0) || !(L < 1e300)) { no_list = true; break; }
        const double inv_l = 1.0 / L, shrink = 1.0 - k * k;
        for (uint32_t i = 0; i < n_chunks; i++) {
            const uint32_t j = i * 64u + lane;
            if (j >= A.n_sph) continue;
            const float4 s = A.sph[j];                                  // (C, r^2)
            const double wx = (double)s.x - o0x, wy = (double)s.y - o0y, wz = (double)s.z - o0z;
            const double ww = wx * wx + wy * wy + wz * wz;
            const double sc = (wx * ax + wy * ay + wz * az) * inv_l;    // foot of C on the central line
            const double d2 = ww - sc * sc;
            const double far = sqrt(ww) + R;
            const double r_eff = sqrt((double)s.w + kListEps * ((double)s.w + far * far));
            const double lam = sc * inv_l;
            const double reach = (r_eff + fabs(1.0 - lam) * R + fabs(lam) * rho) * (1.0 + kListSlack);
            if (!(d2 * shrink > reach * reach)) cand |= 1u << i;
        }
    }
    for (uint32_t i = 0; i < A.n_direct; i++)
        if ((A.direct[i] & 63u) == lane) cand &= ~(1u << (A.direct[i] >> 6));
    for (uint32_t i = 0; i < n_chunks; i++) {
        const unsigned long long m = no_list ? ~0ull : __ballot((cand >> i) & 1u);
        if (lane == 0) {
            masks[(size_t)g * n_blocks + 2u * i] = (uint32_t)m;
            if (2u * i + 1u < n_blocks) masks[(size_t)g * n_blocks + 2u * i + 1u] = (uint32_t)(m >> 32);
        }
    }
}

}  // namespace
