// rt3_adaptive.hpp — the kernels of rt3_render_path_adaptive* around the trace kernels' list form: the reduce pass over an
// active list, the convergence rule, the ordered compaction of the pixels that stay active, and the resolves that divide by a pixel's own count.
// Part of rt3_device.hip (one translation unit, gfx950 only); included from there, in this order.
#pragma once

namespace {

// k_accumulate over a list: entry k of the list adds the round's samples rad[s n_active + k], s = 0 .. ns - 1 in sample order, to the sums and the
// sums of squares of pixel active[k], and sets that pixel's count.  (Round 0 is dense: k_accumulate<true>, and the counts are filled.)
template <bool VAR>
__global__ __launch_bounds__(kBlock) void k_accumulate_list(const Rgb* __restrict__ rad, const uint32_t* __restrict__ active, uint32_t n_active,
                                                           float4* __restrict__ accum, float4* __restrict__ accum_sq, uint32_t* __restrict__ counts,
                                                           uint32_t ns, uint32_t count_after) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_active) return;
    const uint32_t pix = active[k];
    float4 a = accum[pix];
    float4 q = VAR ? accum_sq[pix] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < ns; s++) {
        const Rgb r = rad[(size_t)s * n_active + k];
        a.x = a.x + r.r; a.y = a.y + r.g; a.z = a.z + r.b;
        if (VAR) { q.x = fma_(r.r, r.r, q.x); q.y = fma_(r.g, r.g, q.y); q.z = fma_(r.b, r.b, q.z); }
    }
    accum[pix] = a;
    if (VAR) accum_sq[pix] = q;
    counts[pix] = count_after;
}

// The rule of DESIGN.md 4.15 for every owned pixel, over its own count: all in f32, every operation rounded on its own (-ffp-contract=off), in the
// order written there.  A NaN anywhere compares false: converged.
__global__ __launch_bounds__(kBlock) void k_adaptive_flags(const float4* __restrict__ accum, const float4* __restrict__ accum_sq,
                                                          const uint32_t* __restrict__ counts, uint32_t npix, float threshold, float dark,
                                                          uint8_t* __restrict__ unconverged) {
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float4 S = accum[pix], Q = accum_sq[pix];
    const float n = (float)counts[pix];
    const float mr = S.x / n, mg = S.y / n, mb = S.z / n;
    float vr = Q.x / n - mr * mr, vg = Q.y / n - mg * mg, vb = Q.z / n - mb * mb;
    vr = vr > 0.0f ? vr : 0.0f; vg = vg > 0.0f ? vg : 0.0f; vb = vb > 0.0f ? vb : 0.0f;
    const float e2 = ((vr + vg) + vb) / n;
    const float d = ((mr + mg) + mb) + dark;
    const float lim = threshold * d;
    unconverged[pix] = e2 > lim * lim ? 1 : 0;
}

// Does owned pixel `pix` stay active after the round that brought the active pixels to `done` samples?  It was active (its count is `done`: a
// pixel that left keeps a smaller one) and one of the owned pixels of its 3 x 3 frame neighbourhood, itself included, is unconverged.  Local row
// l +- 1 is a frame neighbour only where frame_row() puts it on the adjoining frame row: inside a row block of the shard, not across two.
struct AdaptiveGeom { uint32_t width, rows, tile_rows, tile_index, tile_count; FastDiv div_width, div_tile_rows; };
__device__ __forceinline__ uint32_t adaptive_frame_row(const AdaptiveGeom& G, uint32_t local_row) {
    if (G.tile_count <= 1) return local_row;
    const uint32_t lb = fdiv(local_row, G.div_tile_rows), in = local_row - lb * G.tile_rows;
    return (lb * G.tile_count + G.tile_index) * G.tile_rows + in;
}
__device__ __forceinline__ bool adaptive_stays(const AdaptiveGeom& G, const uint32_t* __restrict__ counts, const uint8_t* __restrict__ unconverged,
                                               uint32_t pix, uint32_t done) {
    if (counts[pix] != done) return false;
    const uint32_t l = fdiv(pix, G.div_width), x = pix - l * G.width;
    const uint32_t y = adaptive_frame_row(G, l);
    const uint32_t x0 = x > 0 ? x - 1 : x, x1 = x + 1 < G.width ? x + 1 : x;
    bool any = false;
    for (int dl = -1; dl <= 1; dl++) {
        if ((dl < 0 && l == 0) || (dl > 0 && l + 1 >= G.rows)) continue;
        const uint32_t lq = l + (uint32_t)dl;
        if (dl != 0 && adaptive_frame_row(G, lq) != y + (uint32_t)dl) continue;
        for (uint32_t xq = x0; xq <= x1; xq++) any |= unconverged[(size_t)lq * G.width + xq] != 0;
    }
    return any;
}
// Compaction in ascending pixel order, in two passes over the same predicate: k_adaptive_count leaves the number of staying pixels of every block,
// k_adaptive_select sums the counts of the blocks before its own (a few thousand words at 1080p), ranks its pixels by ballot and prefix count and
// writes them; the last block also writes the list's length to *n_out, the one word the host reads back per round.
// (block_sum: rt3_shared_kernels.hpp)
__global__ __launch_bounds__(kBlock) void k_adaptive_count(const AdaptiveGeom G, const uint32_t* __restrict__ counts,
                                                          const uint8_t* __restrict__ unconverged, uint32_t npix, uint32_t done,
                                                          uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t lds[kBlock / 64];
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    const bool stay = pix < npix && adaptive_stays(G, counts, unconverged, pix, done);
    const uint32_t n = block_sum(stay ? 1u : 0u, lds);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = n;
}
__global__ __launch_bounds__(kBlock) void k_adaptive_select(const AdaptiveGeom G, const uint32_t* __restrict__ counts,
                                                           const uint8_t* __restrict__ unconverged, uint32_t npix, uint32_t done,
                                                           const uint32_t* __restrict__ block_counts, uint32_t* __restrict__ active_out,
                                                           uint32_t* __restrict__ n_out) {
    __shared__ uint32_t lds[kBlock / 64];
    __shared__ uint32_t wave_n[kBlock / 64];
    uint32_t before = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kBlock) before += block_counts[b];
    before = block_sum(before, lds);
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    const bool stay = pix < npix && adaptive_stays(G, counts, unconverged, pix, done);
    const unsigned long long m = __ballot(stay);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t at = before;
    for (uint32_t w = 0; w < wave; w++) at += wave_n[w];
    if (stay) active_out[at + prefix_count(m)] = pix;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        uint32_t total = before;
        for (uint32_t w = 0; w < kBlock / 64; w++) total += wave_n[w];
        *n_out = total;
    }
}

// k_resolve / k_resolve_float over an adaptive accumulation: every pixel is divided by its own count.
__global__ __launch_bounds__(kBlock) void k_resolve_counts(const float4* __restrict__ accum, const uint32_t* __restrict__ counts, uint32_t npix,
                                                          uint32_t flags, uint32_t* __restrict__ out) {
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float4 a = accum[pix];
    const float n = (float)counts[pix];
    float r = a.x / n, g = a.y / n, b = a.z / n;
    if (flags & RT3_FLAG_GAMMA2) {
        r = r > 0.0f ? __builtin_sqrtf(r) : 0.0f;
        g = g > 0.0f ? __builtin_sqrtf(g) : 0.0f;
        b = b > 0.0f ? __builtin_sqrtf(b) : 0.0f;
    }
    out[pix] = pack_pixel(r, g, b);
}
__global__ __launch_bounds__(kBlock) void k_resolve_float_counts(const float4* __restrict__ accum, const uint32_t* __restrict__ counts, uint32_t npix,
                                                                float4* __restrict__ out) {
    const uint32_t pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= npix) return;
    const float4 a = accum[pix];
    const float n = (float)counts[pix];
    out[pix] = make_float4(a.x / n, a.y / n, a.z / n, 0.0f);
}

}  // namespace
