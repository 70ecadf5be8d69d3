// rt3_regroup.hpp — the group order of the multi-level filter again, on the device (rt3_regroup*)
// Part of rt3_scene.hip (one translation unit, gfx950 only); included from there, after rt3_scene_kernels.hpp.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------------
// The order is median_split_order's rule with a stable full sort in place of nth_element (tests/regroup_ref.py restates it in numpy):
// every part larger than `group` is sorted by its centres' coordinate along the longest axis of their box and cut after split_half()
// entries.  Part boundaries depend on the counts alone, so the host knows them without looking at a position.
//   parts above kSplitCap entries   one global pass per level: k_part_box, k_part_keys, a stable radix sort of (part, coordinate) -> id
//   parts that fit in LDS           k_split_lds, one workgroup per part, all remaining levels without leaving the CU
// ------------------------------------------------------------------------------------------------------
// LDS per entry of k_split_lds: 8 (key) + 12 (centre) + 4 (id) = 24 bytes, plus 10 KiB of tables.  160 KiB per CU hold 6 400 entries; the
// sorting network wants a power of two: 4096 entries, 106 KiB.
constexpr uint32_t kSplitCap = 4096, kSplitThreads = 1024, kSplitPerThread = kSplitCap / kSplitThreads;
constexpr uint32_t kSplitLevels = 9;                                // 4096 >> 9 = 8 = the leaf group: no part is larger after nine cuts
constexpr uint32_t kSplitSlots = 1u << (kSplitLevels - 1);          // parts of the last level that sorts
constexpr size_t kSplitLds = (size_t)kSplitCap * 24 + kSplitSlots * 6 * 4 + 2 * 1024 * 2;
constexpr uint32_t kBoxPerThread = 16;                              // k_part_box: positions per thread
static_assert(kSplitCap >> kSplitLevels == kLevFan && kSplitLds <= 160 * 1024, "k_split_lds: nine levels down to a leaf group, within one CU's LDS");

// median_split_order's cut: the left part is a multiple of `unit`, so that only the very last group is short (count > group)
__host__ __device__ inline uint32_t split_half(uint32_t count, uint32_t group, uint32_t super) {
    const uint32_t unit = count > group * super ? group * super : group;
    uint32_t half = (count / 2 + unit - 1) / unit * unit;
    if (half >= count) half = count - unit;
    return half;
}
// the sort key of a coordinate: order-preserving, -0 and +0 equal
__device__ __forceinline__ uint32_t split_key(float c) { return ordered_bits(c == 0.0f ? 0.0f : c); }
// first maximum of hi - lo in f32, as the host's loop picks it
__device__ __forceinline__ uint32_t split_axis(const uint32_t* box) {
    float ext[3];
    for (int a = 0; a < 3; a++) ext[a] = ordered_float(box[3 + a]) - ordered_float(box[a]);
    uint32_t axis = 0;
    for (uint32_t a = 1; a < 3; a++) if (ext[a] > ext[axis]) axis = a;
    return axis;
}
// Adds one centre per active lane to the box of its part (box + 6 s: min x, y, z, max x, y, z as ordered integers; LDS or global).  A wave
// whose active lanes all belong to one part — every wave of the upper levels — reduces across its lanes first and issues six atomics.
__device__ __forceinline__ void part_box_merge(uint32_t* box, bool act, uint32_t s, uint32_t lo[3], uint32_t hi[3]) {
    const uint64_t mask = __ballot(act);
    if (mask == 0ull) return;
    const uint32_t s0 = (uint32_t)__shfl((int)s, __ffsll((long long)mask) - 1);
    if (!act) for (int a = 0; a < 3; a++) { lo[a] = 0xFFFFFFFFu; hi[a] = 0u; }
    if (__all(!act || s == s0)) {
        for (int a = 0; a < 3; a++)
            for (int o = 32; o > 0; o >>= 1) {
                lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o));
                hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o));
            }
        if (lane_id() == 0u) for (int a = 0; a < 3; a++) { atomicMin(box + 6 * s0 + a, lo[a]); atomicMax(box + 6 * s0 + 3 + a, hi[a]); }
    } else if (act)
        for (int a = 0; a < 3; a++) { atomicMin(box + 6 * s + a, lo[a]); atomicMax(box + 6 * s + 3 + a, hi[a]); }
}
__device__ __forceinline__ void part_box_add(uint32_t* box, bool act, uint32_t s, float x, float y, float z) {
    uint32_t lo[3] = { ordered_bits(x), ordered_bits(y), ordered_bits(z) }, hi[3] = { lo[0], lo[1], lo[2] };
    part_box_merge(box, act, s, lo, hi);
}

// The coordinates a primitive is sorted by: its centre in the current records, or the class's filter centre where the record is not usable
// (a sphere k_refit_spheres turned into a pad; a face whose bound is no longer finite and below 3e38).
__global__ void k_regroup_centres_sph(const float4* __restrict__ cr, uint32_t n, float ecx, float ecy, float ecz, float4* __restrict__ cen) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 s = cr[i];
    const float r2f = s.w * s.w;
    const bool good = s.w > 0.0f && s.x - s.x == 0.0f && s.y - s.y == 0.0f && s.z - s.z == 0.0f && r2f - r2f == 0.0f;
    cen[i] = good ? make_float4(s.x, s.y, s.z, 0.0f) : make_float4(ecx, ecy, ecz, 0.0f);
}
__global__ void k_regroup_centres_tri(const float4* __restrict__ bound, uint32_t n, const uint32_t* __restrict__ box, float4* __restrict__ cen) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float centre[3];
    box_centre(box, centre);
    const float4 b = bound[i];
    const bool good = b.x - b.x == 0.0f && b.y - b.y == 0.0f && b.z - b.z == 0.0f && b.w >= 0.0f && b.w < 3e38f;
    cen[i] = good ? make_float4(b.x, b.y, b.z, 0.0f) : make_float4(centre[0], centre[1], centre[2], 0.0f);
}

// ---- one level above the LDS limit.  begins[0 .. n_parts]: the level's parts, in position order (the host's table)
__device__ __forceinline__ uint32_t part_of(const uint32_t* __restrict__ begins, uint32_t n_parts, uint32_t p) {
    uint32_t lo = 0, hi = n_parts;                                  // the last k with begins[k] <= p
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) / 2; if (begins[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}
__global__ void k_part_box_clear(uint32_t n_parts, uint32_t* __restrict__ box) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_parts * 6u) box[i] = i % 6u < 3u ? 0xFFFFFFFFu : 0u;
}
// A workgroup covers kBoxPerThread x its size consecutive positions, which lie in a few parts (the largest part of a global level is longer
// than that, the others need not be), and a lane keeps the box of the part it is in: it flushes with atomics of its own when its part changes,
// and at the end a wave whose lanes ended in one part reduces first.  Few atomics on the few words of a level's boxes are the point.
__global__ void k_part_box(const uint32_t* __restrict__ begins, uint32_t n_parts, const uint32_t* __restrict__ ids, const float4* __restrict__ cen,
                           uint32_t n, uint32_t* __restrict__ box) {
    const uint32_t base = blockIdx.x * (blockDim.x * kBoxPerThread) + threadIdx.x;
    uint32_t cur = 0xFFFFFFFFu, lo[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, hi[3] = { 0u, 0u, 0u };
    for (uint32_t k = 0; k < kBoxPerThread; k++) {
        const uint32_t p = base + k * blockDim.x;
        if (p >= n) break;
        const uint32_t s = part_of(begins, n_parts, p);
        if (s != cur) {                                             // the lane crossed into the next part
            if (cur != 0xFFFFFFFFu) for (int a = 0; a < 3; a++) { atomicMin(box + 6 * cur + a, lo[a]); atomicMax(box + 6 * cur + 3 + a, hi[a]); }
            cur = s;
            for (int a = 0; a < 3; a++) { lo[a] = 0xFFFFFFFFu; hi[a] = 0u; }
        }
        const float4 c = cen[ids[p]];
        const uint32_t o[3] = { ordered_bits(c.x), ordered_bits(c.y), ordered_bits(c.z) };
        for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], o[a]); hi[a] = max(hi[a], o[a]); }
    }
    part_box_merge(box, cur != 0xFFFFFFFFu, cur, lo, hi);
}
// key = part : coordinate along the part's axis; a part that is not cut any more (at most `group` entries) keeps its order: one key for all
__global__ void k_part_keys(const uint32_t* __restrict__ begins, uint32_t n_parts, const uint32_t* __restrict__ ids, const float4* __restrict__ cen,
                            uint32_t n, const uint32_t* __restrict__ box, uint32_t group, uint64_t* __restrict__ keys) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = part_of(begins, n_parts, p);
    uint32_t k = 0;
    if (begins[s + 1] - begins[s] > group) {
        const uint32_t axis = split_axis(box + 6 * s);
        const float4 c = cen[ids[p]];
        k = split_key(axis == 0u ? c.x : axis == 1u ? c.y : c.z);
    }
    keys[p] = (uint64_t)s << 32 | k;
}

// ---- every remaining level of one part of at most kSplitCap entries, in LDS (begins: the parts of the last table level)
// Level L has up to 2^L parts, numbered by their path: the children of part s are 2 s and 2 s + 1 (a part that is not cut passes
// everything to 2 s), so part numbers follow positions and one sort of the whole block by (part, coordinate, position) sorts every part
// by itself; the position in the key makes the bitonic network stable.  Key: part (8 bits) : coordinate (32) : position (12) : entry (12) —
// the entry, an index into cx / cy / cz / gid, rides in the bits below everything that orders, so a swap moves one 8-byte word.
__global__ __launch_bounds__(kSplitThreads) void k_split_lds(const uint32_t* __restrict__ begins, const uint32_t* __restrict__ ids,
                                                             const float4* __restrict__ cen, uint32_t group, uint32_t super,
                                                             uint32_t* __restrict__ perm) {
    extern __shared__ uint64_t split_lds[];
    uint64_t* const key = split_lds;
    float* const cx = (float*)(key + kSplitCap);
    float* const cy = cx + kSplitCap;
    float* const cz = cy + kSplitCap;
    uint32_t* const gid = (uint32_t*)(cz + kSplitCap);
    uint32_t* const box = gid + kSplitCap;                          // [kSplitSlots][6]
    uint16_t* const tab_b = (uint16_t*)(box + kSplitSlots * 6);     // level L at [2^L - 1, 2^(L+1) - 1): the parts' first position and count
    uint16_t* const tab_c = tab_b + 1024;
    const uint32_t t = threadIdx.x, first = begins[blockIdx.x], count = begins[blockIdx.x + 1] - first;     // <= kSplitCap: regroup_plan checks its table
    uint32_t n_sort = 2;                                            // the network's size
    while (n_sort < count) n_sort <<= 1;
    for (uint32_t p = t; p < count; p += kSplitThreads) {
        const uint32_t g = ids[first + p];
        const float4 c = cen[g];
        gid[p] = g; cx[p] = c.x; cy[p] = c.y; cz[p] = c.z; key[p] = p;
    }
    if (t == 0) { tab_b[0] = 0; tab_c[0] = (uint16_t)count; }
    uint32_t slot[kSplitPerThread];                                 // the part of position t + k kSplitThreads: a sort never moves an entry out of its part
    for (uint32_t k = 0; k < kSplitPerThread; k++) slot[k] = 0;
    __syncthreads();
    for (uint32_t L = 0; L < kSplitLevels; L++) {
        const uint32_t lvl = (1u << L) - 1u, n_slots = 1u << L;
        if (!__syncthreads_or(t < n_slots && tab_c[lvl + t] > group)) break;       // nothing left to cut
        if (t < n_slots * 6u) box[t] = t % 6u < 3u ? 0xFFFFFFFFu : 0u;
        for (uint32_t i = t + kSplitThreads; i < n_slots * 6u; i += kSplitThreads) box[i] = i % 6u < 3u ? 0xFFFFFFFFu : 0u;
        __syncthreads();
        for (uint32_t k = 0; k < kSplitPerThread; k++) {
            const uint32_t p = t + k * kSplitThreads;
            const bool act = p < count && tab_c[lvl + slot[k]] > group;
            const uint32_t j = act ? (uint32_t)key[p] & 0xFFFu : 0u;
            part_box_add(box, act, slot[k], cx[j], cy[j], cz[j]);
        }
        __syncthreads();
        for (uint32_t k = 0; k < kSplitPerThread; k++) {
            const uint32_t p = t + k * kSplitThreads;
            if (p >= n_sort) continue;
            uint64_t kk = ~0ull;                                    // positions behind the part sort last
            if (p < count) {
                const uint32_t s = slot[k], j = (uint32_t)key[p] & 0xFFFu;
                uint32_t kb = 0;
                if (tab_c[lvl + s] > group) {
                    const uint32_t axis = split_axis(box + 6 * s);
                    kb = split_key(axis == 0u ? cx[j] : axis == 1u ? cy[j] : cz[j]);
                }
                kk = (uint64_t)s << 56 | (uint64_t)kb << 24 | (uint64_t)p << 12 | j;
            }
            key[p] = kk;
        }
        __syncthreads();
        for (uint32_t size = 2; size <= n_sort; size <<= 1)
            for (uint32_t j = size >> 1; j > 0; j >>= 1) {
                for (uint32_t i = t; i < n_sort / 2; i += kSplitThreads) {
                    const uint32_t l = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), r = l | j;
                    const uint64_t a = key[l], b = key[r];
                    if ((a > b) == ((l & size) == 0u)) { key[l] = b; key[r] = a; }
                }
                __syncthreads();
            }
        const uint32_t nxt = (2u << L) - 1u;
        if (t < n_slots) {
            const uint32_t b0 = tab_b[lvl + t], c0 = tab_c[lvl + t];
            const uint32_t h = c0 > group ? split_half(c0, group, super) : c0;
            tab_b[nxt + 2 * t] = (uint16_t)b0; tab_c[nxt + 2 * t] = (uint16_t)h;
            tab_b[nxt + 2 * t + 1] = (uint16_t)(b0 + h); tab_c[nxt + 2 * t + 1] = (uint16_t)(c0 - h);
        }
        for (uint32_t k = 0; k < kSplitPerThread; k++) {
            const uint32_t p = t + k * kSplitThreads, s = slot[k];
            if (p >= count) continue;
            const uint32_t b0 = tab_b[lvl + s], c0 = tab_c[lvl + s];
            slot[k] = 2 * s + (c0 > group && p - b0 >= split_half(c0, group, super) ? 1u : 0u);
        }
        __syncthreads();
    }
    for (uint32_t p = t; p < count; p += kSplitThreads) perm[first + p] = gid[(uint32_t)key[p] & 0xFFFu];
}

// the inverse of the order, for rt3_update_spheres*: slot[perm[k]] = k (direct spheres keep 0xFFFFFFFF)
__global__ void k_inverse_slots(const uint32_t* __restrict__ perm, uint32_t n_pos, uint32_t* __restrict__ slot) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pos) return;
    const uint32_t j = perm[k];
    if (j != 0xFFFFFFFFu) slot[j] = k;
}

}  // namespace
