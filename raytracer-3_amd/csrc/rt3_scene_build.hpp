// rt3_scene_build.hpp — a full scene upload from device arrays (rt3_set_spheres_device / rt3_set_mesh_device): what
// rt3_set_spheres and rt3_mesh_commit decide on one host thread — validation, the filter centre, the direct list, which primitives take part in
// the group order — as kernels over the caller's arrays, and the ordered compaction that writes the initial group order.
// Part of rt3_scene.hip (one translation unit, gfx950 only); included from there, after rt3_regroup.hpp.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------------
// The header of a build: the few words phase 1 leaves for the host (one read-back) and for phase 2's kernels.  The block counts of the
// compaction follow at kSbWords.
// ------------------------------------------------------------------------------------------------------
constexpr uint32_t kSbBadRadius = 0;                                // lowest index of a sphere whose radius is not > 0 (0xFFFFFFFF: none)
constexpr uint32_t kSbBadKind = 1;                                  // != 0: a material kind above RT3_MAT_DIELECTRIC
constexpr uint32_t kSbFinite = 2;                                   // [3] finite coordinates per axis
constexpr uint32_t kSbCentre = 5;                                   // [3] the filter centre (f32 bits)
constexpr uint32_t kSbCand = 8;                                     // candidates for the direct list
constexpr uint32_t kSbInOrder = 9;                                  // primitives the compaction keeps: usable spheres / bounded faces
constexpr uint32_t kSbScene = 10;                                   // [2] the scene size (f64 bits)
constexpr uint32_t kSbBest = 12;                                    // [4 x 2] the direct list as keys, strongest first (0: none)
constexpr uint32_t kSbFaceError = 20;                               // != 0: a face references a vertex out of range (k_commit_mesh's flag)
constexpr uint32_t kSbWords = 32;
static_assert(kSbScene % 2 == 0 && kSbBest % 2 == 0, "the 64-bit words of the header are 8-byte aligned");

__global__ void k_sb_init(uint32_t* __restrict__ hdr) {
    if (threadIdx.x < kSbWords) hdr[threadIdx.x] = threadIdx.x == kSbBadRadius ? 0xFFFFFFFFu : 0u;
}

// ---- validation: what rt3_set_spheres / rt3_mesh_commit refuse, found without touching the scene
__global__ __launch_bounds__(kBlock) void k_sb_check_radii(const float4* __restrict__ cr, uint32_t n, uint32_t* __restrict__ hdr) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool bad = i < n && !(cr[i].w > 0.0f);                    // (NaN is bad)
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && lane_id() == (uint32_t)__ffsll((long long)m) - 1u) atomicMin(hdr + kSbBadRadius, i);      // the wave's lowest bad index
}
__global__ __launch_bounds__(kBlock) void k_sb_check_kinds(const rt3_material* __restrict__ mats, uint32_t n, uint32_t* __restrict__ hdr) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool bad = i < n && mats[i].kind > RT3_MAT_DIELECTRIC;
    if (bad) hdr[kSbBadKind] = 1u;                                  // (every writer stores the same word)
}

// ---- sphere_filter_centre: per axis the median at index m / 2 of the m finite coordinates.  The keys are order-preserving; a coordinate that is
// skipped gets the largest key (a NaN's, which no finite value has) and sorts behind the m that count.
__global__ __launch_bounds__(kBlock) void k_sb_axis_keys(const float4* __restrict__ cr, uint32_t n, uint32_t axis, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ hdr) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    float c = __builtin_nanf("");
    if (i < n) { const float4 s = cr[i]; c = axis == 0u ? s.x : axis == 1u ? s.y : s.z; }
    const bool fin = c - c == 0.0f;
    if (i < n) keys[i] = fin ? ordered_bits(c) : 0xFFFFFFFFu;
    const unsigned long long m = __ballot(fin);
    if (m != 0ull && lane_id() == 0u) atomicAdd(hdr + kSbFinite + axis, (uint32_t)__popcll(m));
}
__global__ void k_sb_pick_centre(const uint32_t* __restrict__ sorted, uint32_t axis, uint32_t* __restrict__ hdr) {
    const uint32_t m = hdr[kSbFinite + axis];
    hdr[kSbCentre + axis] = __float_as_uint(m ? ordered_float(sorted[m / 2u]) : 0.0f);
}

// ---- sphere_direct_list.  The distance of a centre from the filter centre in double, with the host's operations in the host's order (no
// contraction; sqrt and the division are the correctly rounded ones).  Distances are >= 0 or NaN, so their bit patterns order as the values do.
__device__ __forceinline__ double sb_dist(const float4 s, const uint32_t* __restrict__ hdr) {
    const float c0 = __uint_as_float(hdr[kSbCentre]), c1 = __uint_as_float(hdr[kSbCentre + 1]), c2 = __uint_as_float(hdr[kSbCentre + 2]);
    const double dx = (double)s.x - c0, dy = (double)s.y - c1, dz = (double)s.z - c2;
    return sqrt(dx * dx + dy * dy + dz * dz);
}
// the scene size's keys: the distances, a non-finite one counted as 0
__global__ __launch_bounds__(kBlock) void k_sb_dist_keys(const float4* __restrict__ cr, uint32_t n, const uint32_t* __restrict__ hdr,
                                                        uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double d = sb_dist(cr[i], hdr);
    keys[i] = d - d == 0.0 ? (uint64_t)__double_as_longlong(d) : 0ull;
}
__global__ void k_sb_pick_scene(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t* __restrict__ hdr) {
    *(uint64_t*)(hdr + kSbScene) = sorted[n / 2u];
}
// A candidate's key: ratio (>= 0.5: its bits order as the values do) : 0xFFFFFFFF - index — unique per sphere, and among equal ratios the lowest
// index is the strongest.  0 for a sphere that is no candidate.
__global__ __launch_bounds__(kBlock) void k_sb_ratio_keys(const float4* __restrict__ cr, uint32_t n, uint32_t* __restrict__ hdr,
                                                         uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool cand = false;
    if (i < n) {
        const float4 s = cr[i];
        const double dist = sb_dist(s, hdr), scene = __longlong_as_double((long long)*(const uint64_t*)(hdr + kSbScene));
        const double a = dist < scene ? scene : dist;               // std::max(dist, scene): a NaN distance stays
        const double b = a < 1e-30 ? 1e-30 : a;                     // std::max(a, 1e-30)
        const float ratio = (float)((double)s.w / b);
        cand = ratio >= 0.5f;                                       // (NaN: not chosen)
        keys[i] = cand ? (uint64_t)__float_as_uint(ratio) << 32 | (uint64_t)(0xFFFFFFFFu - i) : 0ull;
    }
    const unsigned long long m = __ballot(cand);
    if (m != 0ull && lane_id() == 0u) atomicAdd(hdr + kSbCand, (uint32_t)__popcll(m));
}
// The k-th strongest candidate: the largest key below the (k - 1)-th.  Four launches, k = 0 .. 3; a wave reduces first and issues one atomic.
__global__ __launch_bounds__(kBlock) void k_sb_top(const uint64_t* __restrict__ keys, uint32_t n, uint32_t k, uint32_t* __restrict__ hdr) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long* const best = (unsigned long long*)(hdr + kSbBest);
    const unsigned long long limit = k ? best[k - 1u] : ~0ull;
    unsigned long long v = 0ull;
    if (i < n) { const unsigned long long key = keys[i]; v = key < limit ? key : 0ull; }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        v = other > v ? other : v;
    }
    if (v != 0ull && lane_id() == 0u) atomicMax(best + k, v);
}

// ---- which primitives take part in the group order
// sphere_group_order's condition: not on the direct list, a finite centre and a finite r^2
struct SphInOrder {
    const float4* cr; const uint32_t* hdr;
    __device__ __forceinline__ bool operator()(uint32_t i) const {
        const unsigned long long* const best = (const unsigned long long*)(hdr + kSbBest);
        for (uint32_t k = 0; k < 4u; k++) if (best[k] != 0ull && 0xFFFFFFFFu - (uint32_t)best[k] == i) return false;
        const float4 s = cr[i];
        const float r2 = s.w * s.w;
        return s.x - s.x == 0.0f && s.y - s.y == 0.0f && s.z - s.z == 0.0f && r2 - r2 == 0.0f;
    }
};
// face_group_order's condition on the bounds k_commit_mesh wrote: a bounded hit region
struct FaceInOrder {
    const float4* bound;
    __device__ __forceinline__ bool operator()(uint32_t i) const {
        const float4 b = bound[i];
        return b.x - b.x == 0.0f && b.y - b.y == 0.0f && b.z - b.z == 0.0f && b.w >= 0.0f && b.w < 3e38f;
    }
};
// Compaction in ascending index order, in two passes over the same predicate (as rt3_adaptive.hpp's): the count of every block and the total;
// then every kept index i goes to kept[rank], rank = the kept indices below i, and (rest != null) every other one to rest[i - rank].
template <class P>
__global__ __launch_bounds__(kBlock) void k_compact_count(const P pred, uint32_t n, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ total) {
    __shared__ uint32_t lds[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool keep = i < n && pred(i);
    const uint32_t c = block_sum(keep ? 1u : 0u, lds);
    if (threadIdx.x == 0) { block_counts[blockIdx.x] = c; if (c) atomicAdd(total, c); }
}
template <class P>
__global__ __launch_bounds__(kBlock) void k_compact_select(const P pred, uint32_t n, const uint32_t* __restrict__ block_counts, uint32_t* __restrict__ kept,
                                                          uint32_t* __restrict__ rest) {
    __shared__ uint32_t lds[kBlock / 64];
    __shared__ uint32_t wave_n[kBlock / 64];
    uint32_t before = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kBlock) before += block_counts[b];
    before = block_sum(before, lds);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool keep = i < n && pred(i);
    const unsigned long long m = __ballot(keep);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t rank = before + prefix_count(m);
    for (uint32_t w = 0; w < wave; w++) rank += wave_n[w];
    if (keep) kept[rank] = i;
    else if (i < n && rest) rest[i - rank] = i;
}

// ---- the spheres' buffers: what rt3_set_spheres derives from record j on the host, with the same operations — (C, r^2), the record as given,
// 1 / r, the packed material (pack_material), the sphere's rows of the two flat filters (build_sphere_frags, build_sphere_frags32).  One thread
// per row of the flat filters: rows behind the last sphere and rows of direct spheres can never be candidates, and the records up to the next
// multiple of four are pads.
struct SphDirect { uint32_t n, id[4]; };
__global__ __launch_bounds__(kBlock) void k_build_spheres(const float4* __restrict__ in, const rt3_material* __restrict__ mats, uint32_t n, uint32_t n_rows,
                                                         float ecx, float ecy, float ecz, const SphDirect direct, float4* __restrict__ sph,
                                                         float4* __restrict__ cr, float* __restrict__ invr, float4* __restrict__ mat,
                                                         uint32_t* __restrict__ kind, u32x4* __restrict__ frag, u32x4* __restrict__ frag32) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_rows) return;
    float fx = 0.0f, fy = 0.0f, fz = 0.0f, kj = kNeverCandidate, kj32 = kNeverCandidate;
    if (j < n) {
        const float4 s = in[j];
        sph[j] = make_float4(s.x, s.y, s.z, s.w * s.w);
        cr[j] = s;
        invr[j] = 1.0f / s.w;
        const rt3_material m = mats[j];
        if (m.kind == RT3_MAT_DIELECTRIC) {                         // pack_material()
            const float ri_f = 1.0f / m.param, ri_b = m.param;
            const float r0f = (1.0f - ri_f) / (1.0f + ri_f), r0b = (1.0f - ri_b) / (1.0f + ri_b);
            mat[j] = make_float4(ri_f, r0f * r0f, r0b * r0b, m.param);
        } else mat[j] = make_float4(m.rgb[0], m.rgb[1], m.rgb[2], m.param);
        kind[j] = m.kind;
        bool is_direct = false;
        for (uint32_t k = 0; k < direct.n; k++) is_direct |= direct.id[k] == j;
        if (!is_direct) {
            fx = (float)((double)s.x - ecx); fy = (float)((double)s.y - ecy); fz = (float)((double)s.z - ecz);
            const double c2 = (double)fx * fx + (double)fy * fy + (double)fz * fz, r2 = (double)s.w * s.w;
            kj = filter_kj(c2, r2); kj32 = filter_kj32(c2, r2);
        }
    } else if (j < (n + 3u) / 4u * 4u) sph[j] = kPadSphere;
    uint32_t fr[4][2][4], fr32[4][4];
    bound_frag_row(fx, fy, fz, kj, fr);
    bound_frag32_row(fx, fy, fz, kj32, fr32);
    for (uint32_t q = 0; q < 4; q++)
        for (uint32_t hh = 0; hh < 2; hh++)
            frag[((size_t)(j / 32) * 4 + q) * 64 + hh * 32 + frag_row_of(j % 32)] = u32x4{ fr[q][hh][0], fr[q][hh][1], fr[q][hh][2], fr[q][hh][3] };
    for (uint32_t g = 0; g < 4; g++) frag32[frag32_index(j / 32, j % 32, g)] = u32x4{ fr32[g][0], fr32[g][1], fr32[g][2], fr32[g][3] };
}

}  // namespace
