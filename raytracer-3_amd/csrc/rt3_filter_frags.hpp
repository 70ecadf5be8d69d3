// rt3_filter_frags.hpp — what the scene build and the trace kernels must agree on: the SPHERE side of the matrix filter's operands (one bounding sphere as
// bf16 fragments, host and device, in each of the filter's three forms; the ray side and the derivation: rt3_matrix_filter.hpp), the margins, the
// group sizes of the multi-level rows and the pair lists' row limit.  No kernel: rt3_device.hip includes it in front of rt3_matrix_filter.hpp, rt3_scene.hip
// in front of the scene kernels (k_commit_mesh, k_group_frags, k_refit_rows, k_refit_spheres, k_build_spheres encode with it).
#pragma once

namespace {

constexpr float    kFilterEps = 2e-5f;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// row of the A operand that holds sphere b (0..31) of a row block (the K-slot layout: rt3_matrix_filter.hpp)
__host__ __device__ constexpr uint32_t frag_row_of(uint32_t b) { return ((15u - (b & 15u)) & 3u) + 8u * ((15u - (b & 15u)) >> 2) + 4u * (b >> 4); }

__host__ __device__ inline uint32_t bf16_rn(float x) {            // round to nearest even, finite inputs
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}
__host__ __device__ inline float bf16_up(uint32_t h) { return __builtin_bit_cast(float, h << 16); }
__host__ __device__ inline void split3(float x, uint32_t* parts /*[3]*/) {
    parts[0] = bf16_rn(x);
    const float r1 = x - bf16_up(parts[0]);
    parts[1] = bf16_rn(r1);
    parts[2] = bf16_rn(r1 - bf16_up(parts[1]));
}

// Sphere-side (A operand) fragment of one bounding sphere: out[q][hh][dword] = K elements 8 hh .. 8 hh + 7 of MFMA operand q.
// kj = filter_kj(|C|^2, r^2); a padding row uses C = 0, kj = -1e30 (never a candidate), an unbounded one kj = +1e30 (always).
__host__ __device__ inline void bound_frag_row(float cx, float cy, float cz, float kj, uint32_t out[4][2][4]) {
    uint32_t y[9][3], k[3];                                         // [term][part]
    const double x = cx, yy = cy, z = cz;
    split3((float)(x * x), y[0]); split3((float)(yy * yy), y[1]); split3((float)(z * z), y[2]);
    split3((float)(x * yy), y[3]); split3((float)(x * z), y[4]); split3((float)(yy * z), y[5]);
    split3(cx, y[6]); split3(cy, y[7]); split3(cz, y[8]);
    split3(kj, k);
    const uint32_t one = 0x3F80u;
    auto pk = [](uint32_t lo, uint32_t hi) { return lo | (hi << 16); };
    for (int i = 0; i < 4; i++) {
        for (int q = 0; q < 3; q++) out[q][0][i] = pk(y[2 * i][q], y[2 * i + 1][q]);
        for (int q = 0; q < 2; q++) out[q][1][i] = pk(y[2 * i][q], y[2 * i + 1][q]);
        out[2][1][i] = pk(y[2 * i][0], y[2 * i + 1][0]);
    }
    for (int i = 0; i < 3; i++) out[3][0][i] = pk(y[8][i], k[i]);
    out[3][0][3] = pk(y[8][0], one);
    out[3][1][0] = pk(y[8][1], one);
    out[3][1][1] = pk(y[8][0], one);
    out[3][1][2] = 0u; out[3][1][3] = 0u;
}
__host__ __device__ inline float filter_kj(double c2, double r2) { return (float)((r2 - c2) + (double)kFilterEps * (c2 + r2)); }
constexpr float kNeverCandidate = -1e30f, kAlwaysCandidate = 1e30f;
#ifndef RT3_FACE_K32
#define RT3_FACE_K32 1                                               // 1: faces go through the K = 32 form like the spheres (fragments: k_commit_mesh);
#endif                                                              // 0: the K = 64 16x16x32 form (A/B reference; tools/filter_probe measures both)

// The K = 64 filter on v_mfma_f32_16x16x32_bf16, sphere side: out[q][g][dword] = K-slots 32 q + 8 g .. + 7 of one row (kj, never / always: as bound_frag_row).
__host__ __device__ inline void bound_frag16_row(float cx, float cy, float cz, float kj, uint32_t out[2][4][4]) {
    uint32_t y[9][3], k[3];                                         // [term][part]
    const double x = cx, yy = cy, z = cz;
    split3((float)(x * x), y[0]); split3((float)(yy * yy), y[1]); split3((float)(z * z), y[2]);
    split3((float)(x * yy), y[3]); split3((float)(x * z), y[4]); split3((float)(yy * z), y[5]);
    split3(cx, y[6]); split3(cy, y[7]); split3(cz, y[8]);
    split3(kj, k);
    const uint32_t one = 0x3F80u;
    uint32_t slot[64];
    const int part_of_group[6] = { 0, 1, 2, 0, 1, 0 };              // sphere part of groups A..F
    for (int grp = 0; grp < 6; grp++) {
        for (int t = 0; t < 9; t++) slot[10 * grp + t] = y[t][part_of_group[grp]];
        slot[10 * grp + 9] = grp < 3 ? k[grp] : one;
    }
    for (int i = 60; i < 64; i++) slot[i] = 0u;
    for (int q = 0; q < 2; q++)
        for (int g = 0; g < 4; g++)
            for (int d = 0; d < 4; d++) out[q][g][d] = slot[32 * q + 8 * g + 2 * d] | (slot[32 * q + 8 * g + 2 * d + 1] << 16);
}
// where the fragment of (row block, row b of it, q, lane group g) lives: [blk][operand 2 h + q][lane 16 g + c]
__host__ __device__ constexpr size_t frag16_index(uint32_t blk, uint32_t b, uint32_t q, uint32_t g) {
    return ((size_t)blk * 4 + 2u * (b >> 4) + q) * 64 + 16u * g + (b & 15u);
}

// The K = 32 form (every default kernel), sphere side.
constexpr float kFilterEps32 = 2.2e-4f;
__host__ __device__ inline float filter_kj32(double c2, double r2) { return (float)((r2 - c2) + (double)kFilterEps32 * (c2 + r2)); }
__host__ __device__ inline uint32_t bf16_ceil(float x) {           // smallest bf16 >= x (finite x)
    uint32_t u = __builtin_bit_cast(uint32_t, x) & 0xFFFF0000u;     // towards zero
    if (x > 0.0f && __builtin_bit_cast(float, u) < x) u += 0x10000u;
    return u >> 16;
}
// Sphere side: out[g][dword] = K-slots 8 g .. 8 g + 7 of one row; (cx, cy, cz) are already relative to the filter centre.
__host__ __device__ inline void bound_frag32_row(float cx, float cy, float cz, float kj, uint32_t out[4][4]) {
    uint32_t y[9][3], k[2];
    const double x = cx, yy = cy, z = cz;
    split3((float)(x * x), y[0]); split3((float)(yy * yy), y[1]); split3((float)(z * z), y[2]);
    split3((float)(x * yy), y[3]); split3((float)(x * z), y[4]); split3((float)(yy * z), y[5]);
    split3(cx, y[6]); split3(cy, y[7]); split3(cz, y[8]);
    k[0] = bf16_rn(kj);
    k[1] = bf16_ceil(kj - bf16_up(k[0]));                           // H K + M K >= kj: what the dropped low part would add stays on the safe side
    const uint32_t one = 0x3F80u;
    uint32_t slot[32];
    for (int t = 0; t < 9; t++) { slot[t] = y[t][0]; slot[10 + t] = y[t][1]; slot[20 + t] = y[t][0]; }
    slot[9] = k[0]; slot[19] = k[1]; slot[29] = one; slot[30] = one; slot[31] = one;
    for (int g = 0; g < 4; g++)
        for (int d = 0; d < 4; d++) out[g][d] = slot[8 * g + 2 * d] | (slot[8 * g + 2 * d + 1] << 16);
}
__host__ __device__ constexpr size_t frag32_index(uint32_t blk, uint32_t b, uint32_t g) {       // [blk][h][16 g + c]
    return ((size_t)blk * 2 + (b >> 4)) * 64 + 16u * g + (b & 15u);
}

constexpr uint32_t kPairLaneShift = 26;                             // pair = lane << 26 | primitive row (< 2^26): the pair lists bound a scene's size (check_scene)

// Group sizes of the faces' / spheres' rows and the leaf groups per row (the GT, GS and SUP of k_trace_mfma_tiled, rt3_matrix_filter.hpp).
#ifndef RT3_GROUP_TRI
#define RT3_GROUP_TRI 8
#endif
#ifndef RT3_GROUP_SPH
#define RT3_GROUP_SPH 8
#endif
#ifndef RT3_SUPER
#define RT3_SUPER 8                                                 // leaf groups per row of the matrix filter (1: two levels, rows = leaf groups)
#endif
constexpr uint32_t kGroupTri = RT3_GROUP_TRI, kGroupSph = RT3_GROUP_SPH, kSuper = RT3_SUPER;
constexpr uint32_t kLevFan = 8;                                     // children per node at every level (kGroupTri = kGroupSph = kSuper = 8)

}  // namespace
