// rt3_scene.hip — everything that puts a scene on the context or changes it: the mesh staging calls and rt3_mesh_commit, the full
// uploads from host and from device arrays, refit (rt3_update_*), regroup (rt3_regroup*), the rows of the multi-level filter, the environment map,
// image textures and their bindings, and the two sampling tables.  It talks to the render unit (rt3_device.hip) through struct rt3_ctx alone; the few
// functions that unit calls are declared in rt3_scene.hpp.  No trace kernel is compiled here.
//
//   rt3_kernel_common.hpp   constants and arithmetic helpers (no kernel)
//   rt3_filter_frags.hpp    the sphere side of the matrix filter's operands, the group sizes (no kernel; shared with rt3_device.hip)
//   rt3_shared_kernels.hpp  k_fill_words and block_sum (shared with rt3_device.hip: a copy per unit)
//   rt3_scene_kernels.hpp   HIP equivalents of the pre-render shaders and of the merge; the rows' bounds and fragments; the refit
//   rt3_regroup.hpp         the group order of the multi-level filter again on the device (rt3_regroup*): the median split as stable sorts,
//                           in LDS for parts of up to 4096 primitives
//   rt3_scene_build.hpp     a full upload from device arrays (rt3_set_spheres_device / rt3_set_mesh_device): validation, the medians, the direct
//                           list and the ordered compaction into the initial group order
//   rt3_env_table.hpp       the environment map's sampling table
//   rt3_light_table.hpp     the emitters' sampling table
//   rt3_sphere_plan.hpp     host: the filter centre and the direct list of a sphere upload (shared with rt3_host.cpp)
//
// Compiled with -ffp-contract=off, as every unit of the library.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "rt3_scene.hpp"                                            // (rt3_ctx.hpp, rt3.h)
#include "rt3_sphere_plan.hpp"
#include "rt3_env_sample.hpp"
#include "rt3_light_sample.hpp"
#include "rt3_texture_law.hpp"
#include "rt3_kernel_common.hpp"
#include "rt3_filter_frags.hpp"
#include "rt3_shared_kernels.hpp"
#include "rt3_scene_kernels.hpp"
#include "rt3_regroup.hpp"
#include "rt3_scene_build.hpp"
#include "rt3_env_table.hpp"
#include "rt3_light_table.hpp"

namespace {

// Device form of a material: (rgb, param), except for a dielectric, whose attenuation is 1 and whose per-hit constants are
// precomputed here with the float operations of DESIGN.md §4.5: (1/ior, r0 for ri = 1/ior, r0 for ri = ior, ior), r0 = ((1-ri)/(1+ri))^2.
float4 pack_material(const rt3_material& m) {
    if (m.kind != RT3_MAT_DIELECTRIC) return make_float4(m.rgb[0], m.rgb[1], m.rgb[2], m.param);
    const float ri_f = 1.0f / m.param, ri_b = m.param;
    float r0f = (1.0f - ri_f) / (1.0f + ri_f), r0b = (1.0f - ri_b) / (1.0f + ri_b);
    r0f = r0f * r0f; r0b = r0b * r0b;
    return make_float4(ri_f, r0f, r0b, m.param);
}

// Sphere-side operand fragments of the matrix filter: [row block of 32 spheres][4 MFMA operands][64 lanes] x 8 bf16.
// Lane l holds, for operand row (l & 31) — sphere b of the block sits in row frag_row_of(b) — K elements 8 (l >> 5) .. +7;
// padding rows can never be candidates.  Coordinates relative to `centre` (sphere_filter_centre: it keeps |C|^2 + |o|^2, and with it the
// filter's margin, small for a scene that is not built around the world origin).
// Rows of `direct` spheres (sphere_direct_list below) can never be candidates: the kernels test those spheres for every ray anyway.
bool is_direct(uint32_t j, const uint32_t* direct, uint32_t n_direct) {
    for (uint32_t i = 0; i < n_direct; i++) if (direct[i] == j) return true;
    return false;
}
std::vector<uint32_t> build_sphere_frags(const float* center_radius, uint32_t n, const float centre[3], const uint32_t* direct, uint32_t n_direct) {
    const uint32_t blocks = (n + 31u) / 32u;
    std::vector<uint32_t> out((size_t)blocks * 4 * 64 * 4, 0u);
    for (uint32_t j = 0; j < blocks * 32; j++) {
        uint32_t fr[4][2][4];
        if (j < n && !is_direct(j, direct, n_direct)) {
            const float* s = center_radius + 4 * (size_t)j;
            const float cx = (float)((double)s[0] - centre[0]), cy = (float)((double)s[1] - centre[1]), cz = (float)((double)s[2] - centre[2]);
            const double c2 = (double)cx * cx + (double)cy * cy + (double)cz * cz, r2 = (double)s[3] * s[3];
            bound_frag_row(cx, cy, cz, filter_kj(c2, r2), fr);
        } else bound_frag_row(0.0f, 0.0f, 0.0f, kNeverCandidate, fr);
        for (int q = 0; q < 4; q++)
            for (int hh = 0; hh < 2; hh++)
                std::memcpy(&out[((((size_t)(j / 32) * 4 + q) * 64) + hh * 32 + frag_row_of(j % 32)) * 4], fr[q][hh], 16);
    }
    return out;
}

// The same spheres as fragments of the K = 32 form of the tiled kernels (rt3_matrix_filter.hpp): [row block][h][lane 16 g + c] x 8 bf16,
// coordinates relative to the same centre.
std::vector<uint32_t> build_sphere_frags32(const float* center_radius, uint32_t n, const float centre[3], const uint32_t* direct, uint32_t n_direct) {
    const uint32_t blocks = (n + 31u) / 32u;
    std::vector<uint32_t> out((size_t)blocks * 2 * 64 * 4, 0u);
    for (uint32_t j = 0; j < blocks * 32; j++) {
        uint32_t fr[4][4];
        if (j < n && !is_direct(j, direct, n_direct)) {
            const float* s = center_radius + 4 * (size_t)j;
            const float cx = (float)((double)s[0] - centre[0]), cy = (float)((double)s[1] - centre[1]), cz = (float)((double)s[2] - centre[2]);
            const double c2 = (double)cx * cx + (double)cy * cy + (double)cz * cz, r2 = (double)s[3] * s[3];
            bound_frag32_row(cx, cy, cz, filter_kj32(c2, r2), fr);
        } else bound_frag32_row(0.0f, 0.0f, 0.0f, kNeverCandidate, fr);
        for (uint32_t g = 0; g < 4; g++) std::memcpy(&out[frag32_index(j / 32, j % 32, g) * 4], fr[g], 16);
    }
    return out;
}

// sphere_filter_centre / sphere_direct_list (the filter's centre, the directly tested spheres): rt3_sphere_plan.hpp

// Group order for the two-level filter: a median split of the centres along the longest axis of their box, repeated until a
// part holds at most `group` primitives; the left part of every split is a multiple of `group`, so that only the very last group is short.
// Consecutive runs of `group` entries of the result are the groups; 0xFFFFFFFF pads the last one.  Spheres on the `direct` list (tested for
// every ray anyway) and spheres whose record is not finite (no exact test can accept them) stay out.
// Any order is correct — the nearest-hit key carries the sphere's own index, and the minimum over the keys does not depend on the order the
// pairs are tested in — a compact one keeps the groups' bounding spheres small.
void median_split_order(std::vector<uint32_t>& ids, const float* xyz_stride4, uint32_t group, uint32_t super = 1) {
    struct Part { size_t begin, end; };
    std::vector<Part> stack;
    stack.push_back({ 0, ids.size() });
    while (!stack.empty()) {
        const Part part = stack.back();
        stack.pop_back();
        const size_t count = part.end - part.begin;
        if (count <= group) continue;
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (size_t k = part.begin; k < part.end; k++)
            for (int a = 0; a < 3; a++) { const float c = xyz_stride4[4 * (size_t)ids[k] + a]; lo[a] = std::min(lo[a], c); hi[a] = std::max(hi[a], c); }
        int axis = 0;
        for (int a = 1; a < 3; a++) if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;
        // parts larger than a super group (group x super primitives: one row of the three-level filter) split at multiples of it, so that the
        // `super` leaf groups of a row are one part of the split
        const size_t unit = count > (size_t)group * super ? (size_t)group * super : group;
        size_t half = (count / 2 + unit - 1) / unit * unit;
        if (half >= count) half = count - unit;                     // (count > unit here)
        std::nth_element(ids.begin() + part.begin, ids.begin() + part.begin + half, ids.begin() + part.end,
                         [&](uint32_t x, uint32_t y) { return xyz_stride4[4 * (size_t)x + axis] < xyz_stride4[4 * (size_t)y + axis]; });
        stack.push_back({ part.begin + half, part.end });
        stack.push_back({ part.begin, part.begin + half });
    }
}
std::vector<uint32_t> sphere_group_order(const float* center_radius, uint32_t n, const uint32_t* direct, uint32_t n_direct, uint32_t group, uint32_t super) {
    std::vector<uint32_t> ids;
    ids.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        const float* s = center_radius + 4 * (size_t)i;
        if (is_direct(i, direct, n_direct) || !std::isfinite(s[0]) || !std::isfinite(s[1]) || !std::isfinite(s[2]) || !std::isfinite(s[3] * s[3])) continue;
        ids.push_back(i);
    }
    median_split_order(ids, center_radius, group, super);
    ids.resize((ids.size() + group * super - 1) / (group * super) * (group * super), 0xFFFFFFFFu);
    return ids;
}
// The same for faces, from their bounding spheres (cx, cy, cz, r^2 as k_commit_mesh wrote them): a mesh may list its faces in any order (the
// reference's teddy.obj does), and groups of faces that merely follow each other in the file would span the model.  Faces without a bounded hit
// region (r^2 >= 3e38: always candidates) go last, in groups of their own, so that they make only their own rows always-candidates.
std::vector<uint32_t> face_group_order(const float4* bounds, uint32_t n, uint32_t group, uint32_t super) {
    std::vector<uint32_t> ids, unbounded;
    ids.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        const float4 b = bounds[i];
        if (std::isfinite(b.x) && std::isfinite(b.y) && std::isfinite(b.z) && b.w >= 0.0f && b.w < 3e38f) ids.push_back(i);
        else unbounded.push_back(i);
    }
    median_split_order(ids, reinterpret_cast<const float*>(bounds), group, super);
    ids.resize((ids.size() + group * super - 1) / (group * super) * (group * super), 0xFFFFFFFFu);
    ids.insert(ids.end(), unbounded.begin(), unbounded.end());
    ids.resize((ids.size() + group * super - 1) / (group * super) * (group * super), 0xFFFFFFFFu);
    return ids;
}

uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }
dim3 build_grid(uint32_t threads) { return dim3((threads + kBlock - 1) / kBlock); }     // one thread per item, blocks of kBlock

// The buffers and counts of the rows of the multi-level filter for n_pos positions in groups of `group` — the one place that knows the
// levels' sizes: the members and their primitive indices, the leaf groups' bounds, the rows (kSuper leaves) and the super-rows (kSuper rows), each as f32
// records and as fragments, padded to row blocks of 32.  R is emptied first; a failure leaves it empty.  The caller fills grp and perm and writes the bounds.
int alloc_rows(rt3_ctx* ctx, FilterRows& R, uint32_t n_pos, uint32_t group) {
    static_assert(kSuper > 1, "alloc_rows: the three- and four-level rows");
    R = FilterRows();
    int rc;
    if ((rc = R.grp.alloc(ctx, n_pos)) || (rc = R.perm.alloc(ctx, n_pos))) return rc;
    const uint32_t n_leaves = n_pos / group, n_groups = n_leaves / kSuper;
    if (n_groups == 0) return 0;                                    // (spheres: every one is on the direct list or unusable)
    const uint32_t n_group_rows = round_up(n_groups, 32u), n_super = (n_groups + kSuper - 1u) / kSuper, n_super_rows = round_up(n_super, 32u);
    if ((rc = R.leaf.alloc(ctx, n_leaves)) || (rc = R.gfrag.alloc(ctx, (size_t)n_group_rows * 4)) || (rc = R.rowb.alloc(ctx, n_group_rows)) ||
        (rc = R.sfrag.alloc(ctx, (size_t)n_super_rows * 4)) || (rc = R.srowb.alloc(ctx, n_super_rows))) {
        R = FilterRows();
        return rc;
    }
    R.n_leaves = n_leaves; R.n_groups = n_groups; R.n_super = n_super;
    return 0;
}

// The rows over `members` ((cx, cy, cz, r^2) per primitive) in the group order `order`, groups of `group`, from host vectors: alloc_rows' buffers, the
// members and the order uploaded, then leaf bounds, row fragments, row bounds, super-row fragments and bounds.  Filter coordinates are about the centre
// of the vertex box `box` (faces) or, box = nullptr, about `centre` (spheres).  A failure leaves no rows.  The launches are on ctx->stream; the caller
// synchronises.
int build_rows(rt3_ctx* ctx, FilterRows& R, const float4* members, const std::vector<uint32_t>& order, uint32_t group, const uint32_t* box,
               const float centre[3]) {
    std::vector<float4> grp(order.size(), kPadSphere);
    for (size_t k = 0; k < order.size(); k++) if (order[k] != 0xFFFFFFFFu) grp[k] = members[order[k]];
    int rc;
    if ((rc = alloc_rows(ctx, R, (uint32_t)order.size(), group))) return rc;
    const auto fill = [&]() -> int {
        if (order.empty()) return 0;
        RT3_HIP(hipMemcpy(R.grp.get(), grp.data(), grp.size() * sizeof(float4), hipMemcpyHostToDevice));
        RT3_HIP(hipMemcpy(R.perm.get(), order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (R.n_groups == 0) return 0;
        const uint32_t n_entries = (uint32_t)order.size(), n_leaves = R.n_leaves, n_group_rows = (uint32_t)R.rowb.size(), n_super_rows = (uint32_t)R.srowb.size();
        const float cx = centre[0], cy = centre[1], cz = centre[2];
        const dim3 blk(kBlock);
        // three levels: the leaves' bounds are records of their own, a row bounds kSuper of them — as fragments and as f32 records
        hipLaunchKernelGGL(k_group_bounds, build_grid(n_leaves), blk, 0, ctx->stream, (const float4*)R.grp.get(), n_entries, group, n_leaves, box, cx, cy, cz, R.leaf.get());
        RT3_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_group_frags, build_grid(n_group_rows), blk, 0, ctx->stream, (const float4*)R.leaf.get(), n_leaves, kSuper, n_group_rows, box, cx, cy, cz, R.gfrag.get());
        RT3_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_group_bounds, build_grid(n_group_rows), blk, 0, ctx->stream, (const float4*)R.leaf.get(), n_leaves, kSuper, n_group_rows, box, cx, cy, cz, R.rowb.get());
        RT3_HIP(hipGetLastError());
        // four levels: super-rows of kSuper rows, as fragments for the matrix filter and as f32 records
        hipLaunchKernelGGL(k_group_frags, build_grid(n_super_rows), blk, 0, ctx->stream, R.rowb.get(), n_group_rows, kSuper, n_super_rows, box, cx, cy, cz, R.sfrag.get());
        hipLaunchKernelGGL(k_group_bounds, build_grid(n_super_rows), blk, 0, ctx->stream, R.rowb.get(), n_group_rows, kSuper, n_super_rows, box, cx, cy, cz, R.srowb.get());
        RT3_HIP(hipGetLastError());
        return 0;
    };
    if ((rc = fill())) R = FilterRows();
    return rc;
}

// The same rows again for members that moved (rt3_update_*): R.grp holds the new member records, every bound above them is
// recomputed into the buffers build_rows allocated — k_refit_rows, one launch per level (leaves, rows, super-rows), each bound evaluated once.
// RT3_REFIT_SIMPLE=1 issues build_rows' own five launches instead (A/B reference: the same bits).  Nothing is allocated, nothing waits.
int refit_rows(rt3_ctx* ctx, const FilterRows& R, const uint32_t* box, const float centre[3], hipStream_t stream) {
    static_assert(kSuper == kLevFan && kGroupTri == kLevFan && kGroupSph == kLevFan, "refit_rows: the three-level rows, 8 children per node");
    if (R.n_groups == 0) return 0;
    const uint32_t n_entries = (uint32_t)R.grp.size(), n_leaves = R.n_leaves, n_group_rows = (uint32_t)R.rowb.size(), n_super_rows = (uint32_t)R.srowb.size();
    const float cx = centre[0], cy = centre[1], cz = centre[2];
    const dim3 blk(kBlock);
    if (getenv("RT3_REFIT_SIMPLE")) {
        hipLaunchKernelGGL(k_group_bounds, build_grid(n_leaves), blk, 0, stream, R.grp.get(), n_entries, kLevFan, n_leaves, box, cx, cy, cz, R.leaf.get());
        hipLaunchKernelGGL(k_group_frags, build_grid(n_group_rows), blk, 0, stream, R.leaf.get(), n_leaves, kLevFan, n_group_rows, box, cx, cy, cz, R.gfrag.get());
        hipLaunchKernelGGL(k_group_bounds, build_grid(n_group_rows), blk, 0, stream, R.leaf.get(), n_leaves, kLevFan, n_group_rows, box, cx, cy, cz, R.rowb.get());
        hipLaunchKernelGGL(k_group_frags, build_grid(n_super_rows), blk, 0, stream, R.rowb.get(), n_group_rows, kLevFan, n_super_rows, box, cx, cy, cz, R.sfrag.get());
        hipLaunchKernelGGL(k_group_bounds, build_grid(n_super_rows), blk, 0, stream, R.rowb.get(), n_group_rows, kLevFan, n_super_rows, box, cx, cy, cz, R.srowb.get());
    } else {
        hipLaunchKernelGGL(k_refit_rows, build_grid(n_leaves * kLevFan), blk, 0, stream, R.grp.get(), n_entries, n_leaves, box, cx, cy, cz, R.leaf.get(), (u32x4*)nullptr);
        hipLaunchKernelGGL(k_refit_rows, build_grid(n_group_rows * kLevFan), blk, 0, stream, R.leaf.get(), n_leaves, n_group_rows, box, cx, cy, cz, R.rowb.get(), R.gfrag.get());
        hipLaunchKernelGGL(k_refit_rows, build_grid(n_super_rows * kLevFan), blk, 0, stream, R.rowb.get(), n_group_rows, n_super_rows, box, cx, cy, cz, R.srowb.get(), R.sfrag.get());
    }
    RT3_HIP(hipGetLastError());
    return 0;
}

// A full upload of a class drops its texture binding: the set of slots it names, whatever d_*_tex still holds.
void drop_sphere_binding(rt3_ctx* ctx) { std::memset(ctx->sph_tex_used, 0, sizeof ctx->sph_tex_used); }
void drop_mesh_binding(rt3_ctx* ctx) { std::memset(ctx->tri_tex_used, 0, sizeof ctx->tri_tex_used); }

void clear_spheres(rt3_ctx* ctx) {                           // what rt3_set_spheres(n = 0) leaves
    ctx->n_sph = 0; ctx->n_direct = 0; ctx->sph_left_out = false; ctx->light_table = false;
    drop_sphere_binding(ctx);
    for (int a = 0; a < 3; a++) ctx->sph_centre[a] = 0.0f;
    ctx->sph = FilterRows();
    for (DevBuf<float4>* b : { &ctx->d_sph, &ctx->d_sph_mat, &ctx->d_sph_cr }) b->reset();
    for (DevBuf<uint32_t>* b : { &ctx->d_sph_frag, &ctx->d_sph_frag32, &ctx->d_sph_kind, &ctx->d_sph_slot }) b->reset();
    ctx->d_sph_invr.reset();
}
void clear_mesh(rt3_ctx* ctx) {                              // what rt3_mesh_commit drops before it builds: no mesh
    ctx->n_faces = 0; ctx->mesh_in_sync = false; ctx->update_error_pending = false; ctx->tri_bounded = 0; ctx->light_table = false;
    drop_mesh_binding(ctx);
    ctx->tri = FilterRows();
    for (DevBuf<float4>* b : { &ctx->d_tri, &ctx->d_tri_mat, &ctx->d_tri_bound, &ctx->d_tri_rec }) b->reset();
    ctx->d_tri_kind.reset(); ctx->d_tri_frag.reset(); ctx->d_tri_frag_r.reset(); ctx->d_face_mats_in.reset();
}

// The render layout of n faces from merged entity buffers: the box of the vertices — its centre is what the faces' filter coordinates are taken about
// (k_commit_mesh and the ray side agree on it through box_centre()) — then k_commit_mesh twice, everything about that centre and Mode R's fragments.
// Mode R's rays all start at the world origin, the path tracer's mostly ON the scene: the filter's margin eps (|C - c|^2 + r^2 + |o - c|^2) is smallest
// about the point half-way to the mesh here and about the mesh's own centre there.  Mode R therefore keeps fragments of its own, built by the same
// kernel (with centre_scale 0.5 it writes nothing else) while the merged entity buffers are known to be the ones these faces came from: a render never
// reads d_gfaces / d_verts, so an rt3_mesh_begin without a commit leaves the committed scene renderable.
// The destinations are the caller's: rt3_mesh_commit's are the context's buffers, rt3_set_mesh_device's ones the context does not hold yet.  error: the
// word a face with a vertex index out of range sets.
int render_layout(rt3_ctx* ctx, const rt3_gface* gfaces, const float4* verts, uint32_t n, uint32_t n_verts, const rt3_material* mats, float4* tri, float4* tri_bound,
                  float4* tri_mat, uint32_t* tri_kind, u32x4* tri_frag, u32x4* tri_frag_r, uint32_t* box, uint32_t* error, hipStream_t stream) {
    const uint32_t n_pad = (n + 3u) / 4u * 4u, n_frag_rows = (n + 31u) / 32u * 32u;
    RT3_HIP(hipMemsetAsync(box, 0xFF, 3 * sizeof(uint32_t), stream));
    RT3_HIP(hipMemsetAsync(box + 3, 0, 3 * sizeof(uint32_t), stream));
    if (n_verts) hipLaunchKernelGGL(k_vertex_box, dim3(std::min<uint32_t>(256u, build_grid(n_verts).x)), dim3(kBlock), 0, stream, verts, n_verts, box);
    RT3_HIP(hipGetLastError());
    for (const float scale : { 1.0f, 0.5f }) {
        hipLaunchKernelGGL(k_commit_mesh, build_grid(n_frag_rows), dim3(kBlock), 0, stream, gfaces, verts, n, n_pad, n_verts, mats, tri, tri_bound, tri_mat,
                           tri_kind, error, scale == 1.0f ? tri_frag : tri_frag_r, n_frag_rows, (const uint32_t*)box, scale);
        RT3_HIP(hipGetLastError());
    }
    return 0;
}

// One sampling table of n entries: three launches queued on the calling entry point's stream behind enter() — the two of launches(grid, block): the
// entries' weights into q and their maximum into d_env_wmax, then q and cdf quantised from both; and the prefix sums of cdf in place (integers: order-free) —
// with no host wait: the kernels read the total from the last prefix sum.  d_env_wmax and d_env_temp (the scan's scratch) are shared by both tables: the
// builds are queued behind the event chain, where a later call on another stream finds the table as it finds an update.
template <class Launches>
int build_sampling_table(rt3_ctx* ctx, uint32_t n, DevBuf<uint32_t>& q, DevBuf<unsigned long long>& cdf, hipStream_t stream, Launches launches) {
    size_t temp = 0;
    int rc;
    RT3_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, temp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n, stream));
    if ((rc = q.ensure(ctx, n)) || (rc = cdf.ensure(ctx, n)) || (rc = ctx->d_env_wmax.ensure(ctx, 1)) || (rc = ctx->d_env_temp.ensure(ctx, std::max<size_t>(temp, 1))))
        return rc;
    RT3_HIP(hipMemsetAsync(ctx->d_env_wmax, 0, 4, stream));
    launches(build_grid(n), dim3(kBlock));
    RT3_HIP(hipGetLastError());
    RT3_HIP(hipcub::DeviceScan::InclusiveSum(ctx->d_env_temp.get(), temp, (const unsigned long long*)cdf.get(), cdf.get(), (int)n, stream));
    return 0;
}

}  // namespace

// ---- What the render unit calls (rt3_scene.hpp)
// A scene the trace kernels can take: renders and queries need one, and the pair lists address at most 2^kPairLaneShift - 32 rows.
int check_scene(rt3_ctx* ctx) {
    if (ctx->n_sph == 0 && ctx->n_faces == 0) return fail(ctx, RT3_E_STATE, "no scene: call rt3_set_spheres / rt3_set_mesh first");
    if (ctx->n_faces >= (1u << kPairLaneShift) - 32u || ctx->n_sph >= (1u << kPairLaneShift) - 32u) return fail(ctx, RT3_E_ARG, "too many primitives");
    return 0;
}
// The sampling table of the map the context holds, built once per map by the first call that carries RT3_FLAG_ENV_SAMPLING.
int ensure_env_table(rt3_ctx* ctx, hipStream_t stream) {
    if (ctx->env_table) return 0;
    const uint32_t m = rt3env::cells_per_edge(ctx->env_n), cells = 6u * m * m;
    const int rc = build_sampling_table(ctx, cells, ctx->d_env_q, ctx->d_env_cdf, stream, [&](dim3 grid, dim3 blk) {
        hipLaunchKernelGGL(k_env_cell_weights, grid, blk, 0, stream, (const float4*)ctx->d_env, ctx->env_n, m, cells, ctx->d_env_q.get(), ctx->d_env_wmax.get());
        hipLaunchKernelGGL(k_env_quantise, grid, blk, 0, stream, cells, (const uint32_t*)ctx->d_env_wmax, ctx->d_env_q.get(), ctx->d_env_cdf.get());
    });
    if (!rc) { ctx->env_m = m; ctx->env_table = true; }
    return rc;
}
// The emitters' table of the scene the context holds, one entry per primitive, built by the first call with RT3_FLAG_LIGHT_SAMPLING.
int ensure_light_table(rt3_ctx* ctx, hipStream_t stream) {
    if (ctx->light_table) return 0;
    const uint32_t n = ctx->n_faces + ctx->n_sph;                   // (check_scene: >= 1, and far below 2^31)
    const int rc = build_sampling_table(ctx, n, ctx->d_light_q, ctx->d_light_cdf, stream, [&](dim3 grid, dim3 blk) {
        hipLaunchKernelGGL(k_light_weights, grid, blk, 0, stream, (const float4*)ctx->d_tri, (const float4*)ctx->d_tri_mat, (const uint32_t*)ctx->d_tri_kind, ctx->n_faces,
                           (const float4*)ctx->d_sph_cr, (const float4*)ctx->d_sph_mat, (const uint32_t*)ctx->d_sph_kind, ctx->n_sph, ctx->d_light_q.get(),
                           ctx->d_env_wmax.get());
        hipLaunchKernelGGL(k_light_quantise, grid, blk, 0, stream, n, (const uint32_t*)ctx->d_env_wmax, ctx->d_light_q.get(), ctx->d_light_cdf.get());
    });
    if (!rc) ctx->light_table = true;
    return rc;
}

extern "C" {

int rt3_mesh_begin(rt3_ctx* ctx, uint32_t n_faces, uint32_t n_vertices) {
    if (!ctx) return RT3_E_ARG;
    RT3_HIP(hipSetDevice(ctx->device));
    ctx->mesh_in_sync = false;
    int rc;
    if ((rc = ctx->d_gfaces.alloc(ctx, n_faces)) || (rc = ctx->d_verts.alloc(ctx, n_vertices))) return rc;
    if (n_faces) RT3_HIP(hipMemsetAsync(ctx->d_gfaces, 0, (size_t)n_faces * sizeof(rt3_gface), ctx->stream));
    if (n_vertices) RT3_HIP(hipMemsetAsync(ctx->d_verts, 0, (size_t)n_vertices * sizeof(float4), ctx->stream));
    return 0;
}

int rt3_mesh_put(rt3_ctx* ctx, const rt3_gface* faces, uint32_t n_faces, const float* vertices, uint32_t n_vertices,
                 uint32_t face_offset, uint32_t vertex_offset) {
    if (!ctx) return RT3_E_ARG;
    if ((n_faces && !faces) || (n_vertices && !vertices)) return fail(ctx, RT3_E_ARG, "faces / vertices is NULL");
    if ((uint64_t)face_offset + n_faces > ctx->d_gfaces.size() || (uint64_t)vertex_offset + n_vertices > ctx->d_verts.size())
        return fail(ctx, RT3_E_ARG, "rt3_mesh_put: entity does not fit in the buffers sized by rt3_mesh_begin");
    RT3_HIP(hipSetDevice(ctx->device));
    ctx->mesh_in_sync = false;
    std::vector<rt3_gface> rebased(faces, faces + n_faces);         // transfer_entity: indices += running vertex count
    for (rt3_gface& f : rebased) { f.v1 += vertex_offset; f.v2 += vertex_offset; f.v3 += vertex_offset; }
    if (n_faces) RT3_HIP(hipMemcpyAsync(ctx->d_gfaces + face_offset, rebased.data(), (size_t)n_faces * sizeof(rt3_gface), hipMemcpyHostToDevice, ctx->stream));
    if (n_vertices) RT3_HIP(hipMemcpyAsync(ctx->d_verts + vertex_offset, vertices, (size_t)n_vertices * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    RT3_HIP(hipStreamSynchronize(ctx->stream));                     // `rebased` is a temporary
    return 0;
}

int rt3_mesh_sphere(rt3_ctx* ctx, const float center[3], float radius, uint32_t n_meridians, uint32_t n_parallels, const float color[3],
                    uint32_t face_offset, uint32_t vertex_offset) {
    if (!ctx) return RT3_E_ARG;
    if (!center || !color || n_meridians < 3 || n_parallels < 3) return fail(ctx, RT3_E_ARG, "rt3_mesh_sphere: need >= 3 meridians and parallels");
    const uint32_t nf = 2 * n_meridians * (n_parallels - 2), nv = 2 + (n_parallels - 2) * n_meridians;
    if ((uint64_t)face_offset + nf > ctx->d_gfaces.size() || (uint64_t)vertex_offset + nv > ctx->d_verts.size())
        return fail(ctx, RT3_E_ARG, "rt3_mesh_sphere: entity does not fit in the buffers sized by rt3_mesh_begin");
    RT3_HIP(hipSetDevice(ctx->device));
    ctx->mesh_in_sync = false;
    const SphereGen g{ center[0], center[1], center[2], radius, n_meridians, n_parallels, color[0], color[1], color[2], face_offset, vertex_offset };
    const dim3 blk(32, 8);
    hipLaunchKernelGGL(k_prerender_sphere_vertices, dim3((n_meridians + 31) / 32, (n_parallels + 7) / 8), blk, 0, ctx->stream, g, ctx->d_verts);
    RT3_HIP(hipGetLastError());
    // same stream: the faces kernel starts after the vertices are written (the barrier of Sphere.cpp:446-450)
    hipLaunchKernelGGL(k_prerender_sphere_faces, dim3((n_meridians + 31) / 32, (n_parallels - 1 + 7) / 8), blk, 0, ctx->stream, g, ctx->d_gfaces, ctx->d_verts);
    RT3_HIP(hipGetLastError());
    return 0;
}

int rt3_mesh_commit(rt3_ctx* ctx, const rt3_material* face_materials) {
    if (!ctx) return RT3_E_ARG;
    RT3_HIP(hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t)ctx->d_gfaces.size(), n_pad = (n + 3u) / 4u * 4u, n_frag_rows = (n + 31u) / 32u * 32u, n_verts = (uint32_t)ctx->d_verts.size();
    clear_mesh(ctx);                                                // (the scene changes, and a full upload drops the faces' texture binding)
    if (n == 0) return 0;
    if (face_materials)
        for (uint32_t i = 0; i < n; i++)
            if (face_materials[i].kind > RT3_MAT_DIELECTRIC) return fail(ctx, RT3_E_ARG, "unknown material kind");
    int rc;
    if ((rc = ctx->d_error.ensure(ctx, 1))) return rc;
    RT3_HIP(hipMemsetAsync(ctx->d_error, 0, 4, ctx->stream));
    if ((rc = ctx->d_tri.alloc(ctx, (size_t)n * 4)) || (rc = ctx->d_tri_mat.alloc(ctx, n)) || (rc = ctx->d_tri_kind.alloc(ctx, n)) ||
        (rc = ctx->d_tri_bound.alloc(ctx, n_pad)) || (rc = ctx->d_tri_frag.alloc(ctx, (size_t)n_frag_rows * 8)) ||      // 4 operands x 2 lane halves per row
        (rc = ctx->d_tri_frag_r.alloc(ctx, (size_t)n_frag_rows * 8)))
        return rc;
    if (face_materials) {
        if ((rc = ctx->d_face_mats_in.alloc(ctx, n))) return rc;
        RT3_HIP(hipMemcpyAsync(ctx->d_face_mats_in, face_materials, (size_t)n * sizeof(rt3_material), hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = ctx->d_box.ensure(ctx, 6)) ||
        (rc = render_layout(ctx, ctx->d_gfaces, ctx->d_verts, n, n_verts, ctx->d_face_mats_in, ctx->d_tri, ctx->d_tri_bound, ctx->d_tri_mat, ctx->d_tri_kind,
                            ctx->d_tri_frag, ctx->d_tri_frag_r, ctx->d_box, ctx->d_error, ctx->stream)))
        return rc;
    uint32_t err = 0, box[6];
    RT3_HIP(hipMemcpyAsync(&err, ctx->d_error, 4, hipMemcpyDeviceToHost, ctx->stream));
    RT3_HIP(hipMemcpyAsync(box, ctx->d_box, sizeof(box), hipMemcpyDeviceToHost, ctx->stream));
    RT3_HIP(hipStreamSynchronize(ctx->stream));
    box_centre(box, ctx->tri_centre);
    if (err) return fail(ctx, RT3_E_ARG, "a face references a vertex out of range");
    // rows of the multi-level filter: groups of kGroupTri faces in the order of a spatial median split of their bounds (read back once per
    // commit: 16 bytes per face); then the faces' records in group order
    std::vector<float4> bounds(n);
    RT3_HIP(hipMemcpy(bounds.data(), ctx->d_tri_bound, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    const std::vector<uint32_t> order = face_group_order(bounds.data(), n, kGroupTri, kSuper);
    ctx->tri_bounded = 0;                                           // the region rt3_regroup* reorders: face_group_order's own condition
    for (const float4& b : bounds) ctx->tri_bounded += std::isfinite(b.x) && std::isfinite(b.y) && std::isfinite(b.z) && b.w >= 0.0f && b.w < 3e38f;
    const float no_centre[3] = { 0.0f, 0.0f, 0.0f };
    if ((rc = build_rows(ctx, ctx->tri, bounds.data(), order, kGroupTri, ctx->d_box, no_centre))) return rc;
    if ((rc = ctx->d_tri_rec.alloc(ctx, order.size() * 4))) return rc;
    hipLaunchKernelGGL(k_gather_face_records, build_grid((uint32_t)order.size() * 4u), dim3(kBlock), 0, ctx->stream, (const float4*)ctx->d_tri,
                       (const uint32_t*)ctx->tri.perm, (uint32_t)order.size(), ctx->d_tri_rec.get());
    RT3_HIP(hipGetLastError());
    RT3_HIP(hipStreamSynchronize(ctx->stream));                     // a render may come on another stream
    ctx->n_faces = n;
    ctx->mesh_in_sync = true;
    return 0;
}

int rt3_mesh_download(rt3_ctx* ctx, rt3_gface* faces, float* vertices) {
    if (!ctx) return RT3_E_ARG;
    RT3_HIP(hipSetDevice(ctx->device));
    RT3_HIP(hipStreamSynchronize(ctx->stream));
    if (faces && ctx->d_gfaces.size()) RT3_HIP(hipMemcpy(faces, ctx->d_gfaces, ctx->d_gfaces.size() * sizeof(rt3_gface), hipMemcpyDeviceToHost));
    if (vertices && ctx->d_verts.size()) RT3_HIP(hipMemcpy(vertices, ctx->d_verts, ctx->d_verts.size() * sizeof(float4), hipMemcpyDeviceToHost));
    return 0;
}

int rt3_set_mesh(rt3_ctx* ctx, const rt3_gface* faces, uint32_t n_faces, const float* vertices, uint32_t n_vertices,
                 const rt3_material* face_materials) {
    if (!ctx) return RT3_E_ARG;
    if (n_faces != 0 && (!faces || !vertices)) return fail(ctx, RT3_E_ARG, "faces / vertices is NULL");
    int rc;
    if ((rc = rt3_mesh_begin(ctx, n_faces, n_vertices))) return rc;
    if ((rc = rt3_mesh_put(ctx, faces, n_faces, vertices, n_vertices, 0, 0))) return rc;
    return rt3_mesh_commit(ctx, face_materials);
}

int rt3_set_spheres(rt3_ctx* ctx, const float* center_radius, const rt3_material* materials, uint32_t n) {
    if (!ctx) return RT3_E_ARG;
    if (n != 0 && (!center_radius || !materials)) return fail(ctx, RT3_E_ARG, "center_radius / materials is NULL");
    RT3_HIP(hipSetDevice(ctx->device));
    if (n == 0) { clear_spheres(ctx); return 0; }
    std::vector<float4> sph(((size_t)n + 3) / 4 * 4, kPadSphere), mat(n), cr(n);          // scan works in groups of 4
    std::vector<float> invr(n);
    std::vector<uint32_t> kind(n);
    for (uint32_t i = 0; i < n; i++) {
        const float* s = center_radius + 4 * (size_t)i;
        if (!(s[3] > 0.0f)) return fail(ctx, RT3_E_ARG, "sphere " + std::to_string(i) + " has a non-positive radius");
        if (materials[i].kind > RT3_MAT_DIELECTRIC) return fail(ctx, RT3_E_ARG, "unknown material kind");
        sph[i] = make_float4(s[0], s[1], s[2], s[3] * s[3]);
        cr[i] = make_float4(s[0], s[1], s[2], s[3]);
        invr[i] = 1.0f / s[3];
        mat[i] = pack_material(materials[i]);
        kind[i] = materials[i].kind;
    }
    ctx->n_sph = 0;                                                 // (no spheres until everything below has been issued)
    ctx->light_table = false;
    drop_sphere_binding(ctx);                                       // a full upload: the spheres' texture binding goes with the old spheres
    int rc;
    sphere_filter_centre(center_radius, n, ctx->sph_centre);
    ctx->n_direct = sphere_direct_list(center_radius, n, ctx->sph_centre, ctx->direct);
    if ((rc = ctx->d_sph_frag.upload(ctx, build_sphere_frags(center_radius, n, ctx->sph_centre, ctx->direct, ctx->n_direct)))) return rc;      // k_trace_mfma (K = 64, 32x32x16)
    if ((rc = ctx->d_sph_frag32.upload(ctx, build_sphere_frags32(center_radius, n, ctx->sph_centre, ctx->direct, ctx->n_direct)))) return rc;  // K = 32 form
    if ((rc = ctx->d_sph.upload(ctx, sph)) || (rc = ctx->d_sph_invr.upload(ctx, invr)) || (rc = ctx->d_sph_mat.upload(ctx, mat)) ||
        (rc = ctx->d_sph_kind.upload(ctx, kind)) || (rc = ctx->d_sph_cr.upload(ctx, cr)))
        return rc;
    // rows of the multi-level filter: groups of kGroupSph spheres in the order of a spatial median split
    const std::vector<uint32_t> order = sphere_group_order(center_radius, n, ctx->direct, ctx->n_direct, kGroupSph, kSuper);
    if ((rc = build_rows(ctx, ctx->sph, sph.data(), order, kGroupSph, nullptr, ctx->sph_centre))) return rc;
    std::vector<uint32_t> slot(n, 0xFFFFFFFFu);                     // the inverse of the order (rt3_update_spheres*)
    uint32_t placed = 0;
    for (size_t k = 0; k < order.size(); k++) if (order[k] != 0xFFFFFFFFu) { slot[order[k]] = (uint32_t)k; placed++; }
    if ((rc = ctx->d_sph_slot.upload(ctx, slot))) return rc;
    ctx->sph_left_out = placed + ctx->n_direct != n;
    RT3_HIP(hipStreamSynchronize(ctx->stream));                     // a render may come on another stream
    ctx->n_sph = n;
    return 0;
}

// ---- Refit: new positions for the scene on the context, every derived buffer recomputed in place on the device
static int update_spheres_checks(rt3_ctx* ctx, const void* center_radius, uint32_t n) {
    if (!center_radius) return fail(ctx, RT3_E_ARG, "center_radius is NULL");
    if (ctx->n_sph == 0) return fail(ctx, RT3_E_STATE, "no spheres to update: call rt3_set_spheres first");
    if (ctx->sph_left_out)
        return fail(ctx, RT3_E_STATE, "the last rt3_set_spheres left a non-finite sphere out of the group order: it has no slot an update could fill");
    if (n != ctx->n_sph) return fail(ctx, RT3_E_ARG, "n must equal the context's sphere count");
    return 0;
}

int rt3_update_spheres_device(rt3_ctx* ctx, const void* d_center_radius, uint32_t n, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = update_spheres_checks(ctx, d_center_radius, n);
    if (rc) return rc;
    if ((uintptr_t)d_center_radius % 16u != 0) return fail(ctx, RT3_E_ARG, "device buffers must be 16-byte aligned");
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    ctx->n_sph = 0;                                                 // (no spheres until everything below has been issued)
    ctx->light_table = false;
    hipLaunchKernelGGL(k_refit_spheres, build_grid(n), dim3(kBlock), 0, stream, (const float4*)d_center_radius, n,
                       (const uint32_t*)ctx->d_sph_slot, ctx->sph_centre[0], ctx->sph_centre[1], ctx->sph_centre[2], ctx->d_sph.get(),
                       ctx->d_sph_cr.get(), ctx->d_sph_invr.get(), (u32x4*)ctx->d_sph_frag.get(), (u32x4*)ctx->d_sph_frag32.get(), ctx->sph.grp.get());
    RT3_HIP(hipGetLastError());
    if ((rc = refit_rows(ctx, ctx->sph, nullptr, ctx->sph_centre, stream)) || (rc = leave(ctx, stream))) return rc;
    ctx->n_sph = n;
    return 0;
}

int rt3_update_spheres(rt3_ctx* ctx, const float* center_radius, uint32_t n) {
    if (!ctx) return RT3_E_ARG;
    int rc = update_spheres_checks(ctx, center_radius, n);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++)                                // rt3_set_spheres' check; the scene is untouched
        if (!(center_radius[4 * (size_t)i + 3] > 0.0f)) return fail(ctx, RT3_E_ARG, "sphere " + std::to_string(i) + " has a non-positive radius");
    return staged(ctx, { stage_in(center_radius, (size_t)n * sizeof(float4)) },
                  [&](void* const* d) { return rt3_update_spheres_device(ctx, d[0], n, ctx->stream); });
}

// The launches of a mesh update, after the new vertices (and faces) have been queued into d_verts / d_gfaces on `stream`.
static int refit_mesh(rt3_ctx* ctx, hipStream_t stream) {
    const uint32_t n = ctx->n_faces, n_pad = (n + 3u) / 4u * 4u, n_verts = (uint32_t)ctx->d_verts.size(), n_frag_rows = (n + 31u) / 32u * 32u;
    const uint32_t n_pos = (uint32_t)ctx->tri.perm.size();
    for (const float scale : { 1.0f, 0.5f }) {                      // as rt3_mesh_commit: everything, then Mode R's fragments
        hipLaunchKernelGGL(k_commit_mesh, build_grid(n_frag_rows), dim3(kBlock), 0, stream, ctx->d_gfaces, ctx->d_verts, n, n_pad,
                           n_verts, ctx->d_face_mats_in, ctx->d_tri, ctx->d_tri_bound, ctx->d_tri_mat, ctx->d_tri_kind, ctx->d_error,
                           scale == 1.0f ? ctx->d_tri_frag.get() : ctx->d_tri_frag_r.get(), n_frag_rows, (const uint32_t*)ctx->d_box, scale);
        RT3_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_gather_members, build_grid(n_pos), dim3(kBlock), 0, stream, (const float4*)ctx->d_tri_bound,
                       (const uint32_t*)ctx->tri.perm, n_pos, ctx->tri.grp.get());
    hipLaunchKernelGGL(k_gather_face_records, build_grid(n_pos * 4u), dim3(kBlock), 0, stream, (const float4*)ctx->d_tri,
                       (const uint32_t*)ctx->tri.perm, n_pos, ctx->d_tri_rec.get());
    RT3_HIP(hipGetLastError());
    const float no_centre[3] = { 0.0f, 0.0f, 0.0f };
    return refit_rows(ctx, ctx->tri, ctx->d_box, no_centre, stream);
}
static int update_mesh_checks(rt3_ctx* ctx, const void* vertices, uint32_t n_vertices) {
    if (!vertices) return fail(ctx, RT3_E_ARG, "vertices is NULL");
    if (ctx->n_faces == 0) return fail(ctx, RT3_E_STATE, "no committed mesh to update: call rt3_set_mesh / rt3_mesh_commit first");
    if (!ctx->mesh_in_sync)
        return fail(ctx, RT3_E_STATE, "the merged entity buffers were changed after the last rt3_mesh_commit (rt3_mesh_begin / rt3_mesh_put without a commit)");
    if (n_vertices != ctx->d_verts.size()) return fail(ctx, RT3_E_ARG, "n_vertices must equal the vertex count of the merged entity buffers");
    return 0;
}
// host_err: the host form reads the error word itself, behind the update; the device form (NULL) leaves it to the next rt3_synchronize.
static int update_mesh_issue(rt3_ctx* ctx, const void* d_faces, const void* d_verts, void* stream_, uint32_t* host_err) {
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    const uint32_t n = ctx->n_faces;
    ctx->n_faces = 0;                                               // (no mesh until everything below has been issued)
    ctx->mesh_in_sync = false;
    ctx->light_table = false;
    if (host_err || !ctx->update_error_pending) RT3_HIP(hipMemsetAsync(ctx->d_error, 0, 4, stream));
    RT3_HIP(hipMemcpyAsync(ctx->d_verts, d_verts, ctx->d_verts.size() * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    if (d_faces) RT3_HIP(hipMemcpyAsync(ctx->d_gfaces, d_faces, (size_t)n * sizeof(rt3_gface), hipMemcpyDeviceToDevice, stream));
    ctx->n_faces = n;                                               // (refit_mesh reads the count; taken back below if it fails)
    rc = refit_mesh(ctx, stream);
    if (!rc) rc = leave(ctx, stream);
    if (rc) { ctx->n_faces = 0; return rc; }
    ctx->mesh_in_sync = true;
    if (host_err) RT3_HIP(hipMemcpyAsync(host_err, ctx->d_error, 4, hipMemcpyDeviceToHost, stream));
    return 0;
}

int rt3_update_mesh_device(rt3_ctx* ctx, const void* d_faces, const void* d_vertices, uint32_t n_vertices, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = update_mesh_checks(ctx, d_vertices, n_vertices);
    if (rc) return rc;
    if (((uintptr_t)d_faces | (uintptr_t)d_vertices) % 16u != 0) return fail(ctx, RT3_E_ARG, "device buffers must be 16-byte aligned");
    if ((rc = update_mesh_issue(ctx, d_faces, d_vertices, stream_, nullptr))) return rc;
    if (d_faces) ctx->update_error_pending = true;
    return 0;
}

int rt3_update_mesh(rt3_ctx* ctx, const rt3_gface* faces, const float* vertices, uint32_t n_vertices) {
    if (!ctx) return RT3_E_ARG;
    int rc = update_mesh_checks(ctx, vertices, n_vertices);
    if (rc) return rc;
    uint32_t err = 0;
    rc = staged(ctx, { stage_in(vertices, (size_t)n_vertices * sizeof(float4)), stage_in(faces, (size_t)ctx->n_faces * sizeof(rt3_gface)) },
                [&](void* const* d) { return update_mesh_issue(ctx, d[1], d[0], ctx->stream, &err); });
    if (rc) return rc;
    ctx->update_error_pending = false;
    if (err) {                                                      // as after rt3_set_mesh with such a face: no mesh
        ctx->n_faces = 0; ctx->mesh_in_sync = false;
        return fail(ctx, RT3_E_ARG, "a face references a vertex out of range");
    }
    return 0;
}

// ---- Regroup: the group order again from the records on the device, then the refit's tail
static int regroup_plan(rt3_ctx* ctx, RegroupPlan& P, uint32_t n_reg, uint32_t n_region, uint32_t n_prims) {
    int rc;
    if (!P.ready || P.n_reg != n_reg || P.n_region != n_region) {
        P = RegroupPlan();
        std::vector<uint32_t> parts{ 0u, n_reg }, table;
        for (;;) {
            uint32_t largest = 0;
            for (size_t k = 0; k + 1 < parts.size(); k++) largest = std::max(largest, parts[k + 1] - parts[k]);
            P.levels.push_back({ (uint32_t)table.size(), (uint32_t)parts.size() - 1u });
            table.insert(table.end(), parts.begin(), parts.end());
            if (largest <= kSplitCap) break;
            P.max_parts = std::max(P.max_parts, (uint32_t)parts.size() - 1u);
            std::vector<uint32_t> next;
            for (size_t k = 0; k + 1 < parts.size(); k++) {
                const uint32_t count = parts[k + 1] - parts[k];
                next.push_back(parts[k]);
                if (count > kLevFan) next.push_back(parts[k] + split_half(count, kLevFan, kSuper));
            }
            next.push_back(n_reg);
            parts.swap(next);
        }
        // what k_split_lds relies on: the parts of the last level tile [0, n_reg) and none exceeds its LDS
        const uint32_t* last = table.data() + P.levels.back().offset;
        for (uint32_t k = 0; k < P.levels.back().n_parts; k++)
            if (last[k + 1] <= last[k] || last[k + 1] - last[k] > kSplitCap) return fail(ctx, RT3_E_DEVICE, "rt3_regroup: the part table does not fit k_split_lds");
        if (last[0] != 0 || last[P.levels.back().n_parts] != n_reg) return fail(ctx, RT3_E_DEVICE, "rt3_regroup: the part table does not cover the region");
        if ((rc = P.table.upload(ctx, table))) return rc;
        size_t a = 0, b = 0;
        RT3_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, n_region, 0, 32, ctx->stream));
        RT3_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                   n_reg, 0, 64, ctx->stream));
        P.temp_bytes = std::max<size_t>(std::max(a, b), 16);
        RT3_HIP(hipFuncSetAttribute((const void*)k_split_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSplitLds));
        P.n_reg = n_reg; P.n_region = n_region; P.ready = true;
    }
    // (grow only: nothing happens here once both classes have been regrouped at their sizes)
    if ((rc = ctx->d_rg_cen.ensure(ctx, n_prims)) || (rc = ctx->d_rg_ids[0].ensure(ctx, n_region)) || (rc = ctx->d_rg_ids[1].ensure(ctx, n_region)) ||
        (rc = ctx->d_rg_keys[0].ensure(ctx, n_reg)) || (rc = ctx->d_rg_keys[1].ensure(ctx, n_reg)) ||
        (rc = ctx->d_rg_box.ensure(ctx, (size_t)std::max(P.max_parts, 1u) * 6)) || (rc = ctx->d_rg_temp.ensure(ctx, P.temp_bytes)))
        return rc;
    return 0;
}
// The split of one class: R.perm[0 .. n_reg) becomes the specified order of the primitives it holds; pads and whatever follows stay.
static int regroup_order(rt3_ctx* ctx, const RegroupPlan& P, FilterRows& R, hipStream_t stream) {
    const dim3 blk(kBlock);
    size_t temp = P.temp_bytes;
    // the region's primitive ids in ascending order (pads are 0xFFFFFFFF: they sort behind the n_reg ids)
    RT3_HIP(hipcub::DeviceRadixSort::SortKeys(ctx->d_rg_temp.get(), temp, (const uint32_t*)R.perm.get(), ctx->d_rg_ids[0].get(), P.n_region, 0, 32, stream));
    int cur = 0;
    for (size_t l = 0; l + 1 < P.levels.size(); l++) {
        const uint32_t* begins = P.table.get() + P.levels[l].offset;
        const uint32_t n_parts = P.levels[l].n_parts;
        hipLaunchKernelGGL(k_part_box_clear, build_grid(n_parts * 6), blk, 0, stream, n_parts, ctx->d_rg_box.get());
        hipLaunchKernelGGL(k_part_box, build_grid((P.n_reg + kBoxPerThread - 1) / kBoxPerThread), blk, 0, stream, begins, n_parts, (const uint32_t*)ctx->d_rg_ids[cur].get(),
                           (const float4*)ctx->d_rg_cen.get(), P.n_reg, ctx->d_rg_box.get());
        hipLaunchKernelGGL(k_part_keys, build_grid(P.n_reg), blk, 0, stream, begins, n_parts, (const uint32_t*)ctx->d_rg_ids[cur].get(),
                           (const float4*)ctx->d_rg_cen.get(), P.n_reg, (const uint32_t*)ctx->d_rg_box.get(), kLevFan, ctx->d_rg_keys[0].get());
        RT3_HIP(hipGetLastError());
        int part_bits = 0;                                          // only the bits in use are sorted
        while ((1u << part_bits) < n_parts) part_bits++;
        temp = P.temp_bytes;
        RT3_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->d_rg_temp.get(), temp, (const uint64_t*)ctx->d_rg_keys[0].get(), ctx->d_rg_keys[1].get(),
                                                   (const uint32_t*)ctx->d_rg_ids[cur].get(), ctx->d_rg_ids[cur ^ 1].get(), P.n_reg, 0, 32 + part_bits, stream));
        cur ^= 1;
    }
    const RegroupPlan::Level& last = P.levels.back();
    hipLaunchKernelGGL(k_split_lds, dim3(last.n_parts), dim3(kSplitThreads), kSplitLds, stream, (const uint32_t*)(P.table.get() + last.offset),
                       (const uint32_t*)ctx->d_rg_ids[cur].get(), (const float4*)ctx->d_rg_cen.get(), kLevFan, kSuper, R.perm.get());
    RT3_HIP(hipGetLastError());
    return 0;
}
static int regroup_spheres(rt3_ctx* ctx, hipStream_t stream) {
    const uint32_t n = ctx->n_sph, n_pos = (uint32_t)ctx->sph.perm.size(), n_reg = n - ctx->n_direct;
    if (n_pos == 0 || n_reg == 0) return 0;                         // every sphere is on the direct list: no rows
    int rc;
    if ((rc = regroup_plan(ctx, ctx->rg_sph, n_reg, n_pos, n))) return rc;
    const dim3 blk(kBlock);
    ctx->n_sph = 0;                                                 // (no spheres until everything below has been issued)
    hipLaunchKernelGGL(k_regroup_centres_sph, build_grid(n), blk, 0, stream, (const float4*)ctx->d_sph_cr.get(), n, ctx->sph_centre[0], ctx->sph_centre[1],
                       ctx->sph_centre[2], ctx->d_rg_cen.get());
    RT3_HIP(hipGetLastError());
    if ((rc = regroup_order(ctx, ctx->rg_sph, ctx->sph, stream))) return rc;
    hipLaunchKernelGGL(k_inverse_slots, build_grid(n_pos), blk, 0, stream, (const uint32_t*)ctx->sph.perm.get(), n_pos, ctx->d_sph_slot.get());
    hipLaunchKernelGGL(k_gather_members, build_grid(n_pos), blk, 0, stream, (const float4*)ctx->d_sph.get(), (const uint32_t*)ctx->sph.perm.get(), n_pos,
                       ctx->sph.grp.get());
    RT3_HIP(hipGetLastError());
    return refit_rows(ctx, ctx->sph, nullptr, ctx->sph_centre, stream);
}
static int regroup_mesh(rt3_ctx* ctx, hipStream_t stream) {
    const uint32_t n = ctx->n_faces, n_pos = (uint32_t)ctx->tri.perm.size(), n_reg = ctx->tri_bounded;
    if (n_pos == 0 || n_reg == 0) return 0;                         // no face with a bounded hit region: nothing to order
    int rc;
    if ((rc = regroup_plan(ctx, ctx->rg_tri, n_reg, round_up(n_reg, kGroupTri * kSuper), n))) return rc;
    const dim3 blk(kBlock);
    ctx->n_faces = 0;                                               // (no mesh until everything below has been issued)
    hipLaunchKernelGGL(k_regroup_centres_tri, build_grid(n), blk, 0, stream, (const float4*)ctx->d_tri_bound.get(), n, (const uint32_t*)ctx->d_box.get(),
                       ctx->d_rg_cen.get());
    RT3_HIP(hipGetLastError());
    if ((rc = regroup_order(ctx, ctx->rg_tri, ctx->tri, stream))) return rc;
    hipLaunchKernelGGL(k_gather_members, build_grid(n_pos), blk, 0, stream, (const float4*)ctx->d_tri_bound.get(), (const uint32_t*)ctx->tri.perm.get(), n_pos,
                       ctx->tri.grp.get());
    hipLaunchKernelGGL(k_gather_face_records, build_grid(n_pos * 4u), blk, 0, stream, (const float4*)ctx->d_tri.get(), (const uint32_t*)ctx->tri.perm.get(),
                       n_pos, ctx->d_tri_rec.get());
    RT3_HIP(hipGetLastError());
    const float no_centre[3] = { 0.0f, 0.0f, 0.0f };
    return refit_rows(ctx, ctx->tri, ctx->d_box, no_centre, stream);
}
static int regroup_checks(rt3_ctx* ctx, uint32_t what) {
    if (what == 0 || (what & ~(RT3_REGROUP_SPHERES | RT3_REGROUP_MESH))) return fail(ctx, RT3_E_ARG, "what must name RT3_REGROUP_SPHERES and / or RT3_REGROUP_MESH");
    if (what & RT3_REGROUP_SPHERES) {
        if (ctx->n_sph == 0) return fail(ctx, RT3_E_STATE, "no spheres to regroup: call rt3_set_spheres first");
        if (ctx->sph_left_out)
            return fail(ctx, RT3_E_STATE, "the last rt3_set_spheres left a non-finite sphere out of the group order: it has no position a regroup could give it");
    }
    if (what & RT3_REGROUP_MESH) {
        if (ctx->n_faces == 0) return fail(ctx, RT3_E_STATE, "no committed mesh to regroup: call rt3_set_mesh / rt3_mesh_commit first");
        if (!ctx->mesh_in_sync)
            return fail(ctx, RT3_E_STATE, "the merged entity buffers were changed after the last rt3_mesh_commit (rt3_mesh_begin / rt3_mesh_put without a commit)");
    }
    return 0;
}

int rt3_regroup_device(rt3_ctx* ctx, uint32_t what, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = regroup_checks(ctx, what);
    if (rc) return rc;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    // a class's count is cleared before its first launch (regroup_spheres / regroup_mesh) and published only once the event behind the last
    // launch has been recorded: a failure anywhere leaves no scene of the classes that were touched, never new counts over old buffers
    const uint32_t n_sph = ctx->n_sph, n_faces = ctx->n_faces;
    if ((what & RT3_REGROUP_SPHERES) && (rc = regroup_spheres(ctx, stream))) return rc;
    if ((what & RT3_REGROUP_MESH) && (rc = regroup_mesh(ctx, stream))) return rc;
    if ((rc = leave(ctx, stream))) return rc;
    ctx->n_sph = n_sph; ctx->n_faces = n_faces;
    return 0;
}

int rt3_regroup(rt3_ctx* ctx, uint32_t what) {
    if (!ctx) return RT3_E_ARG;
    const int rc = rt3_regroup_device(ctx, what, ctx->stream);
    if (rc) return rc;
    RT3_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int rt3_debug_group_order(rt3_ctx* ctx, uint32_t what, uint32_t* out, uint64_t capacity_words, uint32_t* n_positions) {
    if (!ctx) return RT3_E_ARG;
    if (what != RT3_REGROUP_SPHERES && what != RT3_REGROUP_MESH) return fail(ctx, RT3_E_ARG, "what must be exactly one of RT3_REGROUP_SPHERES, RT3_REGROUP_MESH");
    if (!n_positions) return fail(ctx, RT3_E_ARG, "n_positions is NULL");
    const bool sph = what == RT3_REGROUP_SPHERES;
    if ((sph ? ctx->n_sph : ctx->n_faces) == 0) return fail(ctx, RT3_E_STATE, "no committed scene of that class");
    const FilterRows& R = sph ? ctx->sph : ctx->tri;
    *n_positions = (uint32_t)R.perm.size();
    if (capacity_words < R.perm.size() || (!out && R.perm.size())) return fail(ctx, RT3_E_ARG, "capacity_words is too small for the group order");
    RT3_HIP(hipSetDevice(ctx->device));
    if (ctx->ev_acc_recorded) RT3_HIP(hipEventSynchronize(ctx->ev_acc));    // (a regroup may have run on a caller's stream)
    if (R.perm.size()) RT3_HIP(hipMemcpy(out, R.perm.get(), R.perm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

// ---- Full upload from device arrays: phase 1 looks at the caller's arrays and writes scratch only, one read-back of the
// build's header follows, phase 2 allocates and queues the rest — the refit's kernels, regroup_order and the refit's tail
// the header and the block counts of a build over n primitives; with sort_scratch the key buffers and the radix sorts' temporary storage of the
// medians (the regroup's scratch: it belongs to the context, and a build's later regroup_plan only grows it)
static int build_scratch(rt3_ctx* ctx, uint32_t n, bool sort_scratch, size_t* temp_bytes) {
    int rc;
    if ((rc = ctx->d_sb.ensure(ctx, (size_t)kSbWords + build_grid(n).x))) return rc;
    if (!sort_scratch) return 0;
    size_t a = 0, b = 0;
    RT3_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32, ctx->stream));
    RT3_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 64, ctx->stream));
    *temp_bytes = std::max<size_t>(std::max(a, b), 16);
    if ((rc = ctx->d_rg_ids[0].ensure(ctx, n)) || (rc = ctx->d_rg_ids[1].ensure(ctx, n)) || (rc = ctx->d_rg_keys[0].ensure(ctx, n)) ||
        (rc = ctx->d_rg_keys[1].ensure(ctx, n)) || (rc = ctx->d_rg_temp.ensure(ctx, *temp_bytes)))
        return rc;
    return 0;
}
int rt3_set_spheres_device(rt3_ctx* ctx, const void* d_center_radius, const void* d_materials, uint32_t n, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    if (n != 0 && (!d_center_radius || !d_materials)) return fail(ctx, RT3_E_ARG, "center_radius / materials is NULL");
    if ((uintptr_t)d_center_radius % 16u != 0 || (uintptr_t)d_materials % 4u != 0)
        return fail(ctx, RT3_E_ARG, "device buffers must be 16-byte aligned (materials: 4-byte)");
    if (n > 0x7FFFFFFFu) return fail(ctx, RT3_E_ARG, "too many primitives");
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    if (n == 0) { clear_spheres(ctx); return 0; }
    const float4* const in = (const float4*)d_center_radius;
    const rt3_material* const mats = (const rt3_material*)d_materials;
    const dim3 blk(kBlock), one(1);
    // ---- phase 1: nothing of the scene is touched
    size_t temp_bytes = 0;
    if ((rc = build_scratch(ctx, n, true, &temp_bytes))) return rc;
    uint32_t* const hdr = ctx->d_sb.get();
    uint32_t* const block_counts = hdr + kSbWords;
    hipLaunchKernelGGL(k_sb_init, one, dim3(64), 0, stream, hdr);
    hipLaunchKernelGGL(k_sb_check_radii, build_grid(n), blk, 0, stream, in, n, hdr);
    hipLaunchKernelGGL(k_sb_check_kinds, build_grid(n), blk, 0, stream, mats, n, hdr);
    RT3_HIP(hipGetLastError());
    for (uint32_t axis = 0; axis < 3; axis++) {                     // the filter centre: three medians
        hipLaunchKernelGGL(k_sb_axis_keys, build_grid(n), blk, 0, stream, in, n, axis, ctx->d_rg_ids[0].get(), hdr);
        size_t temp = temp_bytes;
        RT3_HIP(hipcub::DeviceRadixSort::SortKeys(ctx->d_rg_temp.get(), temp, (const uint32_t*)ctx->d_rg_ids[0].get(), ctx->d_rg_ids[1].get(), n, 0, 32, stream));
        hipLaunchKernelGGL(k_sb_pick_centre, one, one, 0, stream, (const uint32_t*)ctx->d_rg_ids[1].get(), axis, hdr);
        RT3_HIP(hipGetLastError());
    }
    {                                                               // the scene size, the candidates, the four strongest
        hipLaunchKernelGGL(k_sb_dist_keys, build_grid(n), blk, 0, stream, in, n, (const uint32_t*)hdr, ctx->d_rg_keys[0].get());
        size_t temp = temp_bytes;
        RT3_HIP(hipcub::DeviceRadixSort::SortKeys(ctx->d_rg_temp.get(), temp, (const uint64_t*)ctx->d_rg_keys[0].get(), ctx->d_rg_keys[1].get(), n, 0, 64, stream));
        hipLaunchKernelGGL(k_sb_pick_scene, one, one, 0, stream, (const uint64_t*)ctx->d_rg_keys[1].get(), n, hdr);
        hipLaunchKernelGGL(k_sb_ratio_keys, build_grid(n), blk, 0, stream, in, n, hdr, ctx->d_rg_keys[0].get());
        for (uint32_t k = 0; k < 4; k++) hipLaunchKernelGGL(k_sb_top, build_grid(n), blk, 0, stream, (const uint64_t*)ctx->d_rg_keys[0].get(), n, k, hdr);
        RT3_HIP(hipGetLastError());
    }
    const SphInOrder in_order{ in, hdr };
    hipLaunchKernelGGL(k_compact_count<SphInOrder>, build_grid(n), blk, 0, stream, in_order, n, block_counts, hdr + kSbInOrder);
    RT3_HIP(hipGetLastError());
    uint32_t h[kSbFaceError];                                       // the call's one wait for the device
    RT3_HIP(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    RT3_HIP(hipStreamSynchronize(stream));
    if (h[kSbBadRadius] != 0xFFFFFFFFu) return fail(ctx, RT3_E_ARG, "sphere " + std::to_string(h[kSbBadRadius]) + " has a non-positive radius");
    if (h[kSbBadKind]) return fail(ctx, RT3_E_ARG, "unknown material kind");
    // ---- phase 2
    ctx->n_sph = 0;                                                 // (no spheres until everything below has been issued)
    ctx->light_table = false;
    drop_sphere_binding(ctx);
    std::memcpy(ctx->sph_centre, h + kSbCentre, sizeof ctx->sph_centre);
    ctx->n_direct = std::min(h[kSbCand], 4u);
    for (uint32_t k = 0; k < ctx->n_direct; k++) ctx->direct[k] = 0xFFFFFFFFu - h[kSbBest + 2 * k];     // (the key's low word)
    std::sort(ctx->direct, ctx->direct + ctx->n_direct);
    const uint32_t n_in = h[kSbInOrder], n_pos = round_up(n_in, kGroupSph * kSuper), blocks = (n + 31u) / 32u;
    ctx->sph_left_out = n_in + ctx->n_direct != n;
    if ((rc = ctx->d_sph_frag.alloc(ctx, (size_t)blocks * 4 * 64 * 4)) || (rc = ctx->d_sph_frag32.alloc(ctx, (size_t)blocks * 2 * 64 * 4)) ||
        (rc = ctx->d_sph.alloc(ctx, ((size_t)n + 3) / 4 * 4)) || (rc = ctx->d_sph_invr.alloc(ctx, n)) || (rc = ctx->d_sph_mat.alloc(ctx, n)) ||
        (rc = ctx->d_sph_kind.alloc(ctx, n)) || (rc = ctx->d_sph_cr.alloc(ctx, n)) || (rc = ctx->d_sph_slot.alloc(ctx, n)) ||
        (rc = alloc_rows(ctx, ctx->sph, n_pos, kGroupSph)))
        return rc;
    SphDirect direct{ ctx->n_direct, { 0u, 0u, 0u, 0u } };
    for (uint32_t k = 0; k < ctx->n_direct; k++) direct.id[k] = ctx->direct[k];
    hipLaunchKernelGGL(k_build_spheres, build_grid(blocks * 32u), blk, 0, stream, in, mats, n, blocks * 32u, ctx->sph_centre[0], ctx->sph_centre[1],
                       ctx->sph_centre[2], direct, ctx->d_sph.get(), ctx->d_sph_cr.get(), ctx->d_sph_invr.get(), ctx->d_sph_mat.get(), ctx->d_sph_kind.get(),
                       (u32x4*)ctx->d_sph_frag.get(), (u32x4*)ctx->d_sph_frag32.get());
    hipLaunchKernelGGL(k_fill_words, build_grid(n), blk, 0, stream, ctx->d_sph_slot.get(), n, 0xFFFFFFFFu);
    RT3_HIP(hipGetLastError());
    if (n_pos) {
        // the initial order: the usable ids in ascending order, pads behind them; then the regroup's split and the refit's tail
        hipLaunchKernelGGL(k_fill_words, build_grid(n_pos), blk, 0, stream, ctx->sph.perm.get(), n_pos, 0xFFFFFFFFu);
        hipLaunchKernelGGL(k_compact_select<SphInOrder>, build_grid(n), blk, 0, stream, in_order, n, (const uint32_t*)block_counts, ctx->sph.perm.get(),
                           (uint32_t*)nullptr);
        RT3_HIP(hipGetLastError());
        if ((rc = regroup_plan(ctx, ctx->rg_sph, n_in, n_pos, n))) return rc;
        hipLaunchKernelGGL(k_regroup_centres_sph, build_grid(n), blk, 0, stream, in, n, ctx->sph_centre[0], ctx->sph_centre[1], ctx->sph_centre[2],
                           ctx->d_rg_cen.get());
        RT3_HIP(hipGetLastError());
        if ((rc = regroup_order(ctx, ctx->rg_sph, ctx->sph, stream))) return rc;
        hipLaunchKernelGGL(k_inverse_slots, build_grid(n_pos), blk, 0, stream, (const uint32_t*)ctx->sph.perm.get(), n_pos, ctx->d_sph_slot.get());
        hipLaunchKernelGGL(k_gather_members, build_grid(n_pos), blk, 0, stream, (const float4*)ctx->d_sph.get(), (const uint32_t*)ctx->sph.perm.get(), n_pos,
                           ctx->sph.grp.get());
        RT3_HIP(hipGetLastError());
        if ((rc = refit_rows(ctx, ctx->sph, nullptr, ctx->sph_centre, stream))) return rc;
    }
    if ((rc = leave(ctx, stream))) return rc;
    ctx->n_sph = n;
    return 0;
}

int rt3_set_mesh_device(rt3_ctx* ctx, const void* d_faces, uint32_t n_faces, const void* d_vertices, uint32_t n_vertices, const void* d_face_materials,
                        void* stream_) {
    if (!ctx) return RT3_E_ARG;
    if (n_faces != 0 && (!d_faces || !d_vertices)) return fail(ctx, RT3_E_ARG, "faces / vertices is NULL");
    if (n_vertices != 0 && !d_vertices) return fail(ctx, RT3_E_ARG, "faces / vertices is NULL");
    if (((uintptr_t)d_faces | (uintptr_t)d_vertices) % 16u != 0 || (uintptr_t)d_face_materials % 4u != 0)
        return fail(ctx, RT3_E_ARG, "device buffers must be 16-byte aligned (materials: 4-byte)");
    if (n_faces > 0x7FFFFFFFu) return fail(ctx, RT3_E_ARG, "too many primitives");
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    if (n_faces == 0) { clear_mesh(ctx); ctx->d_gfaces.reset(); ctx->d_verts.reset(); return 0; }
    const uint32_t n = n_faces, n_pad = (n + 3u) / 4u * 4u, n_frag_rows = (n + 31u) / 32u * 32u;
    const dim3 blk(kBlock);
    // ---- phase 1: the new mesh is built in buffers the context does not hold yet — its own copy of the caller's arrays, the render layout, the
    // vertex box — so that a refusal leaves the scene as it was
    DevBuf<rt3_gface> gfaces; DevBuf<float4> verts, tri, tri_mat, tri_bound; DevBuf<rt3_material> mats_in; DevBuf<uint32_t> tri_kind, box;
    DevBuf<u32x4> tri_frag, tri_frag_r;
    if ((rc = build_scratch(ctx, n, false, nullptr)) || (rc = gfaces.alloc(ctx, n)) || (rc = verts.alloc(ctx, n_vertices)) ||
        (rc = mats_in.alloc(ctx, d_face_materials ? n : 0)) || (rc = tri.alloc(ctx, (size_t)n * 4)) || (rc = tri_mat.alloc(ctx, n)) ||
        (rc = tri_kind.alloc(ctx, n)) || (rc = tri_bound.alloc(ctx, n_pad)) || (rc = tri_frag.alloc(ctx, (size_t)n_frag_rows * 8)) ||
        (rc = tri_frag_r.alloc(ctx, (size_t)n_frag_rows * 8)) || (rc = box.alloc(ctx, 6)))
        return rc;
    uint32_t* const hdr = ctx->d_sb.get();
    uint32_t* const block_counts = hdr + kSbWords;
    hipLaunchKernelGGL(k_sb_init, dim3(1), dim3(64), 0, stream, hdr);
    RT3_HIP(hipMemcpyAsync(gfaces, d_faces, (size_t)n * sizeof(rt3_gface), hipMemcpyDeviceToDevice, stream));
    RT3_HIP(hipMemcpyAsync(verts, d_vertices, (size_t)n_vertices * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    if (d_face_materials) {
        RT3_HIP(hipMemcpyAsync(mats_in, d_face_materials, (size_t)n * sizeof(rt3_material), hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(k_sb_check_kinds, build_grid(n), blk, 0, stream, (const rt3_material*)mats_in.get(), n, hdr);
    }
    if ((rc = render_layout(ctx, gfaces, verts, n, n_vertices, mats_in, tri, tri_bound, tri_mat, tri_kind, tri_frag, tri_frag_r, box, hdr + kSbFaceError, stream)))
        return rc;
    const FaceInOrder in_order{ tri_bound.get() };
    hipLaunchKernelGGL(k_compact_count<FaceInOrder>, build_grid(n), blk, 0, stream, in_order, n, block_counts, hdr + kSbInOrder);
    RT3_HIP(hipGetLastError());
    uint32_t h[kSbWords], hbox[6];                                  // the call's one wait for the device
    RT3_HIP(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    RT3_HIP(hipMemcpyAsync(hbox, box, sizeof hbox, hipMemcpyDeviceToHost, stream));
    RT3_HIP(hipStreamSynchronize(stream));
    if (h[kSbBadKind]) return fail(ctx, RT3_E_ARG, "unknown material kind");
    // ---- phase 2: the context takes the new buffers
    clear_mesh(ctx);
    ctx->d_gfaces = std::move(gfaces); ctx->d_verts = std::move(verts); ctx->d_face_mats_in = std::move(mats_in);
    if (h[kSbFaceError]) return fail(ctx, RT3_E_ARG, "a face references a vertex out of range");   // (no mesh, as after rt3_set_mesh)
    ctx->d_tri = std::move(tri); ctx->d_tri_mat = std::move(tri_mat); ctx->d_tri_bound = std::move(tri_bound); ctx->d_tri_kind = std::move(tri_kind);
    ctx->d_tri_frag = std::move(tri_frag); ctx->d_tri_frag_r = std::move(tri_frag_r); ctx->d_box = std::move(box);
    box_centre(hbox, ctx->tri_centre);
    if ((rc = ctx->d_error.ensure(ctx, 1))) return rc;
    RT3_HIP(hipMemsetAsync(ctx->d_error, 0, 4, stream));
    // face_group_order's layout: the bounded faces and their pads, then the others in ascending index order and theirs
    const uint32_t n_in = h[kSbInOrder], row = kGroupTri * kSuper, pos_in = round_up(n_in, row), n_pos = pos_in + round_up(n - n_in, row);
    if ((rc = alloc_rows(ctx, ctx->tri, n_pos, kGroupTri)) || (rc = ctx->d_tri_rec.alloc(ctx, (size_t)n_pos * 4))) return rc;
    const FaceInOrder committed{ ctx->d_tri_bound.get() };
    hipLaunchKernelGGL(k_fill_words, build_grid(n_pos), blk, 0, stream, ctx->tri.perm.get(), n_pos, 0xFFFFFFFFu);
    hipLaunchKernelGGL(k_compact_select<FaceInOrder>, build_grid(n), blk, 0, stream, committed, n, (const uint32_t*)block_counts, ctx->tri.perm.get(),
                       ctx->tri.perm.get() + pos_in);
    RT3_HIP(hipGetLastError());
    if (n_in) {
        if ((rc = regroup_plan(ctx, ctx->rg_tri, n_in, pos_in, n))) return rc;
        hipLaunchKernelGGL(k_regroup_centres_tri, build_grid(n), blk, 0, stream, (const float4*)ctx->d_tri_bound.get(), n, (const uint32_t*)ctx->d_box.get(),
                           ctx->d_rg_cen.get());
        RT3_HIP(hipGetLastError());
        if ((rc = regroup_order(ctx, ctx->rg_tri, ctx->tri, stream))) return rc;
    }
    hipLaunchKernelGGL(k_gather_members, build_grid(n_pos), blk, 0, stream, (const float4*)ctx->d_tri_bound.get(), (const uint32_t*)ctx->tri.perm.get(), n_pos,
                       ctx->tri.grp.get());
    hipLaunchKernelGGL(k_gather_face_records, build_grid(n_pos * 4u), blk, 0, stream, (const float4*)ctx->d_tri.get(), (const uint32_t*)ctx->tri.perm.get(),
                       n_pos, ctx->d_tri_rec.get());
    RT3_HIP(hipGetLastError());
    const float no_centre[3] = { 0.0f, 0.0f, 0.0f };
    if ((rc = refit_rows(ctx, ctx->tri, ctx->d_box, no_centre, stream)) || (rc = leave(ctx, stream))) return rc;
    ctx->tri_bounded = n_in;
    ctx->n_faces = n;
    ctx->mesh_in_sync = true;
    return 0;
}

int rt3_debug_sphere_build(rt3_ctx* ctx, float centre[3], uint32_t direct[4], uint32_t* n_direct) {
    if (!ctx) return RT3_E_ARG;
    if (!centre || !direct || !n_direct) return fail(ctx, RT3_E_ARG, "centre / direct / n_direct is NULL");
    if (ctx->n_sph == 0) return fail(ctx, RT3_E_STATE, "no spheres: call rt3_set_spheres first");
    for (int a = 0; a < 3; a++) centre[a] = ctx->sph_centre[a];
    for (int k = 0; k < 4; k++) direct[k] = (uint32_t)k < ctx->n_direct ? ctx->direct[k] : 0xFFFFFFFFu;
    *n_direct = ctx->n_direct;
    return 0;
}
// ---- Environment map: the context's own copy of a cube map, read by the miss of the environment forms (5.2n) and by k_aov_accumulate.
// Replacing it allocates the new copy first and frees the old one behind the event chain, so that a failure leaves the previous map in place.
static int environment_checks(rt3_ctx* ctx, const void* rgba, uint32_t n_face) {
    if (!rgba) return fail(ctx, RT3_E_ARG, "environment array is NULL");
    if (n_face > RT3_ENV_MAX_FACE) return fail(ctx, RT3_E_ARG, "n_face must be <= " + std::to_string(RT3_ENV_MAX_FACE));
    return 0;
}
int rt3_clear_environment(rt3_ctx* ctx) {
    if (!ctx) return RT3_E_ARG;
    if (ctx->env_n == 0) return 0;
    RT3_HIP(hipSetDevice(ctx->device));
    if (ctx->ev_acc_recorded) RT3_HIP(hipEventSynchronize(ctx->ev_acc));       // a launch still in flight may read the map
    ctx->d_env.reset();
    ctx->env_n = 0;
    ctx->env_table = false;                                         // (the table's buffers stay for the next map)
    return 0;
}
uint32_t rt3_environment_size(rt3_ctx* ctx) { return ctx ? ctx->env_n : 0u; }
// The copy of both forms: `src` is a device array (kind device-to-device) or, for the host form, the caller's host array, queued on `stream_`.
static int install_environment(rt3_ctx* ctx, const void* src, hipMemcpyKind kind, uint32_t n_face, void* stream_) {
    const size_t texels = (size_t)6 * n_face * n_face;
    hipStream_t stream;
    int rc;
    if (ctx->env_n == n_face) {                                     // the same size: into the copy the context has, behind whatever still reads it
        if ((rc = enter(ctx, stream_, &stream))) return rc;
        ctx->env_table = false;                                     // the next call with RT3_FLAG_ENV_SAMPLING builds the new map's table
        RT3_HIP(hipMemcpyAsync(ctx->d_env.get(), src, texels * sizeof(float4), kind, stream));
        return leave(ctx, stream);
    }
    DevBuf<float4> fresh;
    if ((rc = fresh.alloc(ctx, texels)) || (rc = enter(ctx, stream_, &stream))) return rc;
    RT3_HIP(hipMemcpyAsync(fresh.get(), src, texels * sizeof(float4), kind, stream));
    if ((rc = leave(ctx, stream))) return rc;
    if (ctx->env_n != 0 && ctx->ev_acc_recorded) RT3_HIP(hipEventSynchronize(ctx->ev_acc));    // the old copy is freed: nothing may still read it
    ctx->d_env = std::move(fresh);
    ctx->env_n = n_face;
    ctx->env_table = false;
    return 0;
}
int rt3_set_environment_device(rt3_ctx* ctx, const void* d_rgba, uint32_t n_face, void* stream) {
    if (!ctx) return RT3_E_ARG;
    if (n_face == 0) return rt3_clear_environment(ctx);
    int rc = environment_checks(ctx, d_rgba, n_face);
    if (rc) return rc;
    if ((uintptr_t)d_rgba % 16u != 0) return fail(ctx, RT3_E_ARG, "d_rgba must be 16-byte aligned");
    return install_environment(ctx, d_rgba, hipMemcpyDeviceToDevice, n_face, stream);
}
int rt3_set_environment(rt3_ctx* ctx, const float* rgba, uint32_t n_face) {
    if (!ctx) return RT3_E_ARG;
    if (n_face == 0) return rt3_clear_environment(ctx);
    int rc = environment_checks(ctx, rgba, n_face);
    if (rc) return rc;
    const size_t texels = (size_t)6 * n_face * n_face;
    for (size_t i = 0; i < texels; i++)
        if (!std::isfinite(rgba[4 * i]) || !std::isfinite(rgba[4 * i + 1]) || !std::isfinite(rgba[4 * i + 2]))
            return fail(ctx, RT3_E_ARG, "environment texel " + std::to_string(i) + " is not finite");
    if ((rc = install_environment(ctx, rgba, hipMemcpyHostToDevice, n_face, ctx->stream))) return rc;      // (no staging buffer: a large map would stay in it)
    RT3_HIP(hipStreamSynchronize(ctx->stream));                     // the caller's array is free again
    return 0;
}

// ---- Image textures: the slots' copies, their descriptors on the device, the two bindings.  Read by shade_lane of the texture forms
// (5.2u) and by k_aov_accumulate, both through tex_modulate.
namespace {
// One slot's descriptor, written on the stream (the value travels in the launch: no host memory has to outlive the call).
__global__ void k_tex_set_slot(uint4* __restrict__ slots, uint32_t slot, uint4 d) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && slot < RT3_TEX_MAX_TEXTURES) slots[slot] = d;
}
// A binding's check: out[0] = the lowest index whose entry is neither RT3_TEX_NONE nor a slot (0xFFFFFFFF: none), out[1 + s / 32] bit s % 32: slot s is named.
__global__ __launch_bounds__(kBlock) void k_tex_check_binding(const uint32_t* __restrict__ slots, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slots[i];
    if (s == RT3_TEX_NONE) return;
    if (s >= RT3_TEX_MAX_TEXTURES) atomicMin(out, i);
    else atomicOr(out + 1u + s / 32u, 1u << (s % 32u));
}
uint4 tex_descriptor(const float4* texels, uint32_t w, uint32_t h, uint32_t wrap) {
    const uint64_t a = (uint64_t)(uintptr_t)texels;
    return make_uint4((uint32_t)a, (uint32_t)(a >> 32), w | (h << 16), wrap);
}
// The descriptor table, allocated (all slots empty) by the first call that needs it.
int ensure_tex_slots(rt3_ctx* ctx) {
    if (ctx->d_tex_slots.size() != 0) return 0;
    const int rc = ctx->d_tex_slots.alloc(ctx, RT3_TEX_MAX_TEXTURES);
    if (rc) return rc;
    RT3_HIP(hipMemset(ctx->d_tex_slots.get(), 0, RT3_TEX_MAX_TEXTURES * sizeof(uint4)));
    return 0;
}
int texture_checks(rt3_ctx* ctx, uint32_t slot, const void* rgba, uint32_t w, uint32_t h, uint32_t wrap) {
    if (slot >= RT3_TEX_MAX_TEXTURES) return fail(ctx, RT3_E_ARG, "slot must be < " + std::to_string(RT3_TEX_MAX_TEXTURES));
    if (w == 0 || h == 0) return 0;                                 // frees the slot: nothing else is read
    if (w > RT3_TEX_MAX_SIDE || h > RT3_TEX_MAX_SIDE) return fail(ctx, RT3_E_ARG, "texture sides must be <= " + std::to_string(RT3_TEX_MAX_SIDE));
    if ((uint64_t)w * h > (1ull << 26)) return fail(ctx, RT3_E_ARG, "a texture holds at most 2^26 texels");
    if (wrap != RT3_TEX_REPEAT && wrap != RT3_TEX_CLAMP) return fail(ctx, RT3_E_ARG, "wrap must be RT3_TEX_REPEAT or RT3_TEX_CLAMP");
    if (!rgba) return fail(ctx, RT3_E_ARG, "texture array is NULL");
    return 0;
}
// Empties the slot: the descriptor first, behind the event chain; then, once nothing in flight can read it, the copy.
int free_texture(rt3_ctx* ctx, uint32_t slot, void* stream_) {
    rt3_ctx::TexSlot& S = ctx->tex[slot];
    if (S.w == 0) return 0;
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    hipLaunchKernelGGL(k_tex_set_slot, dim3(1), dim3(1), 0, stream, ctx->d_tex_slots.get(), slot, make_uint4(0u, 0u, 0u, 0u));
    RT3_HIP(hipGetLastError());
    if ((rc = leave(ctx, stream))) return rc;
    RT3_HIP(hipEventSynchronize(ctx->ev_acc));
    S.texels.reset();
    S.w = S.h = S.wrap = 0;
    return 0;
}
// The copy of both forms (install_environment's pattern): into the copy the slot has when the size is the same, else into a fresh one — allocated first,
// so that a failure leaves the slot as it was — and the old copy is freed once nothing can still read it.
int install_texture(rt3_ctx* ctx, uint32_t slot, const void* src, hipMemcpyKind kind, uint32_t w, uint32_t h, uint32_t wrap, void* stream_) {
    rt3_ctx::TexSlot& S = ctx->tex[slot];
    const size_t texels = (size_t)w * h;
    hipStream_t stream;
    int rc;
    if ((rc = ensure_tex_slots(ctx))) return rc;
    const bool same = S.w != 0 && (size_t)S.w * S.h == texels;
    DevBuf<float4> fresh;
    if (!same && (rc = fresh.alloc(ctx, texels))) return rc;
    float4* const dst = same ? S.texels.get() : fresh.get();
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    RT3_HIP(hipMemcpyAsync(dst, src, texels * sizeof(float4), kind, stream));
    hipLaunchKernelGGL(k_tex_set_slot, dim3(1), dim3(1), 0, stream, ctx->d_tex_slots.get(), slot, tex_descriptor(dst, w, h, wrap));
    RT3_HIP(hipGetLastError());
    if ((rc = leave(ctx, stream))) return rc;
    if (!same) {
        if (S.w != 0) RT3_HIP(hipEventSynchronize(ctx->ev_acc));    // the old copy is freed: nothing may still read it (the new descriptor is behind the event)
        S.texels = std::move(fresh);
    }
    S.w = w; S.h = h; S.wrap = wrap;
    return 0;
}
// A binding of n entries from device arrays (the host forms stage theirs): the check of the caller's slots with the call's one wait, then — nothing of
// the context has been touched so far — the copies into the context's own arrays behind the event chain.
int install_binding(rt3_ctx* ctx, bool mesh, const void* d_slots, const void* d_uv6, uint32_t n, void* stream_) {
    hipStream_t stream;
    int rc;
    if ((rc = ensure_tex_slots(ctx)) || (rc = ctx->d_tex_check.ensure(ctx, 1u + RT3_TEX_MAX_TEXTURES / 32u))) return rc;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    uint32_t h[1u + RT3_TEX_MAX_TEXTURES / 32u];
    RT3_HIP(hipMemsetAsync(ctx->d_tex_check.get(), 0xFF, 4, stream));
    RT3_HIP(hipMemsetAsync(ctx->d_tex_check.get() + 1, 0, sizeof h - 4, stream));
    hipLaunchKernelGGL(k_tex_check_binding, build_grid(n), dim3(kBlock), 0, stream, (const uint32_t*)d_slots, n, ctx->d_tex_check.get());
    RT3_HIP(hipGetLastError());
    RT3_HIP(hipMemcpyAsync(h, ctx->d_tex_check.get(), sizeof h, hipMemcpyDeviceToHost, stream));
    RT3_HIP(hipStreamSynchronize(stream));
    if (h[0] != 0xFFFFFFFFu)
        return fail(ctx, RT3_E_ARG, std::string(mesh ? "face " : "sphere ") + std::to_string(h[0]) + ": its texture slot is neither RT3_TEX_NONE nor < " +
                                    std::to_string(RT3_TEX_MAX_TEXTURES));
    DevBuf<uint32_t>& bind = mesh ? ctx->d_tri_tex : ctx->d_sph_tex;
    if ((rc = bind.ensure(ctx, n)) || (mesh && (rc = ctx->d_tri_uv.ensure(ctx, (size_t)n * 3u)))) return rc;      // (grows behind hipFree's own wait)
    RT3_HIP(hipMemcpyAsync(bind.get(), d_slots, (size_t)n * 4u, hipMemcpyDeviceToDevice, stream));
    if (mesh) RT3_HIP(hipMemcpyAsync(ctx->d_tri_uv.get(), d_uv6, (size_t)n * 6u * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if ((rc = leave(ctx, stream))) return rc;
    std::memcpy(mesh ? ctx->tri_tex_used : ctx->sph_tex_used, h + 1, sizeof ctx->sph_tex_used);
    return 0;
}
// What both forms of a binding check first.  unbind: the call is the class's unbinding (NULL slots or a count of 0).
int binding_checks(rt3_ctx* ctx, bool mesh, const void* slots, const void* uv6, uint32_t n, bool* unbind) {
    *unbind = slots == nullptr || n == 0;
    if (*unbind) return 0;
    const uint32_t have = mesh ? ctx->n_faces : ctx->n_sph;
    if (have == 0) return fail(ctx, RT3_E_STATE, mesh ? "no committed mesh to bind textures to: call rt3_set_mesh / rt3_mesh_commit first"
                                                      : "no spheres to bind textures to: call rt3_set_spheres first");
    if (n != have) return fail(ctx, RT3_E_ARG, mesh ? "n_faces must equal the context's face count" : "n must equal the context's sphere count");
    if (mesh && !uv6) return fail(ctx, RT3_E_ARG, "uv6 is NULL");
    return 0;
}
}  // namespace

int rt3_set_texture_device(rt3_ctx* ctx, uint32_t slot, const void* d_rgba, uint32_t w, uint32_t h, uint32_t wrap, void* stream) {
    if (!ctx) return RT3_E_ARG;
    int rc = texture_checks(ctx, slot, d_rgba, w, h, wrap);
    if (rc) return rc;
    RT3_HIP(hipSetDevice(ctx->device));
    if (w == 0 || h == 0) return free_texture(ctx, slot, stream);
    if ((uintptr_t)d_rgba % 16u != 0) return fail(ctx, RT3_E_ARG, "d_rgba must be 16-byte aligned");
    return install_texture(ctx, slot, d_rgba, hipMemcpyDeviceToDevice, w, h, wrap, stream);
}
int rt3_set_texture(rt3_ctx* ctx, uint32_t slot, const float* rgba, uint32_t w, uint32_t h, uint32_t wrap) {
    if (!ctx) return RT3_E_ARG;
    int rc = texture_checks(ctx, slot, rgba, w, h, wrap);
    if (rc) return rc;
    RT3_HIP(hipSetDevice(ctx->device));
    if (w == 0 || h == 0) return free_texture(ctx, slot, ctx->stream);
    if ((uintptr_t)rgba % 4u != 0) return fail(ctx, RT3_E_ARG, "rgba must be 4-byte aligned");
    const size_t texels = (size_t)w * h;
    for (size_t i = 0; i < texels; i++)
        if (!std::isfinite(rgba[4 * i]) || !std::isfinite(rgba[4 * i + 1]) || !std::isfinite(rgba[4 * i + 2]))
            return fail(ctx, RT3_E_ARG, "texel " + std::to_string(i) + " is not finite");
    if ((rc = install_texture(ctx, slot, rgba, hipMemcpyHostToDevice, w, h, wrap, ctx->stream))) return rc;        // (no staging buffer: a large image would stay in it)
    RT3_HIP(hipStreamSynchronize(ctx->stream));                     // the caller's array is free again
    return 0;
}
int rt3_clear_textures(rt3_ctx* ctx) {
    if (!ctx) return RT3_E_ARG;
    RT3_HIP(hipSetDevice(ctx->device));
    drop_sphere_binding(ctx);
    drop_mesh_binding(ctx);
    for (uint32_t s = 0; s < RT3_TEX_MAX_TEXTURES; s++) {
        const int rc = free_texture(ctx, s, ctx->stream);
        if (rc) return rc;
    }
    return 0;
}
int rt3_texture_size(rt3_ctx* ctx, uint32_t slot, uint32_t* w, uint32_t* h, uint32_t* wrap) {
    if (!ctx) return RT3_E_ARG;
    if (slot >= RT3_TEX_MAX_TEXTURES) return fail(ctx, RT3_E_ARG, "slot must be < " + std::to_string(RT3_TEX_MAX_TEXTURES));
    if (w) *w = ctx->tex[slot].w;
    if (h) *h = ctx->tex[slot].h;
    if (wrap) *wrap = ctx->tex[slot].wrap;
    return 0;
}
int rt3_bind_sphere_textures_device(rt3_ctx* ctx, const void* d_slots, uint32_t n, void* stream) {
    if (!ctx) return RT3_E_ARG;
    bool unbind;
    int rc = binding_checks(ctx, false, d_slots, nullptr, n, &unbind);
    if (rc) return rc;
    if (unbind) { drop_sphere_binding(ctx); return 0; }
    if ((uintptr_t)d_slots % 4u != 0) return fail(ctx, RT3_E_ARG, "d_slots must be 4-byte aligned");
    return install_binding(ctx, false, d_slots, nullptr, n, stream);
}
int rt3_bind_sphere_textures(rt3_ctx* ctx, const uint32_t* slots, uint32_t n) {
    if (!ctx) return RT3_E_ARG;
    bool unbind;
    int rc = binding_checks(ctx, false, slots, nullptr, n, &unbind);
    if (rc) return rc;
    if (unbind) { drop_sphere_binding(ctx); return 0; }
    if ((uintptr_t)slots % 4u != 0) return fail(ctx, RT3_E_ARG, "slots must be 4-byte aligned");
    for (uint32_t i = 0; i < n; i++)
        if (slots[i] != RT3_TEX_NONE && slots[i] >= RT3_TEX_MAX_TEXTURES)
            return fail(ctx, RT3_E_ARG, "sphere " + std::to_string(i) + ": its texture slot is neither RT3_TEX_NONE nor < " + std::to_string(RT3_TEX_MAX_TEXTURES));
    return staged(ctx, { stage_in(slots, (size_t)n * 4u) }, [&](void* const* d) { return install_binding(ctx, false, d[0], nullptr, n, ctx->stream); });
}
int rt3_bind_mesh_textures_device(rt3_ctx* ctx, const void* d_slots, const void* d_uv6, uint32_t n_faces, void* stream) {
    if (!ctx) return RT3_E_ARG;
    bool unbind;
    int rc = binding_checks(ctx, true, d_slots, d_uv6, n_faces, &unbind);
    if (rc) return rc;
    if (unbind) { drop_mesh_binding(ctx); return 0; }
    if (((uintptr_t)d_slots | (uintptr_t)d_uv6) % 4u != 0) return fail(ctx, RT3_E_ARG, "d_slots and d_uv6 must be 4-byte aligned");
    return install_binding(ctx, true, d_slots, d_uv6, n_faces, stream);
}
int rt3_bind_mesh_textures(rt3_ctx* ctx, const uint32_t* slots, const float* uv6, uint32_t n_faces) {
    if (!ctx) return RT3_E_ARG;
    bool unbind;
    int rc = binding_checks(ctx, true, slots, uv6, n_faces, &unbind);
    if (rc) return rc;
    if (unbind) { drop_mesh_binding(ctx); return 0; }
    if (((uintptr_t)slots | (uintptr_t)uv6) % 4u != 0) return fail(ctx, RT3_E_ARG, "slots and uv6 must be 4-byte aligned");
    for (uint32_t i = 0; i < n_faces; i++)
        if (slots[i] != RT3_TEX_NONE && slots[i] >= RT3_TEX_MAX_TEXTURES)
            return fail(ctx, RT3_E_ARG, "face " + std::to_string(i) + ": its texture slot is neither RT3_TEX_NONE nor < " + std::to_string(RT3_TEX_MAX_TEXTURES));
    for (size_t i = 0; i < (size_t)n_faces * 6u; i++)
        if (!std::isfinite(uv6[i])) return fail(ctx, RT3_E_ARG, "face " + std::to_string(i / 6u) + ": a uv coordinate is not finite");
    return staged(ctx, { stage_in(slots, (size_t)n_faces * 4u), stage_in(uv6, (size_t)n_faces * 6u * sizeof(float)) },
                  [&](void* const* d) { return install_binding(ctx, true, d[0], d[1], n_faces, ctx->stream); });
}

// Tests only: a sampling table of n entries downloaded, built first (ensure) if no call that carries its flag has built it yet.
static int download_table(rt3_ctx* ctx, int (*ensure)(rt3_ctx*, hipStream_t), const DevBuf<uint32_t>& q, const DevBuf<unsigned long long>& cdf, size_t n,
                          uint32_t* q_out, uint64_t* cdf_out) {
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, nullptr, &stream)) || (rc = ensure(ctx, stream))) return rc;
    RT3_HIP(hipMemcpyAsync(q_out, q.get(), n * 4u, hipMemcpyDeviceToHost, stream));
    RT3_HIP(hipMemcpyAsync(cdf_out, cdf.get(), n * 8u, hipMemcpyDeviceToHost, stream));
    if ((rc = leave(ctx, stream))) return rc;
    RT3_HIP(hipStreamSynchronize(stream));
    return 0;
}
int rt3_debug_environment_table(rt3_ctx* ctx, uint32_t* q_out, uint64_t* cdf_out, uint64_t capacity_cells, uint32_t* m_out) {
    if (!ctx) return RT3_E_ARG;
    if (!q_out || !cdf_out || !m_out) return fail(ctx, RT3_E_ARG, "q_out / cdf_out / cells_per_edge is NULL");
    if (ctx->env_n == 0) return fail(ctx, RT3_E_STATE, "no environment map: call rt3_set_environment first");
    const uint32_t m = rt3env::cells_per_edge(ctx->env_n);
    const size_t cells = (size_t)6 * m * m;
    *m_out = m;
    if (capacity_cells < cells) return fail(ctx, RT3_E_ARG, "capacity_cells is smaller than the table (6 x cells_per_edge^2 cells)");
    return download_table(ctx, ensure_env_table, ctx->d_env_q, ctx->d_env_cdf, cells, q_out, cdf_out);
}
int rt3_debug_light_table(rt3_ctx* ctx, uint32_t* q_out, uint64_t* cdf_out, uint64_t capacity, uint32_t* n_entries) {
    if (!ctx) return RT3_E_ARG;
    if (!q_out || !cdf_out || !n_entries) return fail(ctx, RT3_E_ARG, "q_out / cdf_out / n_entries is NULL");
    int rc;
    if ((rc = check_scene(ctx))) return rc;
    const size_t n = (size_t)ctx->n_faces + ctx->n_sph;
    *n_entries = (uint32_t)n;
    if (capacity < n) return fail(ctx, RT3_E_ARG, "capacity is smaller than the table (one entry per face and per sphere)");
    return download_table(ctx, ensure_light_table, ctx->d_light_q, ctx->d_light_cdf, n, q_out, cdf_out);
}

}  // extern "C"
