// rt3_device.hip — the render path on gfx950 (CDNA4): HIP kernels + the device half of the C ABI (include/rt3.h).
//
//   rt3_kernel_common.hpp   constants, arithmetic helpers, Mode-X launch arguments, start_path()
//   rt3_path.hpp            refill (ballot + prefix count, ray stock; the caller's rays of queries and of rt3_radiance*) and shade_lane()
//   rt3_valu_scan.hpp       k_mode_r      Mode R: SequentialRenderer::render + ray_color (src/lib/renderer/SequentialRenderer.cpp:47-109,
//                                         269-308; GLSL twin src/lib/shaders/raytracer_v3.glsl:91-143,187-203), one thread per pixel,
//                                         IEEE arithmetic in the reference's order
//                           k_mode_r_fast the same through a conservative bounding-sphere scan on the vector ALU
//                           k_trace       Mode X: the recursion of the (unfinished) raytracer_v4.glsl:187-290 flattened into an
//                                         iterative per-wavefront loop; every lane carries one path, lanes whose path ended are
//                                         refilled by ballot + prefix count, ray state never leaves the registers
//   rt3_matrix_filter.hpp   k_trace_mfma / k_trace_mfma_tiled / k_mode_r_mfma: the same loops with the candidate search on the
//                           matrix cores (the default; RT3_NO_MFMA=1 selects the VALU scans)
//   rt3_reduce.hpp          per-sample radiance (SampleStorage of raytracer_v4.glsl:107-111) summed in sample order and resolved
//                           (the reduce pass reduce_v1.glsl never got) — the image is bitwise independent of scheduling and GPU count
//   rt3_adaptive.hpp        adaptive sampling (rt3_render_path_adaptive*): the reduce pass over an active list, the convergence rule, the
//                           ordered compaction of the pixels that stay active, the resolves by a pixel's own count
//   rt3_texture_law.hpp     image textures: the lookup and the (u, v) of a sphere and of a face, host and device (the texture forms: 5.2u)
//   rt3_aov.hpp             camera rays as records, first-hit AOVs over the query engine, the linear float resolve (in place for 4.18)
//   rt3_filter_frags.hpp    the sphere side of the matrix filter's operands, the group sizes (no kernel; shared with rt3_scene.hip)
//   rt3_shared_kernels.hpp  k_fill_words and block_sum (shared with rt3_scene.hip: a copy per unit)
//   rt3_ctx.hpp             the device context (struct rt3_ctx, DevBuf) and what every entry point shares: RT3_HIP, fail, enter / leave, staged
//   rt3_scene.hpp           what this unit calls in rt3_scene.hip: check_scene, ensure_env_table, ensure_light_table
//   below                   the host side of the render path and its extern "C" entry points: create and destroy, the renders, queries, AOVs, lenses,
//                           radiance, the accumulation, the gather and the stats
// The other entry points live with their kernels, in units of their own that include rt3_ctx.hpp as this one does (the unit map: DESIGN.md 5.6):
//   rt3_scene.hip             the scene on the context: uploads, rt3_update_*, rt3_regroup*, the environment map, textures, the sampling tables
//   rt3_denoise.hip           rt3_denoise*, rt3_denoise_temporal*, rt3_motion* 
//   rt3_display.hip           rt3_display*, rt3_debug_display_state
//   rt3_display_sequence.hip  rt3_display_sequence*, rt3_debug_display_bloom
//
// Compiled with -ffp-contract=off: a*b+c is two roundings unless written __builtin_fmaf.  Division and sqrt are
// the correctly rounded forms (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt), f32 denormals are kept.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "rt3.h"

#include "rt3_ctx.hpp"
#include "rt3_scene.hpp"
#include "rt3_env_sample.hpp"
#include "rt3_light_sample.hpp"
#include "rt3_lens_law.hpp"
#include "rt3_texture_law.hpp"
#include "rt3_aov_chain_law.hpp"
#include "rt3_kernel_common.hpp"
#include "rt3_filter_frags.hpp"
#include "rt3_path.hpp"
#include "rt3_valu_scan.hpp"
#include "rt3_matrix_filter.hpp"
#include "rt3_level_filter.hpp"
#include "rt3_reduce.hpp"
#include "rt3_shared_kernels.hpp"
#include "rt3_adaptive.hpp"
#include "rt3_aov.hpp"
#include "rt3_lens.hpp"
#include "rt3_primary_lists.hpp"

// ======================================================================================================
// Host side of the device context
// ======================================================================================================
namespace {

thread_local std::string g_create_error;

CamDev cam_dev(const rt3_camera* c) {
    return CamDev{ c->origin[0], c->origin[1], c->origin[2], c->horizontal[0], c->horizontal[1], c->horizontal[2],
                   c->vertical[0], c->vertical[1], c->vertical[2],
                   c->lower_left_corner[0], c->lower_left_corner[1], c->lower_left_corner[2] };
}

int take_event_pair(rt3_ctx* ctx, hipEvent_t* a, hipEvent_t* b) {
    if (ctx->ev_used == ctx->ev.size()) {
        hipEvent_t x, y;
        RT3_HIP(hipEventCreate(&x));
        RT3_HIP(hipEventCreate(&y));
        ctx->ev.emplace_back(x, y);
    }
    *a = ctx->ev[ctx->ev_used].first;
    *b = ctx->ev[ctx->ev_used].second;
    ctx->ev_used++;
    return 0;
}

FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{ 0u, 0xFFFFFFFFu };
    if (d <= 1) return f;
    const uint32_t p = 31u - (uint32_t)__builtin_clz(d);
    if ((d & (d - 1)) == 0) { f.magic = 0; f.shift = p - 1; return f; }
    const uint64_t num = 1ull << (32 + p);
    uint64_t m = num / d;
    const uint64_t rem = num % d;
    m += m;
    const uint64_t twice = rem + rem;
    if (twice >= d) m += 1;
    f.magic = (uint32_t)(m + 1);
    f.shift = p;
    return f;
}
uint32_t fastdiv_host(uint32_t n, FastDiv f) {
    if (f.shift == 0xFFFFFFFFu) return n;
    const uint32_t q = (uint32_t)(((uint64_t)f.magic * n) >> 32);
    return (((n - q) >> 1) + q) >> f.shift;
}
// exhaustive near multiples + a pseudo-random sweep; a wrong magic would silently shift pixels
bool fastdiv_ok(uint32_t d, uint32_t n_max) {
    if (d == 0) return false;
    const FastDiv f = make_fastdiv(d);
    uint32_t x = 0x9E3779B9u;
    for (uint32_t i = 0; i < 4096; i++) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        const uint32_t n = x % (n_max + 1u);
        if (fastdiv_host(n, f) != n / d) return false;
    }
    for (uint64_t k = 0; k <= 64 && k * d <= n_max; k++) {
        const uint64_t m = (uint64_t)(n_max / d - k) * d;
        for (int o = -1; o <= 1; o++) {
            const int64_t n = (int64_t)m + o;
            if (n >= 0 && n <= (int64_t)n_max && fastdiv_host((uint32_t)n, f) != (uint32_t)n / d) return false;
        }
    }
    return true;
}

bool row_owned(const rt3_params* p, uint32_t y) {
    if (p->tile_count <= 1) return true;
    return ((y / p->tile_rows) % p->tile_count) == p->tile_index;
}

// Workgroups per CU of `kernel` with `lds` bytes of dynamic LDS; the attribute and the query run once per (kernel, lds).
int blocks_per_cu(rt3_ctx* ctx, const void* kernel, int block, size_t lds, int* out) {
    const auto key = std::make_pair(kernel, lds);
    const auto it = ctx->occupancy.find(key);
    if (it != ctx->occupancy.end()) { *out = it->second; return 0; }
    if (lds > 48 * 1024) RT3_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int n = 0;
    RT3_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, lds));
    ctx->occupancy[key] = n;
    *out = n;
    return 0;
}

bool same_bytes(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

int check_params(rt3_ctx* ctx, const rt3_params* p, uint32_t min_edge = 2) {
    if (!p) return fail(ctx, RT3_E_ARG, "params is NULL");
    if (!(p->t_min >= 0.0f) || !(p->t_min < __builtin_inff())) return fail(ctx, RT3_E_ARG, "t_min must be finite and >= 0");
    if (p->flags & ~(RT3_FLAG_GAMMA2 | RT3_FLAG_BLACK_BACKGROUND | RT3_FLAG_REFERENCE_PRIMARY | RT3_FLAG_VARIANCE | RT3_FLAG_ENV_SAMPLING | RT3_FLAG_LIGHT_SAMPLING))
        return fail(ctx, RT3_E_ARG, "unknown bits in flags");
    if (p->width < min_edge || p->height < min_edge) return fail(ctx, RT3_E_ARG, "width and height must be >= " + std::to_string(min_edge));
    if ((uint64_t)p->width * p->height > 0x7FFFFFFFull) return fail(ctx, RT3_E_ARG, "frame too large");
    if (p->spp < 1 || p->max_depth < 1) return fail(ctx, RT3_E_ARG, "spp and max_depth must be >= 1");
    if (p->tile_count > 1 && (p->tile_rows == 0 || p->tile_index >= p->tile_count))
        return fail(ctx, RT3_E_ARG, "bad tile_rows / tile_index / tile_count");
    return 0;
}

// RT3_FLAG_ENV_SAMPLING in the flags of a render or of rt3_radiance* (rt3.h): the flags it excludes first, then the map it needs.
int check_env_sampling(rt3_ctx* ctx, uint32_t flags) {
    if (!(flags & RT3_FLAG_ENV_SAMPLING)) return 0;
    if (flags & (RT3_FLAG_BLACK_BACKGROUND | RT3_FLAG_REFERENCE_PRIMARY))
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_ENV_SAMPLING cannot be combined with RT3_FLAG_BLACK_BACKGROUND or RT3_FLAG_REFERENCE_PRIMARY");
    if (ctx->env_n == 0) return fail(ctx, RT3_E_STATE, "RT3_FLAG_ENV_SAMPLING needs an environment map: call rt3_set_environment first");
    return 0;
}

// RT3_FLAG_LIGHT_SAMPLING in the flags of a render or of rt3_radiance* (rt3.h): the flags it excludes, each with an answer of its own.
int check_light_sampling(rt3_ctx* ctx, uint32_t flags) {
    if (!(flags & RT3_FLAG_LIGHT_SAMPLING)) return 0;
    if (flags & RT3_FLAG_ENV_SAMPLING)
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_LIGHT_SAMPLING cannot be combined with RT3_FLAG_ENV_SAMPLING (one shadow ray per scatter)");
    if (flags & RT3_FLAG_REFERENCE_PRIMARY) return fail(ctx, RT3_E_ARG, "RT3_FLAG_LIGHT_SAMPLING cannot be combined with RT3_FLAG_REFERENCE_PRIMARY");
    return 0;
}

// Image textures.  A class is bound while its binding names a slot; the context is textured while a class with primitives is bound.
bool any_slot(const uint32_t (&used)[RT3_TEX_MAX_TEXTURES / 32]) { uint32_t a = 0; for (uint32_t w : used) a |= w; return a != 0; }
bool textured(const rt3_ctx* ctx) { return (ctx->n_sph != 0 && any_slot(ctx->sph_tex_used)) || (ctx->n_faces != 0 && any_slot(ctx->tri_tex_used)); }
// What a launch of a textured context hands over; all null otherwise.
TexTable tex_table(const rt3_ctx* ctx) {
    TexTable X{ nullptr, nullptr, nullptr, nullptr };
    if (!textured(ctx)) return X;
    X.slots = ctx->d_tex_slots;
    if (ctx->n_sph != 0 && any_slot(ctx->sph_tex_used)) X.sph_tex = ctx->d_sph_tex;
    if (ctx->n_faces != 0 && any_slot(ctx->tri_tex_used)) { X.tri_tex = ctx->d_tri_tex; X.tri_uv = ctx->d_tri_uv; }
    return X;
}
// An entry point that reads the textures (rt3.h), called with its flags: nothing while the context is not textured; the flags refused while it is, then
// every slot a binding names must hold a texture.
int check_textures(rt3_ctx* ctx, uint32_t flags) {
    if (!textured(ctx)) return 0;
    if (flags & RT3_FLAG_REFERENCE_PRIMARY)
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_REFERENCE_PRIMARY is not available while textures are bound (its primary direction is not a unit vector)");
    if (flags & (RT3_FLAG_ENV_SAMPLING | RT3_FLAG_LIGHT_SAMPLING))
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_ENV_SAMPLING and RT3_FLAG_LIGHT_SAMPLING are not available while textures are bound "
                                    "(the sampling tables' weights do not see the texels)");
    for (uint32_t s = 0; s < RT3_TEX_MAX_TEXTURES; s++) {
        const bool named = (ctx->n_sph != 0 && ((ctx->sph_tex_used[s / 32] >> (s % 32)) & 1u)) || (ctx->n_faces != 0 && ((ctx->tri_tex_used[s / 32] >> (s % 32)) & 1u));
        if (named && ctx->tex[s].w == 0) return fail(ctx, RT3_E_STATE, "a binding names texture slot " + std::to_string(s) + ", which is empty: call rt3_set_texture first");
    }
    return 0;
}

// The scene half of TraceArgs (what renders and queries share): records, filter centres, direct spheres, counters.
TraceArgs scene_args(const rt3_ctx* ctx) {
    TraceArgs A;
    std::memset(&A, 0, sizeof A);
    A.sph = ctx->d_sph; A.sph_invr = ctx->d_sph_invr; A.sph_mat = ctx->d_sph_mat; A.sph_kind = ctx->d_sph_kind; A.n_sph = ctx->n_sph;
    A.tri = ctx->d_tri; A.tri_mat = ctx->d_tri_mat; A.tri_kind = ctx->d_tri_kind; A.tri_bound = ctx->d_tri_bound; A.n_tri = ctx->n_faces;
    A.work_counter = ctx->d_work; A.cast_counter = ctx->d_casts;
    A.fcx = ctx->sph_centre[0]; A.fcy = ctx->sph_centre[1]; A.fcz = ctx->sph_centre[2];
    A.tcx = ctx->tri_centre[0]; A.tcy = ctx->tri_centre[1]; A.tcz = ctx->tri_centre[2];
    A.n_direct = ctx->n_direct;
    for (int i = 0; i < 4; i++) A.direct[i] = ctx->direct[i];
    return A;
}

bool cam_at_origin(const rt3_camera* cam) { return cam->origin[0] == 0.0f && cam->origin[1] == 0.0f && cam->origin[2] == 0.0f; }

// The camera and params half of TraceArgs (on top of scene_args): what start_path() reads to turn an item (sample in batch, owned pixel) into
// Mode X's primary ray.  Renders and the camera-ray / AOV passes (rt3_aov.hpp) share it; s0 and total are set per batch by the caller.
int path_args(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t npix, TraceArgs& A) {
    A = scene_args(ctx);
    A.cam = cam_dev(cam);
    A.lens_radius = p->lens_radius;
    {
        const float* h = cam->horizontal; const float* v = cam->vertical;
        const float lh = std::sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
        const float lv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        A.lux = h[0] / lh; A.luy = h[1] / lh; A.luz = h[2] / lh;
        A.lvx = v[0] / lv; A.lvy = v[1] / lv; A.lvz = v[2] / lv;
    }
    A.width = p->width; A.height = p->height; A.spp = p->spp; A.max_depth = p->max_depth; A.seed = p->seed; A.flags = p->flags;
    {
        uint32_t e = (uint32_t)std::sqrt((double)p->spp);
        while (e * e > p->spp) e--;
        while ((e + 1) * (e + 1) <= p->spp) e++;
        A.edge = (e * e == p->spp && p->spp > 1) ? e : 0;          // stratified only for perfect squares (v4:199)
    }
    A.t_min = p->t_min;
    A.tile_rows = p->tile_rows; A.tile_index = p->tile_index; A.tile_count = p->tile_count;
    A.npix = npix;
    A.div_npix = make_fastdiv(npix); A.div_width = make_fastdiv(p->width);
    A.div_edge = make_fastdiv(A.edge ? A.edge : 1); A.div_tile_rows = make_fastdiv(p->tile_count > 1 ? p->tile_rows : 1);
    if (!fastdiv_ok(npix, 0x7FFFFFFFu) || !fastdiv_ok(p->width, 0x7FFFFFFFu) || !fastdiv_ok(A.edge ? A.edge : 1, p->spp) ||
        !fastdiv_ok(p->tile_count > 1 ? p->tile_rows : 1, p->height))
        return fail(ctx, RT3_E_DEVICE, "internal: magic-number division self-check failed");
    return 0;
}

// ---- which trace kernel: ONE rule for every form (Form, rt3_kernel_common.hpp; the table of forms and families: DESIGN.md 5.2m)
//   brute         every ray against every primitive (debug switch / RT3_BRUTE=1; REFERENCE_PRIMARY with a camera off the origin or a lens)
//   mfma_single   sphere scenes of <= 512 spheres, everything in LDS (the bench kernel)
//   mfma tiled    every other scene
//   valu          RT3_NO_MFMA=1: the vector-ALU scans (A/B reference; renders only)
// Queries and rays have no form of the VALU kernels, of K = 64 or of the flat filter: they ignore those switches (rt3.h).
using TraceKernel = void (*)(const TraceArgs);
using TiledKernel = void (*)(const TraceArgs, const u32x4*, const u32x4*);
using SingleKernel = void (*)(const TraceArgs, const u32x4*, uint32_t);
// The same three signatures by form: an environment form takes an EnvTraceArgs (rt3_kernel_common.hpp).  TracePlan keeps such a kernel under the
// plain pointer type with env_n != 0; launch_trace casts it back before it launches.
template <Form F> using TraceKernelOf = void (*)(const trace_args<F>);
template <Form F> using TiledKernelOf = void (*)(const trace_args<F>, const u32x4*, const u32x4*);
template <Form F> using SingleKernelOf = void (*)(const trace_args<F>, const u32x4*, uint32_t);
struct TracePlan {
    TraceKernel plain = nullptr;
    TiledKernel tiled = nullptr;
    SingleKernel single = nullptr;                                  // k_trace_mfma32 | k_trace_mfma (RT3_MFMA_K64)
    const u32x4* frag_a = nullptr; const u32x4* frag_b = nullptr;   // tiled: faces' and spheres' rows; single: the spheres' fragments in frag_a
    uint32_t mfma_blocks = 0;
    size_t lds = 0;
    int block = kBlock;
    int per_cu = 0;                                                 // workgroups per CU the launch configuration allows (<= 8)
    bool mfma16 = false;                                            // rt3_stats::mfma_flop_per_instruction: 16x16x32 (tiled kernels, k_trace_mfma32)
    uint64_t filter_rows = 0;                                       // rows the matrix filter scans per ray cast
    bool filter_counted = false;                                    // the kernel counts the casts that take the filter (k_trace_mfma32's render form)
    uint32_t list_groups = 0;                                       // strip lists to build before the first batch (k_primary_lists): groups of 64 owned pixels, 0: none
    const float4* env = nullptr; uint32_t env_n = 0;                // environment forms: the map the launch hands over behind TraceArgs (env_n != 0)
    const uint32_t* nee_q = nullptr; const unsigned long long* nee_cdf = nullptr; uint32_t nee_m = 0;      // sampling forms: the table behind the map (nee_m != 0)
    const uint32_t* lt_q = nullptr; const unsigned long long* lt_cdf = nullptr; const float4* lt_sph_cr = nullptr; uint32_t lt_n = 0;   // light sampling forms: the emitters' table (lt_n != 0)
    TexTable tex{ nullptr, nullptr, nullptr, nullptr };             // texture forms: the slot table and the bindings behind the map (tex.slots != null)
};
// Strip lists (rt3_primary_lists.hpp): RT3_PRIMARY_LISTS=0 turns them off (the A/B reference: every primary ray takes the matrix filter),
// RT3_PRIMARY_LIST_MAX=n sets the longest list a restock still traces itself.  The default is the best of a sweep on the bench frame at 1080p (short
// lists) and at 400x225 (long ones): profiles/primary_lists_mi355x.log.
constexpr uint32_t kPrimaryListMax = 32;
void launch_primary_lists(const rt3_ctx* ctx, const TraceArgs& A, uint32_t n_groups, uint32_t n_blocks, hipStream_t stream) {
    constexpr uint32_t per_block = kBlock / 64;
    hipLaunchKernelGGL(k_primary_lists, dim3((n_groups + per_block - 1) / per_block), dim3(kBlock), 0, stream, A, n_groups, n_blocks, ctx->d_prim_masks.get());
}
// The instantiation of each kernel family for a form and a scene.  by_scene writes the face / sphere choice once: pick(HAS_TRI, HAS_SPH) as
// integral constants; RenderRef exists for face-only scenes alone.  A (form, family) pair that does not exist is not instantiated (the kernels'
// static_asserts would refuse it): the answer is nullptr, which plan_trace reports as an internal error.
template <Form F, class Pick>
auto by_scene(bool has_tri, bool has_sph, Pick pick) -> decltype(pick(std::true_type{}, std::false_type{})) {
    if constexpr (F == Form::RenderRef) return has_tri && !has_sph ? pick(std::true_type{}, std::false_type{}) : nullptr;
    else return has_tri ? (has_sph ? pick(std::true_type{}, std::true_type{}) : pick(std::true_type{}, std::false_type{})) : pick(std::false_type{}, std::true_type{});
}
template <Form F>
TiledKernelOf<F> levels_kernel(uint32_t levels, bool resident, bool has_tri, bool has_sph) {
    return by_scene<F>(has_tri, has_sph, [=](auto tri, auto sph) -> TiledKernelOf<F> {
        constexpr bool T = tri(), S = sph();
        return levels == 4 ? (resident ? k_trace_levels<T, S, F, 4, true> : k_trace_levels<T, S, F, 4, false>)
                           : (resident ? k_trace_levels<T, S, F, 3, true> : k_trace_levels<T, S, F, 3, false>);
    });
}
template <Form F>
TiledKernelOf<F> tiled_kernel(bool grouped, bool resident, bool has_tri, bool has_sph) {
    return by_scene<F>(has_tri, has_sph, [=](auto tri, auto sph) -> TiledKernelOf<F> {
        constexpr bool T = tri(), S = sph();
        constexpr uint32_t GT = T ? kGroupTri : 1u, GS = S ? kGroupSph : 1u;       // (a pass over one kind of primitive alone keeps the other's group size 1)
        if (resident) return k_trace_mfma_tiled<T, S, F, GT, GS, kSuper, true>;
        if (grouped) return k_trace_mfma_tiled<T, S, F, GT, GS, kSuper, false>;
        if constexpr (F == Form::Query || F == Form::Rays || is_env(F)) return nullptr;   // the flat filter
        else return k_trace_mfma_tiled<T, S, F, 1, 1, 1, false>;
    });
}
template <Form F>
SingleKernelOf<F> single_kernel(bool k64) {
    if constexpr (F == Form::Render || F == Form::List) return k64 ? k_trace_mfma<F> : k_trace_mfma32<F>;
    else if constexpr (F == Form::RenderRef) return nullptr;
    else return k64 ? nullptr : k_trace_mfma32<F>;
}
template <Form F>
TraceKernelOf<F> valu_kernel(bool sph_lds, bool has_tri, bool has_sph) {
    if constexpr (F == Form::Query || F == Form::Rays || is_env(F)) return nullptr;
    else return by_scene<F>(has_tri, has_sph, [=](auto tri, auto sph) -> TraceKernelOf<F> {
        constexpr bool T = tri(), S = sph();
        return S && sph_lds ? k_trace<T, S, /* SPH_LDS */ S, F> : k_trace<T, S, false, F>;
    });
}
// fn(std::integral_constant<Form, form>): the run-time form as a compile-time one.
// RT3_FORM_MASK (bit f: Form f): the forms whose trace kernels this compilation instantiates — all of them in every build of the library.
// tools/cvt_isa_check.py alone sets it: it reads the listing of every kernel, and compiles the device code as several listings in parallel, each with
// some of the forms (a kernel's code does not depend on which other kernels are compiled beside it).
#ifndef RT3_FORM_MASK
#define RT3_FORM_MASK 0xFFFFFFFFu
#endif
template <Form F, class Fn>
void form_case(Fn& fn) {
    if constexpr (((RT3_FORM_MASK >> (uint32_t)F) & 1u) != 0u) fn(std::integral_constant<Form, F>{});
}
template <class Fn>
void with_form(Form form, Fn fn) {
    switch (form) {
    case Form::Render: return form_case<Form::Render>(fn);
    case Form::RenderRef: return form_case<Form::RenderRef>(fn);
    case Form::Query: return form_case<Form::Query>(fn);
    case Form::List: return form_case<Form::List>(fn);
    case Form::Rays: return form_case<Form::Rays>(fn);
    case Form::RenderEnv: return form_case<Form::RenderEnv>(fn);
    case Form::ListEnv: return form_case<Form::ListEnv>(fn);
    case Form::RaysEnv: return form_case<Form::RaysEnv>(fn);
    case Form::RenderEnvNee: return form_case<Form::RenderEnvNee>(fn);
    case Form::RaysEnvNee: return form_case<Form::RaysEnvNee>(fn);
    case Form::RenderLight: return form_case<Form::RenderLight>(fn);
    case Form::RaysLight: return form_case<Form::RaysLight>(fn);
    case Form::RenderTex: return form_case<Form::RenderTex>(fn);
    case Form::ListTex: return form_case<Form::ListTex>(fn);
    case Form::RaysTex: return form_case<Form::RaysTex>(fn);
    }
}
// Fills A's filter fields and T for the form `form` (rt3_kernel_common.hpp).  ref_brute: a RenderRef with a camera only the brute-force kernel serves.
// List: the kernel a Render would take, strip lists off.  Rays: the kernel a Query would take on this scene — the switches queries ignore are ignored —
// shading as a render; A.q_rays is the caller's to set (its slot is the strip lists': they are off).
// While an environment map is set a Render, List or Rays becomes its environment twin: the same family — the families without such a
// form (VALU, K = 64, the flat filter) are never chosen, their switches are ignored as queries ignore them — and T carries the map for launch_trace.
// nee: the call carries RT3_FLAG_ENV_SAMPLING (a Render or a Rays with a map set and its table built: check_env_sampling, ensure_env_table): the sampling
// twin of the environment form, the same family again; k_trace_mfma32's takes the plain refill, so no strip lists are built for it.
// light: the call carries RT3_FLAG_LIGHT_SAMPLING (a Render or a Rays with the emitters' table built: check_light_sampling, ensure_light_table): the light
// sampling form, which is an environment form whether a map is set or not (env_n == 0: none) and so takes the families an environment form takes.
int plan_trace(rt3_ctx* ctx, TraceArgs& A, Form form, bool ref_brute, TracePlan& T, bool nee = false, bool light = false) {
    const bool query = form == Form::Query, list = form == Form::List, rays = form == Form::Rays;
    const bool map = ctx->env_n != 0 && (form == Form::Render || list || rays);
    const bool tex = textured(ctx) && (form == Form::Render || list || rays);
    const bool env = map || light || tex;
    if (nee && (!map || list || !ctx->env_table || light)) return fail(ctx, RT3_E_DEVICE, "internal: no sampling form for this call");
    if (light && (!(form == Form::Render || rays) || !ctx->light_table)) return fail(ctx, RT3_E_DEVICE, "internal: no light sampling form for this call");
    if (tex && (nee || light)) return fail(ctx, RT3_E_DEVICE, "internal: no texture form under a sampling flag");     // (check_textures refuses the flags)
    if (map) { T.env = ctx->d_env; T.env_n = ctx->env_n; form = form == Form::Render ? Form::RenderEnv : list ? Form::ListEnv : Form::RaysEnv; }
    if (tex) { T.tex = tex_table(ctx); form = rays ? Form::RaysTex : list ? Form::ListTex : Form::RenderTex; }         // (with the map, if one is set)
    if (light) {
        T.lt_q = ctx->d_light_q; T.lt_cdf = ctx->d_light_cdf; T.lt_sph_cr = ctx->d_sph_cr; T.lt_n = ctx->n_faces + ctx->n_sph;
        form = rays ? Form::RaysLight : Form::RenderLight;
    }
    if (nee) { T.nee_q = ctx->d_env_q; T.nee_cdf = ctx->d_env_cdf; T.nee_m = ctx->env_m; form = rays ? Form::RaysEnvNee : Form::RenderEnvNee; }
    const bool has_tri = ctx->n_faces > 0, has_sph = ctx->n_sph > 0;
    const bool brute = ctx->force_brute || getenv("RT3_BRUTE") || ref_brute;
    const bool use_mfma = !brute && (query || rays || env || !getenv("RT3_NO_MFMA"));
    const bool mfma_single = use_mfma && !has_tri && has_sph && ctx->n_sph <= kMfmaSphMax && !getenv("RT3_FORCE_TILED");   // (A/B knob)
    const bool single_k64 = !query && !rays && !env && mfma_single && getenv("RT3_MFMA_K64") != nullptr;
    const bool sph_lds = has_sph && ctx->n_sph <= kSphLdsMax;
    const bool grouped = kGroupTri > 1 && kGroupSph > 1 && (query || rays || env || (!ctx->force_flat && !getenv("RT3_NO_GROUPS")));
    A.n_tri_rows = grouped ? ctx->tri.n_groups : ctx->n_faces;
    A.n_sph_rows = grouped ? ctx->sph.n_groups : ctx->n_sph;
    A.sph_grp = ctx->sph.grp; A.sph_perm = ctx->sph.perm; A.tri_grp = ctx->tri.grp; A.tri_perm = ctx->tri.perm; A.tri_rec = ctx->d_tri_rec;
    A.tri_leaf = ctx->tri.leaf; A.sph_leaf = ctx->sph.leaf; A.n_tri_leaves = ctx->tri.n_leaves; A.n_sph_leaves = ctx->sph.n_leaves;
    A.tri_rowb = ctx->tri.rowb; A.sph_rowb = ctx->sph.rowb;
    T.mfma_blocks = (ctx->n_sph + 31u) / 32u;
    bool resident = false;
    uint32_t levels = 0;                                            // k_trace_levels: 3 | 4
    if (mfma_single) {
        // k_trace_mfma32 (K = 32 form, pair list); RT3_MFMA_K64=1: k_trace_mfma, round 1's K = 64 form on v_mfma_f32_32x32x16_bf16 (A/B reference)
        T.lds = single_k64 ? (size_t)T.mfma_blocks * (4096 + 32 * (16 + 16 + 4 + 4)) + (size_t)kBitmapBytes
                           : (size_t)T.mfma_blocks * (2048 + 32 * (16 + 16 + 4 + 4)) + (size_t)kBitmapBytes + (size_t)kMB * 8 + (size_t)(kMB / 64) * kPairCap * 4;
        if (!single_k64 && !query && RT3_CTR_TABLE) T.lds += kCtrTableBytes;       // the render forms' counter-hash table (shade_lane)
        T.block = kMB;
        T.frag_a = (const u32x4*)(single_k64 ? ctx->d_sph_frag.get() : ctx->d_sph_frag32.get());
        if (!query && !single_k64) {
            T.filter_counted = true;
            const char* on = getenv("RT3_PRIMARY_LISTS"); const char* cap = getenv("RT3_PRIMARY_LIST_MAX");
            if (!rays) A.prim_masks = nullptr;                      // (the slot held the face bounds' address: none in a sphere-only scene; rays: it is q_rays' slot)
            A.prim_list_max = 0;
            if (!list && !rays && !nee && !light && !(on && atoi(on) == 0)) {             // (a list's groups of 64 are not consecutive pixels: no strip lists)
                T.list_groups = (A.npix + 63u) / 64u;
                int rc_;
                if ((rc_ = ctx->d_prim_masks.ensure(ctx, (size_t)T.list_groups * T.mfma_blocks))) return rc_;
                A.prim_masks = ctx->d_prim_masks;
                A.prim_list_max = cap ? (uint32_t)std::min<long>(std::max<long>(atol(cap), 0), (long)kMfmaSphMax) : kPrimaryListMax;
            }
        }
    } else if (use_mfma) {
        // the two-level filter (rows = groups of primitives) unless RT3_NO_GROUPS=1 asks for the flat one (A/B reference, tests)
        constexpr uint32_t SUP = kSuper;
        const uint32_t row_blocks = (has_tri ? (A.n_tri_rows + 31u) / 32u : 0u) + (has_sph ? (A.n_sph_rows + 31u) / 32u : 0u);
        const uint32_t super_blocks = (has_tri ? (ctx->tri.n_super + 31u) / 32u : 0u) + (has_sph ? (ctx->sph.n_super + 31u) / 32u : 0u);
        // While the rows of 64 fit in LDS (<= kResidentBlocks row blocks, 112 000 primitives: both BASELINE scenes) k_trace_mfma_tiled's resident three-level
        // form runs; beyond, k_trace_levels (rt3_level_filter.hpp) with FOUR levels — the matrix cores scan super-rows of 512, resident up to 570 000
        // primitives, through a tile after that.  RT3_LEVELS=3|4 forces k_trace_levels with that many levels, RT3_OLD_GROUPS=1 the nested form (A/B, tests)
        const char* force_levels = getenv("RT3_LEVELS");
        const bool no_res_env = getenv("RT3_NO_RESIDENT") != nullptr;
        const bool lev_kernel = grouped && SUP > 1 && !getenv("RT3_OLD_GROUPS") && (force_levels != nullptr || row_blocks > kResidentBlocks);
        if (lev_kernel) {
            levels = force_levels ? (atoi(force_levels) == 4 ? 4u : 3u) : 4u;
            const uint32_t top_blocks = levels == 4 ? super_blocks : row_blocks;
            resident = !no_res_env && top_blocks <= lev_resident_blocks(levels);
            A.n_tri_top = levels == 4 ? ctx->tri.n_super : ctx->tri.n_groups; A.n_sph_top = levels == 4 ? ctx->sph.n_super : ctx->sph.n_groups;
            A.tri_topb = levels == 4 ? ctx->tri.srowb : ctx->tri.rowb; A.sph_topb = levels == 4 ? ctx->sph.srowb : ctx->sph.rowb;
            T.lds = lev_lds_fixed(levels, resident) + (resident ? (size_t)top_blocks * 2048u : 0u);
        } else {
            resident = grouped && SUP > 1 && row_blocks <= kResidentBlocks && !getenv("RT3_NO_RESIDENT");      // all rows fit in LDS: no tiles, no barriers
            T.lds = resident ? (size_t)row_blocks * 2048u + (size_t)kBmBlocksRes * kTB * 4u + (size_t)kTB * 8u + (size_t)(kTB / 64u) * kPairCap * 4u * 3u : kTraceTiledLdsBytes;
        }
        T.block = kTB;
        if (levels == 4) { T.frag_a = ctx->tri.sfrag; T.frag_b = ctx->sph.sfrag; }
        else { T.frag_a = grouped ? ctx->tri.gfrag : ctx->d_tri_frag; T.frag_b = grouped ? ctx->sph.gfrag.get() : (const u32x4*)ctx->d_sph_frag32.get(); }
    } else if (!brute) {
        T.lds = sph_lds ? (size_t)ctx->n_sph * sizeof(float4) : 0;
    }
    with_form(form, [&](auto f) {                                   // the one place a kernel is named: family x form
        constexpr Form F = decltype(f)::value;
        if (brute) T.plain = reinterpret_cast<TraceKernel>(TraceKernelOf<F>(k_trace_brute<F>));
        else if (mfma_single) T.single = reinterpret_cast<SingleKernel>(single_kernel<F>(single_k64));
        else if (levels) T.tiled = reinterpret_cast<TiledKernel>(levels_kernel<F>(levels, resident, has_tri, has_sph));
        else if (use_mfma) T.tiled = reinterpret_cast<TiledKernel>(tiled_kernel<F>(grouped, resident, has_tri, has_sph));
        else T.plain = reinterpret_cast<TraceKernel>(valu_kernel<F>(sph_lds, has_tri, has_sph));
    });
    const void* kptr = T.single ? (const void*)T.single : T.tiled ? (const void*)T.tiled : (const void*)T.plain;
    if (!kptr) return fail(ctx, RT3_E_DEVICE, "internal: the trace kernel chosen has no such form");
    int rc;
    if ((rc = blocks_per_cu(ctx, kptr, T.block, T.lds, &T.per_cu))) return rc;
    if (T.per_cu < 1) return fail(ctx, RT3_E_DEVICE, "the trace kernel does not fit on a CU");
    T.per_cu = std::min(T.per_cu, 8);
    if (T.tiled && grouped) {                                       // one strip per wave of the largest grid this launch configuration can have
        if ((rc = ctx->d_strips.ensure(ctx, (size_t)ctx->num_cu * T.per_cu * (kTB / 64u) * kStripPairs))) return rc;
        A.pair_strips = ctx->d_strips;
    }
    T.mfma16 = T.tiled != nullptr || (mfma_single && !single_k64);
    T.filter_rows = levels ? (uint64_t)(has_tri ? A.n_tri_top : 0u) + (has_sph ? A.n_sph_top : 0u) : T.tiled ? (uint64_t)A.n_tri_rows + A.n_sph_rows
                  : mfma_single ? ctx->n_sph : 0;
    return 0;
}
// Workgroups for `total` work items: enough for kWorkChunk items per wave, at most what fits on the device at once.
uint32_t trace_grid(const rt3_ctx* ctx, const TracePlan& T, uint32_t total) {
    const uint32_t waves_per_block = (uint32_t)T.block / 64u;
    const uint32_t want_blocks = (total + kWorkChunk * waves_per_block - 1) / (kWorkChunk * waves_per_block);
    return std::max(1u, std::min<uint32_t>((uint32_t)(ctx->num_cu * T.per_cu), want_blocks));
}
// The launch of T's kernel — single, tiled or plain — with the argument struct E of the forms that share F's signatures.
template <Form F, class Args>
void launch_as(const TracePlan& T, const Args& E, uint32_t grid, hipStream_t stream) {
    static_assert(std::is_same<Args, trace_args<F>>::value, "the argument struct of the form the kernel pointer is cast back to");
    if (T.single) hipLaunchKernelGGL(reinterpret_cast<SingleKernelOf<F>>(T.single), dim3(grid), dim3(kMB), T.lds, stream, E, T.frag_a, T.mfma_blocks);
    else if (T.tiled) hipLaunchKernelGGL(reinterpret_cast<TiledKernelOf<F>>(T.tiled), dim3(grid), dim3(kTB), T.lds, stream, E, T.frag_a, T.frag_b);
    else hipLaunchKernelGGL(reinterpret_cast<TraceKernelOf<F>>(T.plain), dim3(grid), dim3(kBlock), T.lds, stream, E);
}
void launch_trace(const TracePlan& T, const TraceArgs& A, uint32_t grid, hipStream_t stream) {
    const auto with_map = [&](EnvTraceArgs& E) { static_cast<TraceArgs&>(E) = A; E.env = T.env; E.env_n = T.env_n; E.env_pad = 0u; };
    if (T.tex.slots != nullptr) {                                   // a texture form: the map (or none), then the slot table and the bindings
        TexTraceArgs E;
        with_map(E);
        E.tex = T.tex;
        launch_as<Form::RenderTex>(T, E, grid, stream);             // (the three texture forms share their signatures)
    } else if (T.lt_n != 0) {                                       // a light sampling form: the map (or none) and the emitters' table behind the arguments
        LightTraceArgs E;
        with_map(E);
        E.lt_q = T.lt_q; E.lt_cdf = (const uint64_t*)T.lt_cdf; E.lt_sph_cr = T.lt_sph_cr; E.lt_n = T.lt_n; E.lt_pad = 0u;
        launch_as<Form::RenderLight>(T, E, grid, stream);           // (the two light sampling forms share their signatures)
    } else if (T.nee_m != 0) {                                      // a sampling form: the map and its table behind the arguments
        NeeTraceArgs E;
        with_map(E);
        E.nee_q = T.nee_q; E.nee_cdf = (const uint64_t*)T.nee_cdf; E.nee_m = T.nee_m; E.nee_cells = 6u * T.nee_m * T.nee_m;
        launch_as<Form::RenderEnvNee>(T, E, grid, stream);          // (the two sampling forms share their signatures)
    } else if (T.env_n != 0) {                                      // an environment form: the same launch with the map behind the arguments
        EnvTraceArgs E;
        with_map(E);
        launch_as<Form::RenderEnv>(T, E, grid, stream);             // (the three environment forms share their signatures)
    } else {
        launch_as<Form::Render>(T, A, grid, stream);
    }
}

// One timed trace launch of a call: the kernel of T over the n work items A describes (a batch of samples; DESIGN.md 4.9: the rays A.q_rays points to).
// Renders, the adaptive rounds, rt3_radiance* and the AOV pass issue it once per sample batch, rt3_intersect* / rt3_occluded* once; the caller records
// ev_begin, clears the counters before the first one and finishes the call (ev_end, ev_acc, the stats fields).
int issue_trace(rt3_ctx* ctx, const TraceArgs& A, const TracePlan& T, uint32_t n, hipStream_t stream) {
    hipEvent_t a, b;
    int rc;
    if ((rc = take_event_pair(ctx, &a, &b))) return rc;
    RT3_HIP(hipMemsetAsync(ctx->d_work, 0, 4, stream));
    RT3_HIP(hipEventRecord(a, stream));
    launch_trace(T, A, trace_grid(ctx, T, n), stream);
    RT3_HIP(hipGetLastError());
    RT3_HIP(hipEventRecord(b, stream));
    return 0;
}

// Samples per batch: as many of `count` as the sample storage cap holds at `bytes` per item and sample, and as keep the item index of a batch over
// n items below 2^31 - 2^16.  0: not even one sample fits the index.
uint32_t sample_batch(const rt3_ctx* ctx, uint32_t count, uint32_t n, size_t bytes) {
    const uint64_t batch = std::min<uint64_t>(count, std::max<uint64_t>(1, ctx->rad_cap_bytes / ((uint64_t)n * bytes)));
    return (uint32_t)std::min<uint64_t>(batch, 0x7FFF0000ull / n);
}
// The accumulation is valid again: what a later rt3_render_path_range must match to continue it, and what rt3_accum_* read.
void commit_accumulation(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t done, uint32_t npix, bool adaptive) {
    ctx->acc_valid = true; ctx->acc_adaptive = adaptive; ctx->acc_params = *p; ctx->acc_cam = *cam; ctx->acc_done = done; ctx->acc_npix = npix;
}
// plan_trace for a call whose flags may carry RT3_FLAG_ENV_SAMPLING or RT3_FLAG_LIGHT_SAMPLING: the tables those flags need first, queued on `stream`.
int plan_sampled_trace(rt3_ctx* ctx, TraceArgs& A, Form form, bool ref_brute, uint32_t flags, hipStream_t stream, TracePlan& T) {
    const bool nee = (flags & RT3_FLAG_ENV_SAMPLING) != 0, light = (flags & RT3_FLAG_LIGHT_SAMPLING) != 0;
    int rc;
    if (nee && (rc = ensure_env_table(ctx, stream))) return rc;
    if (light && (rc = ensure_light_table(ctx, stream))) return rc;
    return plan_trace(ctx, A, form, ref_brute, T, nee, light);
}

// The calls rt3_get_stats reports on (Mode-X renders, queries, AOVs) issue their launches between these two; each clears ctx->rendered before
// anything that can fail, and end_timed sets it once the last launch has been issued.  plan: nullptr when nothing was traced (no owned pixels).
constexpr size_t kCastSlots = 32;                                   // d_casts: [0..15] as the kernels' comments say, [16] casts through the filter, [17] restock phase, [18..22] its parts
int begin_timed(rt3_ctx* ctx, hipStream_t stream) {
    ctx->ev_used = 0;
    RT3_HIP(hipEventRecord(ctx->ev_begin, stream));
    RT3_HIP(hipMemsetAsync(ctx->d_casts, 0, kCastSlots * 8, stream));
    return 0;
}
int end_timed(rt3_ctx* ctx, hipStream_t stream, uint64_t samples, const TracePlan* plan) {
    RT3_HIP(hipEventRecord(ctx->ev_end, stream));
    const int rc = leave(ctx, stream);
    if (rc) return rc;
    ctx->last_stream = stream;
    ctx->last_samples = samples;
    ctx->last_was_path = true;
    if (plan) { ctx->last_mfma16 = plan->mfma16; ctx->last_filter_rows = plan->filter_rows; ctx->last_filter_counted = plan->filter_counted; }
    ctx->rendered = true;
    return 0;
}

}  // namespace

extern "C" {

uint32_t rt3_abi_version(void) { return RT3_ABI_VERSION; }

uint32_t rt3_rows_owned(const rt3_params* p) {
    uint32_t n = 0;
    for (uint32_t y = 0; y < p->height; y++) n += row_owned(p, y) ? 1u : 0u;
    return n;
}
uint32_t rt3_row_of_local(const rt3_params* p, uint32_t local_row) {
    if (p->tile_count <= 1) return local_row;
    const uint32_t lb = local_row / p->tile_rows, in = local_row % p->tile_rows;
    return (lb * p->tile_count + p->tile_index) * p->tile_rows + in;
}

rt3_ctx* rt3_create(int device_id) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_error = std::string("rt3_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
                         "); this library has no CPU fallback";
        return nullptr;
    }
    if (device_id < 0 || device_id >= count) { g_create_error = "rt3_create: device_id out of range"; return nullptr; }
    rt3_ctx* ctx = new rt3_ctx();
    ctx->device = device_id;
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess ||
        (e = hipStreamCreate(&ctx->stream)) != hipSuccess || (e = hipEventCreate(&ctx->ev_begin)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev_end)) != hipSuccess || (e = hipEventCreateWithFlags(&ctx->ev_acc, hipEventDisableTiming)) != hipSuccess ||
        ctx->d_work.alloc(ctx, 16) || ctx->d_casts.alloc(ctx, kCastSlots)) {
        g_create_error = "rt3_create: " + (e != hipSuccess ? std::string(hipGetErrorString(e)) : ctx->err);
        delete ctx;
        return nullptr;
    }
    ctx->num_cu = prop.multiProcessorCount;
    return ctx;
}

void rt3_destroy(rt3_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();                                   // (the buffers are freed with the context)
    for (auto& p : ctx->ev) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    if (ctx->ev_begin) (void)hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_end) (void)hipEventDestroy(ctx->ev_end);
    if (ctx->ev_acc) (void)hipEventDestroy(ctx->ev_acc);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* rt3_last_error(const rt3_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rt3_set_sample_storage_cap(rt3_ctx* ctx, uint64_t bytes) {
    if (!ctx) return RT3_E_ARG;
    if (bytes < (1ull << 20)) return fail(ctx, RT3_E_ARG, "sample storage cap must be >= 1 MiB");
    ctx->rad_cap_bytes = bytes;
    return 0;
}

int rt3_debug_force_plain_mode_r(rt3_ctx* ctx, int on) {
    if (!ctx) return RT3_E_ARG;
    ctx->force_plain_mode_r = on != 0;
    return 0;
}

int rt3_debug_force_brute(rt3_ctx* ctx, int on) {
    if (!ctx) return RT3_E_ARG;
    ctx->force_brute = on != 0;
    return 0;
}

int rt3_debug_force_flat_filter(rt3_ctx* ctx, int on) {
    if (!ctx) return RT3_E_ARG;
    ctx->force_flat = on != 0;
    return 0;
}

void* rt3_stream(rt3_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int rt3_synchronize(rt3_ctx* ctx) {
    if (!ctx) return RT3_E_ARG;
    RT3_HIP(hipSetDevice(ctx->device));
    RT3_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->update_error_pending) {                                // rt3_update_mesh_device with faces: a face index out of range is reported here, once
        ctx->update_error_pending = false;
        uint32_t err = 0;
        if (ctx->ev_acc_recorded) RT3_HIP(hipEventSynchronize(ctx->ev_acc));    // (the update may have run on a caller's stream)
        RT3_HIP(hipMemcpy(&err, ctx->d_error, 4, hipMemcpyDeviceToHost));
        if (err) {
            RT3_HIP(hipMemset(ctx->d_error, 0, 4));
            return fail(ctx, RT3_E_ARG, "rt3_update_mesh_device: a face references a vertex out of range (that face cannot be hit)");
        }
    }
    return 0;
}

void* rt3_device_alloc_words(rt3_ctx* ctx, uint64_t n_words) {
    if (!ctx || n_words == 0) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&p, n_words * 4) != hipSuccess) { ctx->err = "rt3_device_alloc_words: hipMalloc failed"; return nullptr; }
    return p;
}
void rt3_device_free(rt3_ctx* ctx, void* d_ptr) {
    if (!ctx || !d_ptr) return;
    (void)hipSetDevice(ctx->device);
    (void)hipFree(d_ptr);
}
int rt3_device_read_words(rt3_ctx* ctx, const void* d_ptr, uint64_t n_words, uint32_t* out) {
    if (!ctx) return RT3_E_ARG;
    if (!d_ptr || !out) return fail(ctx, RT3_E_ARG, "rt3_device_read_words: NULL buffer");
    RT3_HIP(hipSetDevice(ctx->device));
    RT3_HIP(hipMemcpyAsync(out, d_ptr, n_words * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT3_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int rt3_render_device(rt3_ctx* ctx, const rt3_camera* cam, uint32_t width, uint32_t height, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    if (!cam || !d_out) return fail(ctx, RT3_E_ARG, "cam / d_out_pixels is NULL");
    if (width < 2 || height < 2 || (uint64_t)width * height > 0x7FFFFFFFull) return fail(ctx, RT3_E_ARG, "bad frame size");
    hipStream_t stream;
    int rc;
    if ((rc = enter(ctx, stream_, &stream))) return rc;            // (Mode R's buffers are the caller's; the scene's are not: an update may be in flight)
    ctx->rendered = false;                                          // stats are valid again once every launch below has been issued
    ctx->ev_used = 0;
    hipEvent_t a, b;
    if ((rc = take_event_pair(ctx, &a, &b))) return rc;
    const uint32_t npix = width * height;
    // k_mode_r_mfma / k_mode_r_fast need n.o == 0 exactly (camera at the origin, as Camera::update always builds it) and finite rays;
    // any other camera takes the plain brute-force kernel, which reproduces the reference for every input.
    const bool at_origin = cam->origin[0] == 0.0f && cam->origin[1] == 0.0f && cam->origin[2] == 0.0f;
    const bool use_mfma = at_origin && !ctx->force_plain_mode_r && !getenv("RT3_NO_MFMA") && ctx->n_faces > 0;
    if (use_mfma) {
        int per_cu = 0;
        if ((rc = blocks_per_cu(ctx, (const void*)k_mode_r_mfma, kMB, kTiledLdsBytes, &per_cu))) return rc;
        if (per_cu < 1) return fail(ctx, RT3_E_DEVICE, "k_mode_r_mfma does not fit on a CU");
        if (!ctx->d_tri_frag_r) return fail(ctx, RT3_E_STATE, "internal: the committed mesh has no Mode-R fragments");     // (built by rt3_mesh_commit)
    }
    RT3_HIP(hipEventRecord(ctx->ev_begin, stream));
    RT3_HIP(hipEventRecord(a, stream));
    if (use_mfma)
        hipLaunchKernelGGL(k_mode_r_mfma, dim3((npix + kMB - 1) / kMB), dim3(kMB), kTiledLdsBytes, stream,
                           ctx->d_tri, ctx->d_tri_frag_r, ctx->d_tri_mat, ctx->n_faces, cam_dev(cam), width, height, (uint32_t*)d_out,
                           0.5f * ctx->tri_centre[0], 0.5f * ctx->tri_centre[1], 0.5f * ctx->tri_centre[2]);
    else if (at_origin && !ctx->force_plain_mode_r)
        hipLaunchKernelGGL(k_mode_r_fast, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                           ctx->d_tri, ctx->d_tri_bound, ctx->d_tri_mat, ctx->n_faces, cam_dev(cam), width, height, (uint32_t*)d_out);
    else
        hipLaunchKernelGGL(k_mode_r, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                           ctx->d_tri, ctx->d_tri_mat, ctx->n_faces, cam_dev(cam), width, height, (uint32_t*)d_out);
    RT3_HIP(hipGetLastError());
    RT3_HIP(hipEventRecord(b, stream));
    RT3_HIP(hipEventRecord(ctx->ev_end, stream));
    if ((rc = leave(ctx, stream))) return rc;                      // (an update on another stream starts behind this render)
    ctx->last_stream = stream;
    ctx->last_samples = npix;
    ctx->last_was_path = false;
    ctx->rendered = true;
    return 0;
}

int rt3_render(rt3_ctx* ctx, const rt3_camera* cam, uint32_t width, uint32_t height, uint32_t* out_pixels) {
    if (!ctx) return RT3_E_ARG;
    if (!out_pixels) return fail(ctx, RT3_E_ARG, "out_pixels is NULL");
    if (width < 2 || height < 2 || (uint64_t)width * height > 0x7FFFFFFFull) return fail(ctx, RT3_E_ARG, "bad frame size");
    return staged(ctx, { stage_out(out_pixels, (size_t)width * height * 4) },
                  [&](void* const* d) { return rt3_render_device(ctx, cam, width, height, d[0], ctx->stream); });
}

// Samples [s_begin, s_begin + s_count) of B's n_items items (every owned pixel, or the list `active`: DESIGN.md 4.15), at most `per` per batch: the trace, then the sums.
static int trace_and_sum(rt3_ctx* ctx, const TracePlan& P, TraceArgs& B, uint32_t n_items, const uint32_t* active, bool var, uint32_t s_begin,
                         uint32_t s_count, uint32_t per, hipStream_t stream) {
    const dim3 ag((n_items + kBlock - 1) / kBlock), ab(kBlock);
    for (uint32_t s0 = s_begin; s0 < s_begin + s_count; s0 += per) {
        const uint32_t ns = std::min(per, s_begin + s_count - s0);
        B.s0 = s0;
        B.total = n_items * ns;
        const int rc = issue_trace(ctx, B, P, B.total, stream);
        if (rc) return rc;
        if (active) hipLaunchKernelGGL(k_accumulate_list<true>, ag, ab, 0, stream, ctx->d_rad, active, n_items, ctx->d_accum, ctx->d_accum_sq,
                                       ctx->d_counts, ns, s0 + ns);
        else if (var) hipLaunchKernelGGL(k_accumulate<true>, ag, ab, 0, stream, ctx->d_rad, ctx->d_accum, ctx->d_accum_sq, n_items, ns, s0 == 0 ? 1 : 0);
        else hipLaunchKernelGGL(k_accumulate<false>, ag, ab, 0, stream, ctx->d_rad, ctx->d_accum, (float4*)nullptr, n_items, ns, s0 == 0 ? 1 : 0);
        RT3_HIP(hipGetLastError());
    }
    return 0;
}

int rt3_render_path_range_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count,
                                 void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    if (!cam || !d_out) return fail(ctx, RT3_E_ARG, "cam / d_out_pixels is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if ((rc = check_light_sampling(ctx, p->flags))) return rc;     // (the flag's own answers come before every older refusal)
    if (sample_count == 0 || (uint64_t)sample_begin + sample_count > p->spp) return fail(ctx, RT3_E_ARG, "sample range outside [0, spp)");
    if ((rc = check_scene(ctx))) return rc;
    const bool ref = (p->flags & RT3_FLAG_REFERENCE_PRIMARY) != 0, var = (p->flags & RT3_FLAG_VARIANCE) != 0;
    if ((rc = check_env_sampling(ctx, p->flags))) return rc;       // (before the older refusals of RT3_FLAG_REFERENCE_PRIMARY: the flag's own answer comes first)
    if (ref && ctx->n_sph != 0) return fail(ctx, RT3_E_ARG, "RT3_FLAG_REFERENCE_PRIMARY needs a triangle-only scene");
    if (ref && ctx->env_n != 0)
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_REFERENCE_PRIMARY is not available while an environment map is set (its primary direction is not a unit vector)");
    if ((rc = check_textures(ctx, p->flags))) return rc;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;

    const uint32_t npix = rt3_rows_owned(p) * p->width;
    if (sample_begin != 0) {                                        // a continuation: of this very accumulation?
        if (ctx->acc_valid && ctx->acc_adaptive)
            return fail(ctx, RT3_E_STATE, "the accumulation held by this context is an adaptive one: it cannot be continued (start with sample_begin = 0)");
        if (!ctx->acc_valid || ctx->acc_done != sample_begin || ctx->acc_npix != npix || !same_bytes(&ctx->acc_params, p, sizeof *p) ||
            !same_bytes(&ctx->acc_cam, cam, sizeof *cam))
            return fail(ctx, RT3_E_STATE, "sample_begin does not continue the accumulation held by this context (same camera, params and "
                                          "samples done are required; start with sample_begin = 0 or rt3_accum_upload)");
    }
    ctx->rendered = false;                                          // stats: valid again once every launch below has been issued
    ctx->acc_valid = false;                                         // accumulation: valid again once this call has been issued completely
    ctx->acc_adaptive = false;
    if (npix == 0) {
        if ((rc = begin_timed(ctx, stream)) || (rc = end_timed(ctx, stream, 0, nullptr))) return rc;
        commit_accumulation(ctx, cam, p, sample_begin + sample_count, 0, false);
        return 0;
    }
    const uint32_t batch = sample_batch(ctx, sample_count, npix, sizeof(Rgb));      // 12 B per (pixel, sample)
    if (batch == 0) return fail(ctx, RT3_E_ARG, "frame too large for one sample batch");
    if ((rc = ctx->d_rad.ensure(ctx, (size_t)npix * batch))) return rc;
    if (sample_begin == 0) {
        if ((rc = ctx->d_accum.ensure(ctx, npix))) return rc;
        if (var && (rc = ctx->d_accum_sq.ensure(ctx, npix))) return rc;
    }

    TraceArgs A;
    if ((rc = path_args(ctx, cam, p, npix, A))) return rc;
    A.rad = ctx->d_rad;
    TracePlan T;
    if ((rc = plan_sampled_trace(ctx, A, ref ? Form::RenderRef : Form::Render, ref && !(cam_at_origin(cam) && !(p->lens_radius > 0.0f)), p->flags, stream, T)))
        return rc;
    if ((rc = begin_timed(ctx, stream))) return rc;
#ifdef RT3_PROFILE
    RT3_HIP(hipMemsetAsync(ctx->d_casts + 6, 0xFF, 8, stream));
    RT3_HIP(hipMemsetAsync(ctx->d_casts + 8, 0xFF, 16, stream));       // [8] first wave start, [9] first time a wave found the queue empty
#endif
    if (T.list_groups) {                                            // camera, params and scene may all have changed since the last call: built every time
        launch_primary_lists(ctx, A, T.list_groups, T.mfma_blocks, stream);
        RT3_HIP(hipGetLastError());
    }
    if ((rc = trace_and_sum(ctx, T, A, npix, nullptr, var, sample_begin, sample_count, batch, stream))) return rc;
    hipLaunchKernelGGL(k_resolve, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                       ctx->d_accum, npix, sample_begin + sample_count, p->flags, (uint32_t*)d_out);
    RT3_HIP(hipGetLastError());
    if ((rc = end_timed(ctx, stream, (uint64_t)npix * sample_count, &T))) return rc;
    commit_accumulation(ctx, cam, p, sample_begin + sample_count, npix, false);
    return 0;
}

int rt3_render_path_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, void* d_out, void* stream) {
    if (!ctx) return RT3_E_ARG;
    if (!p) return fail(ctx, RT3_E_ARG, "params is NULL");
    return rt3_render_path_range_device(ctx, cam, p, 0, p->spp, d_out, stream);
}

int rt3_render_path_range(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, uint32_t* out_pixels) {
    if (!ctx) return RT3_E_ARG;
    if (!out_pixels) return fail(ctx, RT3_E_ARG, "out_pixels is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    return staged(ctx, { stage_out(out_pixels, (size_t)rt3_rows_owned(p) * p->width * 4) },
                  [&](void* const* d) { return rt3_render_path_range_device(ctx, cam, p, sample_begin, sample_count, d[0], ctx->stream); });
}

int rt3_render_path(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t* out_pixels) {
    if (!ctx) return RT3_E_ARG;
    if (!p) return fail(ctx, RT3_E_ARG, "params is NULL");
    return rt3_render_path_range(ctx, cam, p, 0, p->spp, out_pixels);
}

// Adaptive sampling: round 0 is the dense launch of rt3_render_path_range_device over samples [0, min_spp); every later round
// traces the next samples of the pixels on the active list (the trace kernels' list form: TraceArgs::active), adds them with k_accumulate_list,
// applies the rule and compacts the pixels that stay.  The host reads one word per round, the length of the new list.
static_assert(sizeof(rt3_adaptive_params) == 16, "rt3.h: rt3_adaptive_params");
int rt3_render_path_adaptive_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, const rt3_adaptive_params* ap, void* d_out,
                                    void* d_out_counts, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    if (!cam || !ap || !d_out) return fail(ctx, RT3_E_ARG, "cam / adaptive params / d_out_pixels is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (p->flags & RT3_FLAG_LIGHT_SAMPLING)
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_LIGHT_SAMPLING is not available to the adaptive render (the light sampling forms have no list form)");
    if (p->flags & RT3_FLAG_REFERENCE_PRIMARY) return fail(ctx, RT3_E_ARG, "RT3_FLAG_REFERENCE_PRIMARY is not available to the adaptive render");
    if (p->flags & RT3_FLAG_ENV_SAMPLING) return fail(ctx, RT3_E_ARG, "RT3_FLAG_ENV_SAMPLING is not available to the adaptive render (the sampling forms have no list form)");
    if (ap->min_spp < 2 || ap->min_spp > p->spp) return fail(ctx, RT3_E_ARG, "min_spp must lie in [2, spp]");
    if (ap->step_spp < 1) return fail(ctx, RT3_E_ARG, "step_spp must be >= 1");
    if (!(ap->threshold > 0.0f) || !(ap->threshold < __builtin_inff())) return fail(ctx, RT3_E_ARG, "threshold must be finite and > 0");
    if (!(ap->dark >= 0.0f) || !(ap->dark < __builtin_inff())) return fail(ctx, RT3_E_ARG, "dark must be finite and >= 0");
    if ((uintptr_t)d_out % 16u != 0) return fail(ctx, RT3_E_ARG, "d_out_pixels must be 16-byte aligned");
    if ((uintptr_t)d_out_counts % 4u != 0) return fail(ctx, RT3_E_ARG, "d_out_counts must be 4-byte aligned");
    if ((rc = check_scene(ctx)) || (rc = check_textures(ctx, p->flags))) return rc;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;

    const uint32_t rows = rt3_rows_owned(p);
    const uint32_t npix = rows * p->width;
    ctx->rendered = false;
    ctx->acc_valid = false;
    ctx->acc_adaptive = false;
    if (npix == 0) {
        if ((rc = begin_timed(ctx, stream)) || (rc = end_timed(ctx, stream, 0, nullptr))) return rc;
        commit_accumulation(ctx, cam, p, p->spp, 0, true);
        return 0;
    }

    // sample storage: sized once, for the dense round or the longest later round over every pixel; a list round takes as many samples per batch
    // as fit in it (n_active in the place of npix)
    const uint32_t batch = sample_batch(ctx, std::max(ap->min_spp, std::min(ap->step_spp, p->spp)), npix, sizeof(Rgb));
    if (batch == 0) return fail(ctx, RT3_E_ARG, "frame too large for one sample batch");
    const size_t rad_items = (size_t)npix * batch;
    const uint32_t n_blocks = (npix + kBlock - 1) / kBlock;
    if ((rc = ctx->d_rad.ensure(ctx, rad_items)) || (rc = ctx->d_accum.ensure(ctx, npix)) || (rc = ctx->d_accum_sq.ensure(ctx, npix)) ||
        (rc = ctx->d_counts.ensure(ctx, npix)) || (rc = ctx->d_active[0].ensure(ctx, npix)) || (rc = ctx->d_active[1].ensure(ctx, npix)) ||
        (rc = ctx->d_unconverged.ensure(ctx, npix)) || (rc = ctx->d_block_counts.ensure(ctx, (size_t)n_blocks + 1)))
        return rc;
    uint32_t* const d_n_active = ctx->d_block_counts.get() + n_blocks;

    TraceArgs A;
    if ((rc = path_args(ctx, cam, p, npix, A))) return rc;
    A.rad = ctx->d_rad;
    TracePlan T, TL;                                                // the dense launch of round 0, the list form of the same kernel for the later rounds
    if ((rc = plan_trace(ctx, A, Form::Render, false, T))) return rc;
    TraceArgs AL = A;
    if ((rc = plan_trace(ctx, AL, Form::List, false, TL))) return rc;
    AdaptiveGeom G{ p->width, rows, p->tile_rows, p->tile_index, p->tile_count, A.div_width, A.div_tile_rows };

    if ((rc = begin_timed(ctx, stream))) return rc;
    if (T.list_groups) {
        launch_primary_lists(ctx, A, T.list_groups, T.mfma_blocks, stream);
        RT3_HIP(hipGetLastError());
    }
    if ((rc = trace_and_sum(ctx, T, A, npix, nullptr, true, 0, ap->min_spp, batch, stream))) return rc;
    hipLaunchKernelGGL(k_fill_words, dim3(n_blocks), dim3(kBlock), 0, stream, ctx->d_counts, npix, ap->min_spp);
    RT3_HIP(hipGetLastError());

    uint64_t samples = (uint64_t)npix * ap->min_spp;
    uint32_t done = ap->min_spp, cur = 0;
    while (done < p->spp) {
        // who stays active after the round that ended at `done`: the rule, then the ordered compaction into the other list
        hipLaunchKernelGGL(k_adaptive_flags, dim3(n_blocks), dim3(kBlock), 0, stream, (const float4*)ctx->d_accum, (const float4*)ctx->d_accum_sq,
                           (const uint32_t*)ctx->d_counts, npix, ap->threshold, ap->dark, ctx->d_unconverged.get());
        hipLaunchKernelGGL(k_adaptive_count, dim3(n_blocks), dim3(kBlock), 0, stream, G, (const uint32_t*)ctx->d_counts,
                           (const uint8_t*)ctx->d_unconverged, npix, done, ctx->d_block_counts.get());
        hipLaunchKernelGGL(k_adaptive_select, dim3(n_blocks), dim3(kBlock), 0, stream, G, (const uint32_t*)ctx->d_counts,
                           (const uint8_t*)ctx->d_unconverged, npix, done, (const uint32_t*)ctx->d_block_counts, ctx->d_active[cur].get(), d_n_active);
        RT3_HIP(hipGetLastError());
        uint32_t n_active = 0;
        RT3_HIP(hipMemcpyAsync(&n_active, d_n_active, 4, hipMemcpyDeviceToHost, stream));
        RT3_HIP(hipStreamSynchronize(stream));
        if (n_active == 0) break;
        if (n_active > npix) return fail(ctx, RT3_E_DEVICE, "internal: the active list is longer than the frame");
        TraceArgs B = AL;
        B.active = ctx->d_active[cur];
        B.npix = n_active;
        B.div_npix = make_fastdiv(n_active);
        if (!fastdiv_ok(n_active, 0x7FFFFFFFu)) return fail(ctx, RT3_E_DEVICE, "internal: magic-number division self-check failed");
        const uint32_t ns = std::min(ap->step_spp, p->spp - done);
        const uint32_t per = (uint32_t)std::min<uint64_t>(rad_items / n_active, 0x7FFF0000ull / n_active);      // the list's samples per batch of the storage
        if ((rc = trace_and_sum(ctx, TL, B, n_active, ctx->d_active[cur], true, done, ns, per, stream))) return rc;
        samples += (uint64_t)n_active * ns;
        done += ns;
        cur ^= 1u;
    }
    hipLaunchKernelGGL(k_resolve_counts, dim3(n_blocks), dim3(kBlock), 0, stream, (const float4*)ctx->d_accum, (const uint32_t*)ctx->d_counts, npix,
                       p->flags, (uint32_t*)d_out);
    RT3_HIP(hipGetLastError());
    if (d_out_counts) RT3_HIP(hipMemcpyAsync(d_out_counts, ctx->d_counts, (size_t)npix * 4, hipMemcpyDeviceToDevice, stream));
    if ((rc = end_timed(ctx, stream, samples, &T))) return rc;
    commit_accumulation(ctx, cam, p, p->spp, npix, true);
    return 0;
}

int rt3_render_path_adaptive(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, const rt3_adaptive_params* ap, uint32_t* out_pixels,
                             uint32_t* out_counts) {
    if (!ctx) return RT3_E_ARG;
    if (!out_pixels) return fail(ctx, RT3_E_ARG, "out_pixels is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    const size_t bytes = (size_t)rt3_rows_owned(p) * p->width * 4;
    return staged(ctx, { stage_out(out_pixels, bytes), stage_out(out_counts, bytes) },
                  [&](void* const* d) { return rt3_render_path_adaptive_device(ctx, cam, p, ap, d[0], d[1], ctx->stream); });      // (no counts asked for: a NULL d_out_counts)
}

// Checkpoint of the accumulation: what rt3_render_path_range keeps between calls, 4 floats per owned pixel.
int rt3_accum_download(rt3_ctx* ctx, float* sum, float* sum_sq, uint32_t* samples_done) {
    if (!ctx) return RT3_E_ARG;
    if (!ctx->acc_valid) return fail(ctx, RT3_E_STATE, "no accumulation on this context");
    if (ctx->acc_adaptive) return fail(ctx, RT3_E_STATE, "the accumulation is an adaptive one (per-pixel sample counts): it has no checkpoint form");
    RT3_HIP(hipSetDevice(ctx->device));
    if (ctx->ev_acc_recorded) RT3_HIP(hipEventSynchronize(ctx->ev_acc));        // the render may have run on a caller's stream (which may be gone by now)
    const size_t bytes = (size_t)ctx->acc_npix * sizeof(float4);
    if (sum && bytes) RT3_HIP(hipMemcpy(sum, ctx->d_accum, bytes, hipMemcpyDeviceToHost));
    if (sum_sq) {
        if (!(ctx->acc_params.flags & RT3_FLAG_VARIANCE)) return fail(ctx, RT3_E_STATE, "the accumulation was not started with RT3_FLAG_VARIANCE");
        if (bytes) RT3_HIP(hipMemcpy(sum_sq, ctx->d_accum_sq, bytes, hipMemcpyDeviceToHost));
    }
    if (samples_done) *samples_done = ctx->acc_done;
    return 0;
}

int rt3_accum_upload(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, const float* sum, const float* sum_sq, uint32_t samples_done) {
    if (!ctx) return RT3_E_ARG;
    if (!cam || !sum) return fail(ctx, RT3_E_ARG, "cam / sum_rgba is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (samples_done == 0 || samples_done > p->spp) return fail(ctx, RT3_E_ARG, "samples_done outside (0, spp]");
    const bool var = (p->flags & RT3_FLAG_VARIANCE) != 0;
    if (var && !sum_sq) return fail(ctx, RT3_E_ARG, "params ask for RT3_FLAG_VARIANCE: sum_sq_rgba is required");
    RT3_HIP(hipSetDevice(ctx->device));
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    ctx->acc_valid = false;
    ctx->acc_adaptive = false;
    if (ctx->ev_acc_recorded) RT3_HIP(hipEventSynchronize(ctx->ev_acc));        // a render still in flight reads and writes what is overwritten here
    if (npix) {
        if ((rc = ctx->d_accum.ensure(ctx, npix))) return rc;
        RT3_HIP(hipMemcpy(ctx->d_accum, sum, (size_t)npix * sizeof(float4), hipMemcpyHostToDevice));
        if (var) {
            if ((rc = ctx->d_accum_sq.ensure(ctx, npix))) return rc;
            RT3_HIP(hipMemcpy(ctx->d_accum_sq, sum_sq, (size_t)npix * sizeof(float4), hipMemcpyHostToDevice));
        }
    }
    commit_accumulation(ctx, cam, p, samples_done, npix, false);
    return 0;
}

// The copies of rt3_gather_rows as plain arithmetic (no device): row block lb of the shard (tile_rows rows, compact in the tile) is row block
// lb * tile_count + tile_index of the frame — one 2-D copy whose "rows" are whole row blocks, with the tile's block size as the source pitch and
// tile_count times that as the destination pitch; only the frame's very last row block can be ragged, and it then travels as one more 1-D copy.
int rt3_gather_plan(const rt3_params* p, rt3_gather_copy out[2]) {
    if (!p || !out || p->width == 0 || p->height == 0) return RT3_E_ARG;
    if (p->tile_count > 1 && (p->tile_rows == 0 || p->tile_index >= p->tile_count)) return RT3_E_ARG;
    const uint64_t row_bytes = (uint64_t)p->width * 4;
    if (p->tile_count <= 1) {
        out[0] = rt3_gather_copy{ 0, 0, row_bytes * p->height, row_bytes * p->height, row_bytes * p->height, 1 };
        return 1;
    }
    const uint32_t n_blocks_frame = (p->height + p->tile_rows - 1) / p->tile_rows;
    if (p->tile_index >= n_blocks_frame) return 0;                                  // more shards than row blocks: this one owns nothing
    const uint32_t my_blocks = (n_blocks_frame - 1 - p->tile_index) / p->tile_count + 1;
    const uint32_t last_block = (my_blocks - 1) * p->tile_count + p->tile_index;    // frame index of this shard's last block
    const uint32_t last_rows = std::min(p->tile_rows, p->height - last_block * p->tile_rows);
    const uint32_t full = last_rows == p->tile_rows ? my_blocks : my_blocks - 1;
    const uint64_t block_bytes = row_bytes * p->tile_rows;
    int n = 0;
    if (full) out[n++] = rt3_gather_copy{ (uint64_t)p->tile_index * block_bytes, 0, block_bytes * p->tile_count, block_bytes, block_bytes, full };
    if (full != my_blocks) out[n++] = rt3_gather_copy{ (uint64_t)last_block * block_bytes, (uint64_t)full * block_bytes, row_bytes * last_rows, row_bytes * last_rows,
                                                       row_bytes * last_rows, 1 };
    return n;
}

// The gather of final pixels, device to device.  Row block lb of the shard (tile_rows rows, compact in d_tile)
// is row block lb * tile_count + tile_index of the frame: one 2-D copy with the tile's pitch on one side and tile_count times that on
// the other; only the frame's very last row block can be ragged, and it then travels as one more 1-D copy.
int rt3_gather_rows(rt3_ctx* root, void* d_frame, rt3_ctx* shard, const void* d_tile, const rt3_params* p, void* stream_) {
    if (!root || !shard) return RT3_E_ARG;
    rt3_ctx* ctx = shard;
    if (!d_frame || !d_tile) return fail(ctx, RT3_E_ARG, "rt3_gather_rows: NULL buffer");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    RT3_HIP(hipSetDevice(shard->device));
    const hipStream_t stream = stream_of(shard, stream_);           // (d_frame and d_tile are the caller's: no wait for ev_acc)
    if (root->device != shard->device && !shard->peers_enabled.count(root->device)) {
        int can = 0;
        RT3_HIP(hipDeviceCanAccessPeer(&can, shard->device, root->device));
        if (!can) return fail(ctx, RT3_E_DEVICE, "rt3_gather_rows: no peer access from device " + std::to_string(shard->device) + " to " + std::to_string(root->device));
        const hipError_t e = hipDeviceEnablePeerAccess(root->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { ctx->err = std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e); return RT3_E_DEVICE; }
        (void)hipGetLastError();
        shard->peers_enabled.insert(root->device);
    }
    rt3_gather_copy plan[2];
    const int n_copies = rt3_gather_plan(p, plan);
    if (n_copies < 0) return fail(ctx, RT3_E_ARG, "rt3_gather_rows: bad shard parameters");
    uint8_t* frame = (uint8_t*)d_frame;
    const uint8_t* tile = (const uint8_t*)d_tile;
    for (int i = 0; i < n_copies; i++) {
        const rt3_gather_copy& c = plan[i];
        if (c.rows == 1) RT3_HIP(hipMemcpyAsync(frame + c.dst_offset, tile + c.src_offset, c.row_bytes, hipMemcpyDeviceToDevice, stream));
        else RT3_HIP(hipMemcpy2DAsync(frame + c.dst_offset, c.dst_pitch, tile + c.src_offset, c.src_pitch, c.row_bytes, c.rows, hipMemcpyDeviceToDevice, stream));
    }
    return 0;
}

// Batched ray queries: the query form of the kernel Mode X would take for the scene, one launch, one item per ray.
static int query_device(rt3_ctx* ctx, const void* d_rays, uint32_t n, float t_min, void* d_out, void* stream_, bool occluded) {
    if (!ctx) return RT3_E_ARG;
    if (!(t_min >= 0.0f) || !(t_min < __builtin_inff())) return fail(ctx, RT3_E_ARG, "t_min must be finite and >= 0");
    if (n > (1u << 30)) return fail(ctx, RT3_E_ARG, "at most 2^30 rays per query");
    if (n == 0) return 0;
    if (!d_rays || !d_out) return fail(ctx, RT3_E_ARG, "rays / results buffer is NULL");
    if ((uintptr_t)d_rays % 16u != 0 || (uintptr_t)d_out % (occluded ? 4u : 16u) != 0)
        return fail(ctx, RT3_E_ARG, occluded ? "rays must be 16-byte and occlusion words 4-byte aligned" : "rays and hits must be 16-byte aligned");
    int rc = check_scene(ctx);
    if (rc) return rc;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    ctx->rendered = false;
    TraceArgs A = scene_args(ctx);
    A.t_min = t_min;
    A.total = n;
    A.q_rays = (const float4*)d_rays; A.q_out = d_out; A.q_occluded = occluded ? 1u : 0u;
    TracePlan T;
    if ((rc = plan_trace(ctx, A, Form::Query, false, T)) || (rc = begin_timed(ctx, stream)) || (rc = issue_trace(ctx, A, T, n, stream))) return rc;
    return end_timed(ctx, stream, 0, &T);
}
static int query_host(rt3_ctx* ctx, const rt3_ray* rays, uint32_t n, float t_min, void* out, bool occluded) {
    if (!ctx) return RT3_E_ARG;
    if (!(t_min >= 0.0f) || !(t_min < __builtin_inff())) return fail(ctx, RT3_E_ARG, "t_min must be finite and >= 0");
    if (n > (1u << 30)) return fail(ctx, RT3_E_ARG, "at most 2^30 rays per query");
    if (n == 0) return 0;
    if (!rays || !out) return fail(ctx, RT3_E_ARG, "rays / results array is NULL");
    int rc = check_scene(ctx);
    if (rc) return rc;
    return staged(ctx, { stage_in(rays, (size_t)n * sizeof(rt3_ray)), stage_out(out, (size_t)n * (occluded ? 4u : sizeof(rt3_hit))) },
                  [&](void* const* d) { return query_device(ctx, d[0], n, t_min, d[1], ctx->stream, occluded); });
}
static_assert(sizeof(rt3_ray) == 32 && sizeof(rt3_hit) == 16, "rt3.h: query wire structs");

int rt3_intersect(rt3_ctx* ctx, const rt3_ray* rays, uint32_t n, float t_min, rt3_hit* hits) { return query_host(ctx, rays, n, t_min, hits, false); }
int rt3_occluded(rt3_ctx* ctx, const rt3_ray* rays, uint32_t n, float t_min, uint32_t* out) { return query_host(ctx, rays, n, t_min, out, true); }
int rt3_intersect_device(rt3_ctx* ctx, const void* d_rays, uint32_t n, float t_min, void* d_hits, void* stream) {
    return query_device(ctx, d_rays, n, t_min, d_hits, stream, false);
}
int rt3_occluded_device(rt3_ctx* ctx, const void* d_rays, uint32_t n, float t_min, void* d_out, void* stream) {
    return query_device(ctx, d_rays, n, t_min, d_out, stream, true);
}

// ---- Camera rays, first-hit AOVs and the linear resolve
static int aov_common_checks(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, const void* d_out, const char* what) {
    if (!cam || !d_out) return fail(ctx, RT3_E_ARG, std::string("cam / ") + what + " is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (p->flags & RT3_FLAG_REFERENCE_PRIMARY)
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_REFERENCE_PRIMARY: its primary directions are not unit vectors, which the query engine needs");
    if ((uintptr_t)d_out % 16u != 0) return fail(ctx, RT3_E_ARG, std::string(what) + " must be 16-byte aligned");
    return 0;
}

int rt3_camera_rays_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = aov_common_checks(ctx, cam, p, d_out, "rays");
    if (rc) return rc;
    if (sample_count == 0 || (uint64_t)sample_begin + sample_count > p->spp) return fail(ctx, RT3_E_ARG, "sample range outside [0, spp)");
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    if ((uint64_t)npix * sample_count > 0x7FFF0000ull) return fail(ctx, RT3_E_ARG, "too many rays for one call (owned pixels x samples > 2^31 - 2^16)");
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    if (npix != 0) {
        TraceArgs A;
        if ((rc = path_args(ctx, cam, p, npix, A))) return rc;
        A.s0 = sample_begin;
        A.total = npix * sample_count;
        hipLaunchKernelGGL(k_camera_rays, dim3((A.total + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, A, (float4*)d_out);
        RT3_HIP(hipGetLastError());
    }
    return leave(ctx, stream);
}

int rt3_camera_rays(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, rt3_ray* out) {
    if (!ctx) return RT3_E_ARG;
    if (!out) return fail(ctx, RT3_E_ARG, "out_rays is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (sample_count == 0 || (uint64_t)sample_begin + sample_count > p->spp) return fail(ctx, RT3_E_ARG, "sample range outside [0, spp)");
    const uint64_t n = (uint64_t)rt3_rows_owned(p) * p->width * sample_count;
    if (n > 0x7FFF0000ull) return fail(ctx, RT3_E_ARG, "too many rays for one call (owned pixels x samples > 2^31 - 2^16)");
    return staged(ctx, { stage_out(out, n * sizeof(rt3_ray)) },
                  [&](void* const* d) { return rt3_camera_rays_device(ctx, cam, p, sample_begin, sample_count, d[0], ctx->stream); });
}

// Per sample batch: the batch's rays (make_rays(s0, ns): k_camera_rays, or k_lens_rays for a lens frame) into d_arays -> the query form of the scene's
// trace kernel on that buffer -> k_aov_accumulate; then one k_aov_resolve.  The batches share one ev_begin / ev_end and one counter reset, as the
// render's batch loop does.  A: what k_aov_accumulate reads — the scene's records and the flags.  The caller has checked its arguments and the scene
// and is behind enter().
// chain (rt3_render_aov_specular*): each ray is followed through mirrors and glass.  Per batch at most max_bounces + 1 rounds of
// query -> k_aov_bounce on the same ray buffer (a finished chain's ray is INVALID to the query and costs no trace), the primary hits in d_ahits and
// every later round's in d_chits; then k_aov_accumulate_chain.  After each round the host reads one word, the chains still running, and leaves the
// loop at 0 (the adaptive render's precedent; RT3_AOV_CHAIN_NO_WAIT=1 queues every round without waiting — the A/B of DESIGN.md 5.2v).
static int aov_pass(rt3_ctx* ctx, const rt3_params* p, const TraceArgs& A, void* d_out, hipStream_t stream,
                    const std::function<int(uint32_t, uint32_t)>& make_rays, const rt3_aov_chain_params* chain = nullptr) {
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    ctx->rendered = false;
    int rc;
    if (npix == 0) return (rc = begin_timed(ctx, stream)) ? rc : end_timed(ctx, stream, 0, nullptr);
    // 48 B per (pixel, sample): the ray and its hit; a chain adds 48: the bounce queries' hit, the state, the normal
    const uint32_t batch = sample_batch(ctx, p->spp, npix, sizeof(rt3_ray) + sizeof(rt3_hit) + (chain ? sizeof(rt3_hit) + 2 * sizeof(float4) : 0));
    if (batch == 0) return fail(ctx, RT3_E_ARG, "frame too large for one sample batch");
    if ((rc = ctx->d_arays.ensure(ctx, (size_t)npix * batch * 2u)) || (rc = ctx->d_ahits.ensure(ctx, (size_t)npix * batch)) ||
        (rc = ctx->d_aacc.ensure(ctx, (size_t)npix * 3u)))
        return rc;
    if (chain && ((rc = ctx->d_chits.ensure(ctx, (size_t)npix * batch)) || (rc = ctx->d_cstate.ensure(ctx, (size_t)npix * batch)) ||
                  (rc = ctx->d_cnorm.ensure(ctx, (size_t)npix * batch)) || (rc = ctx->d_calive.ensure(ctx, 1))))
        return rc;
    const char* no_wait = getenv("RT3_AOV_CHAIN_NO_WAIT");
    const bool wait = !(no_wait && no_wait[0] == '1');
    TraceArgs Q = scene_args(ctx);                                  // the query launches, as query_device sets them up
    Q.t_min = p->t_min;
    Q.q_rays = ctx->d_arays; Q.q_out = ctx->d_ahits; Q.q_occluded = 0u;
    TracePlan T;
    if ((rc = plan_trace(ctx, Q, Form::Query, false, T)) || (rc = begin_timed(ctx, stream))) return rc;
    for (uint32_t s0 = 0; s0 < p->spp; s0 += batch) {
        const uint32_t ns = std::min(batch, p->spp - s0);
        Q.total = npix * ns;
        if ((rc = make_rays(s0, ns))) return rc;
        if (chain) {
            TraceArgs B = A;                                        // the bounce kernel: the scene's records, the flags and the batch's item count
            B.total = Q.total;
            const dim3 bg((Q.total + kBlock - 1) / kBlock), bb(kBlock);
            for (uint32_t b = 0; b <= chain->max_bounces; b++) {
                Q.q_out = b ? ctx->d_chits.get() : ctx->d_ahits.get();
                if ((rc = issue_trace(ctx, Q, T, Q.total, stream))) return rc;
                const bool count = wait && b < chain->max_bounces;  // (the last round ends every chain)
                if (count) {
                    RT3_HIP(hipMemsetAsync(ctx->d_calive, 0, 4, stream));
                    hipLaunchKernelGGL(k_aov_bounce<true>, bg, bb, 0, stream, B, ctx->d_arays.get(), (const uint4*)Q.q_out, ctx->d_cstate.get(),
                                       ctx->d_cnorm.get(), b, chain->max_bounces, chain->max_fuzz, (const float4*)ctx->d_env, ctx->env_n,
                                       tex_table(ctx), ctx->d_calive.get());
                } else {
                    hipLaunchKernelGGL(k_aov_bounce<false>, bg, bb, 0, stream, B, ctx->d_arays.get(), (const uint4*)Q.q_out, ctx->d_cstate.get(),
                                       ctx->d_cnorm.get(), b, chain->max_bounces, chain->max_fuzz, (const float4*)ctx->d_env, ctx->env_n,
                                       tex_table(ctx), (uint32_t*)nullptr);
                }
                RT3_HIP(hipGetLastError());
                if (count) {
                    uint32_t n_alive = 0;
                    RT3_HIP(hipMemcpyAsync(&n_alive, ctx->d_calive.get(), 4, hipMemcpyDeviceToHost, stream));
                    RT3_HIP(hipStreamSynchronize(stream));
                    if (n_alive == 0) break;
                }
            }
            hipLaunchKernelGGL(k_aov_accumulate_chain, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, (const uint4*)ctx->d_ahits,
                               (const float4*)ctx->d_cstate, (const float4*)ctx->d_cnorm, ctx->d_aacc.get(), npix, ns, s0 == 0 ? 1 : 0);
            RT3_HIP(hipGetLastError());
            continue;
        }
        if ((rc = issue_trace(ctx, Q, T, Q.total, stream))) return rc;
        hipLaunchKernelGGL(k_aov_accumulate, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, A, (const float4*)ctx->d_arays,
                           (const uint4*)ctx->d_ahits, ctx->d_aacc, npix, ns, s0 == 0 ? 1 : 0, (const float4*)ctx->d_env, ctx->env_n, tex_table(ctx));
        RT3_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_aov_resolve, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, (const float4*)ctx->d_aacc, npix, p->spp, (float4*)d_out);
    RT3_HIP(hipGetLastError());
    return end_timed(ctx, stream, (uint64_t)npix * p->spp, &T);
}

// The Rays form over n rays: samples [rp.sample_begin, rp.sample_begin + rp.sample_count) in batches under the sample storage cap;
// per batch the trace, then k_accumulate<false> into d_out in sample order (d_accum and the acc_* state are never touched), and the division in place.
// d_rays: the caller's rays, one launch per batch over the items (sample in batch, ray).  Without them every sample has rays of its own: make_rays(s0, ns)
// writes a batch's into d_arays and, the Rays form mapping item j to ray j % n, each sample is a launch over its slice of the rays and of the storage.
// d_keys: the rays' keys or nullptr.  Called behind the arguments' checks and enter().
static int radiance_pass(rt3_ctx* ctx, uint32_t n, const rt3_radiance_params& rp, void* d_out, const uint32_t* d_keys, const float4* d_rays,
                         hipStream_t stream, const std::function<int(uint32_t, uint32_t)>& make_rays) {
    const bool per_sample = d_rays == nullptr;
    ctx->rendered = false;
    int rc;
    if (n == 0) return (rc = begin_timed(ctx, stream)) ? rc : end_timed(ctx, stream, 0, nullptr);
    // 12 B per (ray, sample) of radiance and, for rays made here, the ray's 32 (n <= 2^27: at least 15 samples fit the item index)
    const uint32_t batch = sample_batch(ctx, rp.sample_count, n, sizeof(Rgb) + (per_sample ? sizeof(rt3_ray) : 0));
    if ((rc = ctx->d_rad.ensure(ctx, (size_t)n * batch)) || (per_sample && (rc = ctx->d_arays.ensure(ctx, (size_t)n * batch * 2u)))) return rc;
    TraceArgs A = scene_args(ctx);
    A.max_depth = rp.max_depth; A.seed = rp.seed; A.flags = rp.flags; A.t_min = rp.t_min;
    A.npix = n; A.div_npix = make_fastdiv(n);
    if (!fastdiv_ok(n, 0x7FFFFFFFu)) return fail(ctx, RT3_E_DEVICE, "internal: magic-number division self-check failed");
    TracePlan T;
    if ((rc = plan_sampled_trace(ctx, A, Form::Rays, false, rp.flags, stream, T))) return rc;
    A.ray_keys = d_keys;
    if ((rc = begin_timed(ctx, stream))) return rc;
    const uint32_t s_end = rp.sample_begin + rp.sample_count;
    const dim3 ag((n + kBlock - 1) / kBlock), ab(kBlock);
    for (uint32_t s0 = rp.sample_begin; s0 < s_end; s0 += batch) {
        const uint32_t ns = std::min(batch, s_end - s0);
        if (per_sample && (rc = make_rays(s0, ns))) return rc;
        const uint32_t launches = per_sample ? ns : 1u, each = ns / launches;      // samples per launch
        for (uint32_t i = 0; i < launches; i++) {
            A.s0 = s0 + i * each;
            A.total = n * each;
            A.q_rays = per_sample ? ctx->d_arays.get() + (size_t)i * n * 2u : d_rays;
            A.rad = ctx->d_rad.get() + (size_t)i * n * each;
            if ((rc = issue_trace(ctx, A, T, A.total, stream))) return rc;
        }
        hipLaunchKernelGGL(k_accumulate<false>, ag, ab, 0, stream, ctx->d_rad, (float4*)d_out, (float4*)nullptr, n, ns, s0 == rp.sample_begin ? 1 : 0);
        RT3_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_resolve_float_inplace, ag, ab, 0, stream, (float4*)d_out, n, rp.sample_count);
    RT3_HIP(hipGetLastError());
    return end_timed(ctx, stream, (uint64_t)n * rp.sample_count, &T);
}

// rt3_render_aov_device (chain == nullptr) and rt3_render_aov_specular_device: the same checks and set-up, the chain's own refusals behind the common ones.
static int render_aov_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, const rt3_aov_chain_params* chain, bool specular, void* d_out,
                             void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = aov_common_checks(ctx, cam, p, d_out, "d_out_aov");
    if (rc) return rc;
    if (specular) if (const char* why = rt3chain::refusal(chain)) return fail(ctx, RT3_E_ARG, std::string("rt3_render_aov_specular: ") + why);
    if ((rc = check_scene(ctx)) || (rc = check_textures(ctx, 0u))) return rc;       // (the AOVs draw no shadow rays: the sampling flags change nothing here)
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    ctx->rendered = false;
    TraceArgs A = scene_args(ctx);                                  // camera rays and the accumulation (a shard that owns no pixel launches neither)
    if (npix != 0 && (rc = path_args(ctx, cam, p, npix, A))) return rc;
    return aov_pass(ctx, p, A, d_out, stream, [&](uint32_t s0, uint32_t ns) {
        A.s0 = s0;
        A.total = npix * ns;
        hipLaunchKernelGGL(k_camera_rays, dim3((A.total + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, A, ctx->d_arays.get());
        RT3_HIP(hipGetLastError());
        return 0;
    }, chain);
}
int rt3_render_aov_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, void* d_out, void* stream) {
    return render_aov_device(ctx, cam, p, nullptr, false, d_out, stream);
}
int rt3_render_aov_specular_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, const rt3_aov_chain_params* chain, void* d_out, void* stream) {
    return render_aov_device(ctx, cam, p, chain, true, d_out, stream);
}

int rt3_render_aov(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, rt3_aov* out) {
    if (!ctx) return RT3_E_ARG;
    if (!out) return fail(ctx, RT3_E_ARG, "out_aov is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    return staged(ctx, { stage_out(out, (size_t)rt3_rows_owned(p) * p->width * sizeof(rt3_aov)) },
                  [&](void* const* d) { return rt3_render_aov_device(ctx, cam, p, d[0], ctx->stream); });
}
int rt3_render_aov_specular(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, const rt3_aov_chain_params* chain, rt3_aov* out) {
    if (!ctx) return RT3_E_ARG;
    if (!out) return fail(ctx, RT3_E_ARG, "out_aov is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (const char* why = rt3chain::refusal(chain)) return fail(ctx, RT3_E_ARG, std::string("rt3_render_aov_specular: ") + why);
    return staged(ctx, { stage_out(out, (size_t)rt3_rows_owned(p) * p->width * sizeof(rt3_aov)) },
                  [&](void* const* d) { return rt3_render_aov_specular_device(ctx, cam, p, chain, d[0], ctx->stream); });
}

int rt3_accum_resolve_device(rt3_ctx* ctx, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    if (!d_out) return fail(ctx, RT3_E_ARG, "d_out_rgba is NULL");
    if ((uintptr_t)d_out % 16u != 0) return fail(ctx, RT3_E_ARG, "d_out_rgba must be 16-byte aligned");
    if (!ctx->acc_valid) return fail(ctx, RT3_E_STATE, "no accumulation on this context");
    hipStream_t stream;
    const int rc = enter(ctx, stream_, &stream);                    // behind the render that wrote d_accum
    if (rc) return rc;
    if (ctx->acc_npix) {
        const dim3 grid((ctx->acc_npix + kBlock - 1) / kBlock);
        if (ctx->acc_adaptive) hipLaunchKernelGGL(k_resolve_float_counts, grid, dim3(kBlock), 0, stream, (const float4*)ctx->d_accum,
                                                  (const uint32_t*)ctx->d_counts, ctx->acc_npix, (float4*)d_out);
        else hipLaunchKernelGGL(k_resolve_float, grid, dim3(kBlock), 0, stream, (const float4*)ctx->d_accum, ctx->acc_npix, ctx->acc_done, (float4*)d_out);
        RT3_HIP(hipGetLastError());
    }
    return leave(ctx, stream);                                      // a later render that overwrites d_accum waits for this
}

int rt3_accum_resolve(rt3_ctx* ctx, float* rgba) {
    if (!ctx) return RT3_E_ARG;
    if (!rgba) return fail(ctx, RT3_E_ARG, "rgba is NULL");
    if (!ctx->acc_valid) return fail(ctx, RT3_E_STATE, "no accumulation on this context");
    return staged(ctx, { stage_out(rgba, (size_t)ctx->acc_npix * sizeof(float4)) },
                  [&](void* const* d) { return rt3_accum_resolve_device(ctx, d[0], ctx->stream); });
}
static_assert(sizeof(rt3_aov) == 48, "rt3.h: rt3_aov");

// ---- Radiance along caller-supplied rays: the rays form of the kernel a query would take on the scene, over the items
// (sample in batch, ray), through radiance_pass with the caller's rays and the caller's output as the sum buffer.
static_assert(sizeof(rt3_radiance_params) == 24, "rt3.h: rt3_radiance_params");
static int radiance_checks(rt3_ctx* ctx, uint32_t n, const rt3_radiance_params* rp) {
    if (!rp) return fail(ctx, RT3_E_ARG, "radiance params is NULL");
    if (!(rp->t_min >= 0.0f) || !(rp->t_min < __builtin_inff())) return fail(ctx, RT3_E_ARG, "t_min must be finite and >= 0");
    int rc_light = check_light_sampling(ctx, rp->flags);           // (the flag's own answers come before every older refusal)
    if (rc_light) return rc_light;
    if (rp->flags & ~(RT3_FLAG_BLACK_BACKGROUND | RT3_FLAG_ENV_SAMPLING | RT3_FLAG_LIGHT_SAMPLING))
        return fail(ctx, RT3_E_ARG, "rt3_radiance: flags may only hold RT3_FLAG_BLACK_BACKGROUND, RT3_FLAG_ENV_SAMPLING or RT3_FLAG_LIGHT_SAMPLING");
    if ((rp->flags & RT3_FLAG_ENV_SAMPLING) && (rp->flags & RT3_FLAG_BLACK_BACKGROUND))
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_ENV_SAMPLING cannot be combined with RT3_FLAG_BLACK_BACKGROUND or RT3_FLAG_REFERENCE_PRIMARY");
    if (rp->max_depth < 1 || rp->sample_count < 1) return fail(ctx, RT3_E_ARG, "max_depth and sample_count must be >= 1");
    if ((uint64_t)rp->sample_begin + rp->sample_count > (1ull << 31)) return fail(ctx, RT3_E_ARG, "sample_begin + sample_count must be <= 2^31");
    if (n > (1u << 27)) return fail(ctx, RT3_E_ARG, "at most 2^27 rays per radiance call (split the batch and pass keys)");
    return 0;
}
int rt3_radiance_device(rt3_ctx* ctx, const void* d_rays, const void* d_keys, uint32_t n, const rt3_radiance_params* rp, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = radiance_checks(ctx, n, rp);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!d_rays || !d_out) return fail(ctx, RT3_E_ARG, "rays / out_rgba buffer is NULL");
    if ((uintptr_t)d_rays % 16u != 0 || (uintptr_t)d_out % 16u != 0 || (uintptr_t)d_keys % 4u != 0)
        return fail(ctx, RT3_E_ARG, "rays and out_rgba must be 16-byte and keys 4-byte aligned");
    if (ranges_overlap(d_out, (size_t)n * 16u, d_rays, (size_t)n * sizeof(rt3_ray)) || (d_keys && ranges_overlap(d_out, (size_t)n * 16u, d_keys, (size_t)n * 4u)))
        return fail(ctx, RT3_E_ARG, "out_rgba overlaps the rays or the keys");
    if ((rc = check_scene(ctx)) || (rc = check_env_sampling(ctx, rp->flags)) || (rc = check_textures(ctx, rp->flags))) return rc;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    return radiance_pass(ctx, n, *rp, d_out, (const uint32_t*)d_keys, (const float4*)d_rays, stream, nullptr);
}
int rt3_radiance(rt3_ctx* ctx, const rt3_ray* rays, const uint32_t* keys, uint32_t n, const rt3_radiance_params* rp, float* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = radiance_checks(ctx, n, rp);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!rays || !out) return fail(ctx, RT3_E_ARG, "rays / out_rgba array is NULL");
    if ((rc = check_scene(ctx))) return rc;
    return staged(ctx, { stage_in(rays, (size_t)n * sizeof(rt3_ray)), stage_in(keys, (size_t)n * 4u), stage_out(out, (size_t)n * 16u) },
                  [&](void* const* d) { return rt3_radiance_device(ctx, d[0], d[1], n, rp, d[2], ctx->stream); });
}

// ---- Lens models: k_lens_rays writes a batch's rays (and a shard's keys) into the context's scratch; a render is
// radiance_pass with k_lens_rays as its ray generator (one trace launch per sample), and the AOVs are aov_pass with k_lens_rays in k_camera_rays' place.
static_assert(sizeof(rt3_lens) == 80, "rt3.h: rt3_lens");
// rt3_params' own rules (check_params) for a frame that may be one pixel wide or high (a cube of N = 1), then the lens.
static int lens_checks(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, const void* d_out, const char* what, bool device) {
    if (!lens || !d_out) return fail(ctx, RT3_E_ARG, std::string("lens / ") + what + " is NULL");
    const int rc = check_params(ctx, p, 1);
    if (rc) return rc;
    if (const char* why = rt3lens::refusal(lens, p->width, p->height)) return fail(ctx, RT3_E_ARG, why);
    if (device && (uintptr_t)d_out % 16u != 0) return fail(ctx, RT3_E_ARG, std::string(what) + " must be 16-byte aligned");
    return 0;
}
// The rays of samples [s0, s0 + ns) of the npix owned pixels -> d_rays (2 * npix * ns float4) and, non-null, the pixels' keys -> d_keys (npix words).
static int launch_lens_rays(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, uint32_t npix, uint32_t s0, uint32_t ns, float4* d_rays,
                            uint32_t* d_keys, hipStream_t stream) {
    LensArgs A;
    A.lens = *lens;
    A.frame = rt3lens::Frame{ p->width, p->height, p->spp, p->seed, rt3lens::edge_of(p->spp) };
    A.tile_rows = p->tile_rows; A.tile_index = p->tile_index; A.tile_count = p->tile_count;
    A.npix = npix; A.s0 = s0; A.total = npix * ns;
    const dim3 grid((A.total + kBlock - 1) / kBlock), block(kBlock);
    switch (lens->model) {
    case RT3_LENS_EQUIRECT: hipLaunchKernelGGL(k_lens_rays<RT3_LENS_EQUIRECT>, grid, block, 0, stream, A, d_rays, d_keys); break;
    case RT3_LENS_FISHEYE:  hipLaunchKernelGGL(k_lens_rays<RT3_LENS_FISHEYE>, grid, block, 0, stream, A, d_rays, d_keys); break;
    case RT3_LENS_ORTHO:    hipLaunchKernelGGL(k_lens_rays<RT3_LENS_ORTHO>, grid, block, 0, stream, A, d_rays, d_keys); break;
    default:                hipLaunchKernelGGL(k_lens_rays<RT3_LENS_CUBE>, grid, block, 0, stream, A, d_rays, d_keys); break;
    }
    RT3_HIP(hipGetLastError());
    return 0;
}
static bool lens_sample_range_ok(const rt3_params* p, uint32_t sample_begin, uint32_t sample_count) {
    return sample_count != 0 && (uint64_t)sample_begin + sample_count <= p->spp;
}

int rt3_lens_rays_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = lens_checks(ctx, lens, p, d_out, "rays", true);
    if (rc) return rc;
    if (!lens_sample_range_ok(p, sample_begin, sample_count)) return fail(ctx, RT3_E_ARG, "sample range outside [0, spp)");
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    if ((uint64_t)npix * sample_count > 0x7FFF0000ull) return fail(ctx, RT3_E_ARG, "too many rays for one call (owned pixels x samples > 2^31 - 2^16)");
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    if (npix != 0 && (rc = launch_lens_rays(ctx, lens, p, npix, sample_begin, sample_count, (float4*)d_out, nullptr, stream))) return rc;
    return leave(ctx, stream);
}

int rt3_lens_rays(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, rt3_ray* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = lens_checks(ctx, lens, p, out, "out_rays", false);
    if (rc) return rc;
    if (!lens_sample_range_ok(p, sample_begin, sample_count)) return fail(ctx, RT3_E_ARG, "sample range outside [0, spp)");
    const uint64_t n = (uint64_t)rt3_rows_owned(p) * p->width * sample_count;
    if (n > 0x7FFF0000ull) return fail(ctx, RT3_E_ARG, "too many rays for one call (owned pixels x samples > 2^31 - 2^16)");
    return staged(ctx, { stage_out(out, n * sizeof(rt3_ray)) },
                  [&](void* const* d) { return rt3_lens_rays_device(ctx, lens, p, sample_begin, sample_count, d[0], ctx->stream); });
}

static int render_lens_checks(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, const void* out,
                              const char* what, bool device) {
    int rc = lens_checks(ctx, lens, p, out, what, device);
    if (rc) return rc;
    if ((rc = check_light_sampling(ctx, p->flags))) return rc;      // (the flag's own answers come before every older refusal)
    if (p->flags & (RT3_FLAG_REFERENCE_PRIMARY | RT3_FLAG_VARIANCE))
        return fail(ctx, RT3_E_ARG, "rt3_render_lens: RT3_FLAG_REFERENCE_PRIMARY and RT3_FLAG_VARIANCE do not apply to a lens frame");
    if ((p->flags & RT3_FLAG_ENV_SAMPLING) && (p->flags & RT3_FLAG_BLACK_BACKGROUND))
        return fail(ctx, RT3_E_ARG, "RT3_FLAG_ENV_SAMPLING cannot be combined with RT3_FLAG_BLACK_BACKGROUND or RT3_FLAG_REFERENCE_PRIMARY");
    if (!(p->lens_radius == 0.0f)) return fail(ctx, RT3_E_ARG, "rt3_render_lens: lens_radius must be 0 (no depth of field for the lens models)");
    if (!lens_sample_range_ok(p, sample_begin, sample_count)) return fail(ctx, RT3_E_ARG, "sample range outside [0, spp)");
    if ((uint64_t)rt3_rows_owned(p) * p->width > (1ull << 27)) return fail(ctx, RT3_E_ARG, "at most 2^27 owned pixels per lens render (shard the frame)");
    return 0;
}

int rt3_render_lens_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, void* d_out, void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = render_lens_checks(ctx, lens, p, sample_begin, sample_count, d_out, "d_out_rgba", true);
    if (rc) return rc;
    if ((rc = check_scene(ctx)) || (rc = check_env_sampling(ctx, p->flags)) || (rc = check_textures(ctx, p->flags))) return rc;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    const bool shard = p->tile_count > 1;                           // a whole frame's ray index is its frame pixel index: no keys
    if (shard && npix && (rc = ctx->d_lens_keys.ensure(ctx, npix))) return rc;
    uint32_t* const d_keys = shard ? ctx->d_lens_keys.get() : nullptr;
    const rt3_radiance_params rp{ p->max_depth, p->seed, p->flags & (RT3_FLAG_BLACK_BACKGROUND | RT3_FLAG_ENV_SAMPLING | RT3_FLAG_LIGHT_SAMPLING),
                                  sample_begin, sample_count, p->t_min };
    return radiance_pass(ctx, npix, rp, d_out, d_keys, nullptr, stream, [&](uint32_t s0, uint32_t ns) {
        return launch_lens_rays(ctx, lens, p, npix, s0, ns, ctx->d_arays, d_keys, stream);
    });
}

int rt3_render_lens(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, uint32_t sample_begin, uint32_t sample_count, float* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = render_lens_checks(ctx, lens, p, sample_begin, sample_count, out, "out_rgba", false);
    if (rc) return rc;
    if ((rc = check_scene(ctx))) return rc;
    return staged(ctx, { stage_out(out, (size_t)rt3_rows_owned(p) * p->width * 16u) },
                  [&](void* const* d) { return rt3_render_lens_device(ctx, lens, p, sample_begin, sample_count, d[0], ctx->stream); });
}

static int lens_aov_checks(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, const void* out, const char* what, bool device) {
    int rc = lens_checks(ctx, lens, p, out, what, device);
    if (rc) return rc;
    if (p->flags & RT3_FLAG_REFERENCE_PRIMARY) return fail(ctx, RT3_E_ARG, "rt3_render_lens_aov: RT3_FLAG_REFERENCE_PRIMARY does not apply to a lens frame");
    if (!(p->lens_radius == 0.0f)) return fail(ctx, RT3_E_ARG, "rt3_render_lens_aov: lens_radius must be 0 (no depth of field for the lens models)");
    return 0;
}

// aov_pass with k_lens_rays in k_camera_rays' place.
static int render_lens_aov_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, const rt3_aov_chain_params* chain, bool specular, void* d_out,
                                  void* stream_) {
    if (!ctx) return RT3_E_ARG;
    int rc = lens_aov_checks(ctx, lens, p, d_out, "d_out_aov", true);
    if (rc) return rc;
    if (specular) if (const char* why = rt3chain::refusal(chain)) return fail(ctx, RT3_E_ARG, std::string("rt3_render_lens_aov_specular: ") + why);
    if ((rc = check_scene(ctx)) || (rc = check_textures(ctx, 0u))) return rc;
    hipStream_t stream;
    if ((rc = enter(ctx, stream_, &stream))) return rc;
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    TraceArgs A = scene_args(ctx);                                  // the accumulation: the scene's records and the flags
    A.flags = p->flags;
    return aov_pass(ctx, p, A, d_out, stream, [&](uint32_t s0, uint32_t ns) {
        return launch_lens_rays(ctx, lens, p, npix, s0, ns, ctx->d_arays, nullptr, stream);
    }, chain);
}
int rt3_render_lens_aov_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, void* d_out, void* stream) {
    return render_lens_aov_device(ctx, lens, p, nullptr, false, d_out, stream);
}
int rt3_render_lens_aov_specular_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, const rt3_aov_chain_params* chain, void* d_out,
                                        void* stream) {
    return render_lens_aov_device(ctx, lens, p, chain, true, d_out, stream);
}

int rt3_render_lens_aov(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, rt3_aov* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = lens_aov_checks(ctx, lens, p, out, "out_aov", false);
    if (rc) return rc;
    if ((rc = check_scene(ctx))) return rc;
    return staged(ctx, { stage_out(out, (size_t)rt3_rows_owned(p) * p->width * sizeof(rt3_aov)) },
                  [&](void* const* d) { return rt3_render_lens_aov_device(ctx, lens, p, d[0], ctx->stream); });
}
int rt3_render_lens_aov_specular(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* p, const rt3_aov_chain_params* chain, rt3_aov* out) {
    if (!ctx) return RT3_E_ARG;
    int rc = lens_aov_checks(ctx, lens, p, out, "out_aov", false);
    if (rc) return rc;
    if (const char* why = rt3chain::refusal(chain)) return fail(ctx, RT3_E_ARG, std::string("rt3_render_lens_aov_specular: ") + why);
    if ((rc = check_scene(ctx))) return rc;
    return staged(ctx, { stage_out(out, (size_t)rt3_rows_owned(p) * p->width * sizeof(rt3_aov)) },
                  [&](void* const* d) { return rt3_render_lens_aov_specular_device(ctx, lens, p, chain, d[0], ctx->stream); });
}

int rt3_get_stats(rt3_ctx* ctx, rt3_stats* out) {
    if (!ctx || !out) return RT3_E_ARG;
    RT3_HIP(hipSetDevice(ctx->device));
    std::memset(out, 0, sizeof *out);
    if (!ctx->rendered) return fail(ctx, RT3_E_STATE, "no render has been issued on this context (or the last one failed)");
    RT3_HIP(hipEventSynchronize(ctx->ev_end));
    float ms = 0.0f;
    for (uint32_t i = 0; i < ctx->ev_used; i++) {
        float t = 0.0f;
        RT3_HIP(hipEventElapsedTime(&t, ctx->ev[i].first, ctx->ev[i].second));
        ms += t;
    }
    out->trace_ms = ms;
    RT3_HIP(hipEventElapsedTime(&out->total_ms, ctx->ev_begin, ctx->ev_end));
    out->launches = ctx->ev_used;
    out->samples = ctx->last_samples;
    out->n_spheres = ctx->n_sph;
    out->n_faces = ctx->n_faces;
    if (ctx->last_was_path) {
        unsigned long long counters[kCastSlots] = { 0 };
        RT3_HIP(hipMemcpy(counters, ctx->d_casts, sizeof counters, hipMemcpyDeviceToHost));
#ifdef RT3_PROFILE_PHASES
        if (counters[13] != 0) {                                     // k_trace_mfma: where its waves spend their time
            const double all = (double)(counters[11] + counters[12] + counters[13] + counters[14] + counters[15] + counters[17]);
            fprintf(stderr, "[rt3 profile] k_trace_mfma32 / k_trace_mfma, share of wave time: refill %.1f %%, ray operands (+ direct spheres) %.1f %%, scan %.1f %%, "
                            "push + exact tests %.1f %%, decode + shade %.1f %%, restock (primary pass) %.1f %%\n",
                    100.0 * counters[11] / all, 100.0 * counters[12] / all, 100.0 * counters[13] / all, 100.0 * counters[14] / all, 100.0 * counters[15] / all,
                    100.0 * counters[17] / all);
            if (counters[17] != 0)                                   // k_trace_mfma32's render form: the parts of a restock
                fprintf(stderr, "[rt3 profile] restock, share of its wave time: ray generation %.1f %%, list fetch %.1f %%, direct + listed tests %.1f %%, "
                                "shade %.1f %%, compaction %.1f %%\n", 100.0 * counters[18] / counters[17], 100.0 * counters[19] / counters[17],
                        100.0 * counters[20] / counters[17], 100.0 * counters[21] / counters[17], 100.0 * counters[22] / counters[17]);
        }
#endif
#ifdef RT3_PROFILE
        if (counters[13] == 0)
        fprintf(stderr, "[rt3 profile] wave iterations %llu, flush iterations/wave-iter %.2f, candidates/ray %.2f, live lanes/wave-iter %.1f, "
                        "fresh paths/wave-iter %.1f\n", counters[4], (double)counters[2] / (double)counters[4],
                (double)counters[3] / (double)counters[0], (double)counters[0] / (double)counters[4], (double)counters[5] / (double)counters[4]);
        if (counters[13] != 0) {                                     // tiled kernel: where its waves spend their time
            const double all = (double)(counters[12] + counters[13] + counters[14] + counters[15] + counters[4]);
            fprintf(stderr, "[rt3 profile] tiled kernel, share of wave time: barriers + tile fill %.1f %%, scan %.1f %%, push %.1f %%, exact tests %.1f %%, "
                            "refill / operands / shade %.1f %%\n", 100.0 * counters[12] / all, 100.0 * counters[13] / all, 100.0 * counters[14] / all,
                    100.0 * counters[15] / all, 100.0 * counters[4] / all);
        } else {
        fprintf(stderr, "[rt3 profile] first wave ended %.1f us before the last one\n", (double)(counters[7] - counters[6]) / 100.0);
        fprintf(stderr, "[rt3 profile] timeline from the first wave's start (us): last wave start %.1f, queue first seen empty %.1f, last seen empty %.1f, "
                        "first wave end %.1f, last wave end %.1f\n", (double)(counters[11] - counters[8]) / 100.0, (double)(counters[9] - counters[8]) / 100.0,
                (double)(counters[10] - counters[8]) / 100.0, (double)(counters[6] - counters[8]) / 100.0, (double)(counters[7] - counters[8]) / 100.0);
        }
#endif
        out->ray_casts = counters[0];
        out->prim_tests = counters[0] * ((uint64_t)ctx->n_sph + ctx->n_faces);
        out->mfma_instructions = counters[1];
        out->mfma_flop_per_instruction = counters[1] ? (ctx->last_mfma16 ? 16384u : 32768u) : 0u;
#ifndef RT3_PROFILE
        out->exact_tests = counters[2];
        out->bound_tests = counters[3];
#endif
        out->filter_tests = (ctx->last_filter_counted ? counters[16] : counters[0]) * ctx->last_filter_rows;
    } else {
        out->ray_casts = ctx->last_samples;
        out->prim_tests = ctx->last_samples * (uint64_t)ctx->n_faces;
    }
    return 0;
}

// Debug probe (tests only): element-wise device arithmetic, see tests/test_gpu_arith.py.
int rt3_debug_arith(rt3_ctx* ctx, const float* a, const float* b, uint32_t n, float* div, float* sq, float* fm,
                    float* cs, float* sn, float* sk3, uint32_t* pk) {
    if (!ctx) return RT3_E_ARG;
    RT3_HIP(hipSetDevice(ctx->device));
    float* d = nullptr;
    const size_t N = n;
    RT3_HIP(hipMalloc((void**)&d, N * 4 * 11));
    struct Free { float* p; ~Free() { (void)hipFree(p); } } free_on_return{ d };   // every early return below releases it
    float *da = d, *db = d + N, *ddiv = d + 2 * N, *dsq = d + 3 * N, *dfm = d + 4 * N, *dcs = d + 5 * N, *dsn = d + 6 * N, *dsk = d + 7 * N;
    uint32_t* dpk = (uint32_t*)(d + 10 * N);
    RT3_HIP(hipMemcpy(da, a, N * 4, hipMemcpyHostToDevice));
    RT3_HIP(hipMemcpy(db, b, N * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_arith, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, da, db, n, ddiv, dsq, dfm, dcs, dsn, dsk, dpk);
    RT3_HIP(hipGetLastError());
    RT3_HIP(hipStreamSynchronize(ctx->stream));
    RT3_HIP(hipMemcpy(div, ddiv, N * 4, hipMemcpyDeviceToHost));
    RT3_HIP(hipMemcpy(sq, dsq, N * 4, hipMemcpyDeviceToHost));
    RT3_HIP(hipMemcpy(fm, dfm, N * 4, hipMemcpyDeviceToHost));
    RT3_HIP(hipMemcpy(cs, dcs, N * 4, hipMemcpyDeviceToHost));
    RT3_HIP(hipMemcpy(sn, dsn, N * 4, hipMemcpyDeviceToHost));
    RT3_HIP(hipMemcpy(sk3, dsk, N * 12, hipMemcpyDeviceToHost));
    RT3_HIP(hipMemcpy(pk, dpk, N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Debug probe (tests only, host code): the counter-hash table as k_trace_mfma32's prologue fills it, see tests/test_restock_uniform.py.
uint32_t rt3_debug_ctr_table(uint32_t* out, uint32_t capacity_rows) {
    if (out) for (uint32_t k = 0; k < std::min(capacity_rows, kCtrDepthCap) * 4u; k++) out[k] = ctr_table_word(k);
    return kCtrDepthCap;
}

// Debug probe (tests only): the strip lists k_trace_mfma32's render form would use for this camera and these params, see tests/test_gpu_primary_lists.py.
int rt3_debug_primary_lists(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t* out_masks, uint64_t capacity_words, uint32_t* n_groups,
                            uint32_t* n_blocks) {
    if (!ctx) return RT3_E_ARG;
    if (!cam || !n_groups || !n_blocks) return fail(ctx, RT3_E_ARG, "cam / n_groups / n_blocks is NULL");
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (ctx->n_sph == 0 || ctx->n_faces != 0 || ctx->n_sph > kMfmaSphMax) return fail(ctx, RT3_E_STATE, "strip lists need a sphere-only scene of <= 512 spheres");
    hipStream_t stream;
    if ((rc = enter(ctx, nullptr, &stream))) return rc;
    const uint32_t npix = rt3_rows_owned(p) * p->width;
    *n_groups = (npix + 63u) / 64u;
    *n_blocks = (ctx->n_sph + 31u) / 32u;
    const size_t words = (size_t)*n_groups * *n_blocks;
    if (!out_masks || capacity_words < words) return fail(ctx, RT3_E_ARG, "out_masks holds fewer than n_groups * n_blocks words");
    if (words == 0) return 0;
    TraceArgs A;
    if ((rc = path_args(ctx, cam, p, npix, A)) || (rc = ctx->d_prim_masks.ensure(ctx, words))) return rc;
    launch_primary_lists(ctx, A, *n_groups, *n_blocks, stream);
    RT3_HIP(hipGetLastError());
    RT3_HIP(hipMemcpyAsync(out_masks, ctx->d_prim_masks.get(), words * 4, hipMemcpyDeviceToHost, stream));
    RT3_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
