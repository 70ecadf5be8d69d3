// rt3_ctx.hpp — the device context (struct rt3_ctx) and what every entry point shares, for every unit of the library that defines entry points:
// rt3_device.hip, rt3_scene.hip, rt3_denoise.hip, rt3_display.hip and rt3_display_sequence.hip.  The owned device buffers (DevBuf), RT3_HIP and fail, the
// stream convention and the event chain (stream_of, enter, leave), the host forms' round trip (staged) and ranges_overlap.  Needs
// <hip/hip_runtime.h> and rt3.h only: none of the kernel headers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "rt3.h"

// The kernel-side types the context's buffers hold, by name only (a DevBuf<T> member needs no more than T*): they belong to the unnamed
// namespace of the units that allocate and read those buffers (rt3_kernel_common.hpp, rt3_filter_frags.hpp), which complete them.
namespace {
struct Rgb;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
}  // namespace

// A device buffer of n elements of T that the context owns: freed when it is replaced and when the context is deleted.  A failed allocation
// leaves it null with capacity 0 and reports through ctx->err (alloc / upload below).
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }      // (what this held leaves with o)
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    int alloc(rt3_ctx* ctx, size_t n);                              // exactly n elements (n = 0: none)
    int ensure(rt3_ctx* ctx, size_t n) { return n_ >= n && p_ ? 0 : alloc(ctx, n); }     // grows only
    int upload(rt3_ctx* ctx, const std::vector<T>& v);              // exactly v (empty: none)
private:
    void swap(DevBuf& o) { std::swap(p_, o.p_); std::swap(n_, o.n_); }
    T* p_ = nullptr;
    size_t n_ = 0;
};

// The rows of the multi-level filter of one primitive class, built by build_rows: the members' (cx, cy, cz, r^2) records in
// group order and the primitive index of each, the leaf groups' bounds, the rows' bounds in f32 (rows behind a ray are dropped before their
// leaves are tested) and as fragments, and the super-rows of kSuper rows (four levels) as f32 records and as fragments.
struct FilterRows {
    DevBuf<float4> grp; DevBuf<uint32_t> perm; DevBuf<float4> leaf; DevBuf<float4> rowb; DevBuf<u32x4> gfrag; DevBuf<float4> srowb; DevBuf<u32x4> sfrag;
    uint32_t n_groups = 0, n_leaves = 0, n_super = 0;              // rows the matrix filter scans, leaf groups, super-rows
};

// What rt3_regroup* keeps per primitive class: the parts of every level above the LDS limit and of the level k_split_lds
// starts from, as begins[0 .. n_parts] one after the other — they depend on the count alone — built with the first regroup of a scene size.
struct RegroupPlan {
    struct Level { uint32_t offset, n_parts; };
    bool ready = false;
    uint32_t n_reg = 0, n_region = 0, max_parts = 0;                // primitives in the split region, its positions (pads included), parts of the widest global level
    size_t temp_bytes = 0;                                          // the radix sorts' temporary storage
    std::vector<Level> levels;
    DevBuf<uint32_t> table;
};

struct rt3_ctx {
    int device = 0;
    int num_cu = 0;
    hipStream_t stream = nullptr;                                   // used by the synchronous entry points
    std::string err;

    // mesh
    uint32_t n_faces = 0;
    DevBuf<float4> d_tri, d_tri_mat, d_tri_bound; DevBuf<uint32_t> d_tri_kind; DevBuf<u32x4> d_tri_frag;
    // merged entity buffers on the device (GFace[] / vec4[] as the reference keeps them), filled by rt3_mesh_*; their sizes bound rt3_mesh_put
    DevBuf<rt3_gface> d_gfaces; DevBuf<float4> d_verts;
    bool mesh_in_sync = false;                                      // d_gfaces / d_verts are what the committed faces were built from (rt3_motion reads them)
    DevBuf<rt3_material> d_face_mats_in; DevBuf<uint32_t> d_error;
    // spheres
    uint32_t n_sph = 0;
    DevBuf<float4> d_sph; DevBuf<uint32_t> d_sph_frag, d_sph_frag32; float sph_centre[3] = { 0.0f, 0.0f, 0.0f }; uint32_t n_direct = 0; uint32_t direct[4] = { 0, 0, 0, 0 }; float tri_centre[3] = { 0.0f, 0.0f, 0.0f }; DevBuf<uint32_t> d_box; DevBuf<u32x4> d_tri_frag_r; DevBuf<float> d_sph_invr; DevBuf<float4> d_sph_mat; DevBuf<uint32_t> d_sph_kind;

    DevBuf<float4> d_sph_cr;                                        // (C, r) as the caller gave them, in the caller's order (rt3_motion compares and scales by them)
    // what rt3_update_spheres* needs from the last rt3_set_spheres: every sphere's position in sph.grp (0xFFFFFFFF: a direct sphere), and whether
    // a sphere was left out of the group order for a non-finite record (an update could make it finite again, and it has no slot)
    DevBuf<uint32_t> d_sph_slot; bool sph_left_out = false;
    // rt3_regroup*: the faces face_group_order put in the bounded part at commit; the plans; scratch (centres, ping-pong ids and keys, the
    // parts' boxes, sort temporaries), grown by the first regroup of a scene size and kept
    uint32_t tri_bounded = 0;
    RegroupPlan rg_sph, rg_tri;
    DevBuf<float4> d_rg_cen; DevBuf<uint32_t> d_rg_ids[2], d_rg_box; DevBuf<uint64_t> d_rg_keys[2]; DevBuf<uint8_t> d_rg_temp;
    DevBuf<uint32_t> d_sb;                                          // rt3_set_*_device: the build's header and the compaction's block counts (rt3_scene_build.hpp)
    bool update_error_pending = false;                              // a device-form rt3_update_mesh_device with faces: d_error is read by the next rt3_synchronize

    // rows of the multi-level filter: faces and spheres, each in the order of a spatial median split
    FilterRows tri, sph;
    DevBuf<float4> d_tri_rec;                                       // the faces' records in group order (the exact test of the multi-level filter reads these)
    DevBuf<uint32_t> d_strips;                                      // deferred member tests: kStripPairs pairs per wave of the grid
    DevBuf<uint32_t> d_prim_masks;                                  // strip lists of the last k_trace_mfma32 render: [group of 64 owned pixels][row block]
    // environment map (rt3_set_environment*): the context's copy, 6 faces of env_n x env_n float4 texels; env_n == 0: none.  Scene
    // uploads, updates and regroups never touch it.
    DevBuf<float4> d_env; uint32_t env_n = 0;
    // ... and its sampling table (RT3_FLAG_ENV_SAMPLING): env_m cells per face edge, the cells' quantised weights and their inclusive
    // prefix sums.  Built by the first call that carries the flag (ensure_env_table), kept until the map is set or cleared again (env_table = false).
    DevBuf<uint32_t> d_env_q, d_env_wmax; DevBuf<unsigned long long> d_env_cdf; DevBuf<uint8_t> d_env_temp; uint32_t env_m = 0; bool env_table = false;
    // the emitters' sampling table (RT3_FLAG_LIGHT_SAMPLING): one entry per primitive, faces first and then spheres in the caller's order,
    // the entries' quantised weights and their inclusive prefix sums.  Built by the first call that carries the flag (ensure_light_table), kept until the
    // scene changes: every upload, commit and update sets light_table = false; regroups and the environment calls do not.  d_env_wmax and d_env_temp
    // (the largest weight, the scan's scratch) are shared with the map's table: both builds are queued behind the event chain.
    DevBuf<uint32_t> d_light_q; DevBuf<unsigned long long> d_light_cdf; bool light_table = false;
    // image textures (rt3_set_texture*, rt3_bind_*_textures*): the slots' own copies (w == 0: empty) and their descriptors on the device
    // (d_tex_slots, RT3_TEX_MAX_TEXTURES of them, written behind the event chain); per class the binding in the caller's order and, on the host, the set
    // of slots it names (one bit per slot) — all zero: the class has no binding, whatever d_*_tex still holds.  Uploads of a class clear its set
    // (drop_*_binding); updates and regroups never touch any of this.
    struct TexSlot { DevBuf<float4> texels; uint32_t w = 0, h = 0, wrap = 0; };
    TexSlot tex[RT3_TEX_MAX_TEXTURES];
    DevBuf<uint4> d_tex_slots; DevBuf<uint32_t> d_sph_tex, d_tri_tex, d_tex_check; DevBuf<float2> d_tri_uv;
    uint32_t sph_tex_used[RT3_TEX_MAX_TEXTURES / 32] = {}, tri_tex_used[RT3_TEX_MAX_TEXTURES / 32] = {};

    // work buffers
    DevBuf<Rgb> d_rad;
    DevBuf<float4> d_accum;
    DevBuf<float4> d_accum_sq;                                      // RT3_FLAG_VARIANCE: per-pixel sums of squares
    DevBuf<float4> d_arays;                                         // first-hit AOVs (rt3_render_aov*): one batch's camera rays and their hits,
    DevBuf<uint4> d_ahits;                                          // and the per-pixel running sums (three planes; not d_accum, which belongs to
    DevBuf<float4> d_aacc;                                          // the progressive render)
    // specular-chain AOVs (rt3_render_aov_specular*): per item of a batch the bounce queries' hits (the primary ones stay in d_ahits),
    // the chain's state (T, L) and its last normal; the count of chains still running, read back once per bounce
    DevBuf<uint4> d_chits; DevBuf<float4> d_cstate, d_cnorm; DevBuf<uint32_t> d_calive;
    DevBuf<uint32_t> d_lens_keys;                                  // a shard's frame pixel indices (rt3_render_lens*: the keys of its rays)
    DevBuf<float4> d_dn;                                            // denoiser scratch (rt3_denoise*): two (I, v) planes, the guide plane, the depth slopes
    // the display transform's auto-exposure (rt3_display*): hist[512], dark, n and the gain's bits, allocated by the first call with the flag and
    // zeroed at the start of each such call; display_auto: there has been one (rt3_debug_display_state)
    DevBuf<uint32_t> d_display; bool display_auto = false;
    // the bloom pyramid of rt3_display_sequence* (DESIGN.md 4.25): D_1 .. D_L one behind the other, grown on demand and kept after the call —
    // plane 1 then holds U_1 of the bloom_w x bloom_h frame (bloom_levels != 0: there has been such a call); d_bloom_plane: rt3_debug_display_bloom's B
    DevBuf<float4> d_bloom, d_bloom_plane; uint32_t bloom_w = 0, bloom_h = 0, bloom_levels = 0;
    // The host forms' inputs and results on the device, each carved out at a float4 offset by staged().  Shared by all of them: each one ends in
    // hipStreamSynchronize(ctx->stream), and no device form touches it.
    DevBuf<float4> stage;
    DevBuf<uint32_t> d_work;                                        // [0] work counter
    DevBuf<unsigned long long> d_casts;
    uint64_t rad_cap_bytes = 16ull << 30;
    bool force_plain_mode_r = false;                                // tests: compare the two Mode-R kernels
    bool force_brute = false;                                       // tests / fuzzers: unfiltered Mode-X kernel
    bool force_flat = false;                                        // tests / A-B: one filter row per primitive (no groups)
    uint64_t last_filter_rows = 0;                                  // rows the matrix filter scanned per ray cast in the last Mode-X render
    bool last_filter_counted = false;                               // ... and the kernel counted the casts that took the filter itself (d_casts[16])
    // the accumulation a progressive render continues (rt3_render_path_range): what it belongs to and how far it got
    bool acc_valid = false; rt3_params acc_params{}; rt3_camera acc_cam{}; uint32_t acc_done = 0; uint32_t acc_npix = 0;
    // adaptive sampling (rt3_render_path_adaptive*): the accumulation holds a different number of samples per pixel, d_counts[pix]; the two
    // active lists (ping-pong), the rule's verdict per pixel, the compaction's block counts and, behind them, the length of the new list
    bool acc_adaptive = false;
    DevBuf<uint32_t> d_counts, d_active[2], d_block_counts; DevBuf<uint8_t> d_unconverged;
    // launch configuration per (kernel, dynamic LDS): max dynamic LDS attribute set, workgroups per CU
    std::map<std::pair<const void*, size_t>, int> occupancy;
    std::set<int> peers_enabled;                                    // devices this context's device may already write to

    // stats of the last render
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;              // per dominant-kernel launch
    uint32_t ev_used = 0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t ev_acc = nullptr; bool ev_acc_recorded = false;      // end of the last Mode-X render: what the next user of d_rad / d_accum waits for
    hipStream_t last_stream = nullptr;
    uint64_t last_samples = 0;
    bool last_was_path = false;
    bool last_mfma16 = false;                                       // the last trace kernel was a tiled one (16x16x32 MFMAs)
    bool rendered = false;
    // what the render in flight will report once its last launch has been issued (committed only then)
};

#define RT3_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
            return RT3_E_DEVICE;                                                                        \
        }                                                                                               \
    } while (0)

template <typename T>
int DevBuf<T>::alloc(rt3_ctx* ctx, size_t n) {
    reset();
    if (n) RT3_HIP(hipMalloc((void**)&p_, n * sizeof(T)));
    n_ = n;
    return 0;
}
template <typename T>
int DevBuf<T>::upload(rt3_ctx* ctx, const std::vector<T>& v) {
    const int rc = alloc(ctx, v.size());
    if (rc) return rc;
    if (!v.empty()) RT3_HIP(hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// A refusal: the message rt3_last_error returns, and the code.
inline int fail(rt3_ctx* ctx, int code, const std::string& msg) { ctx->err = msg; return code; }

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// ---- What the entry points share.  rt3.h: a NULL stream is the context's own.
inline hipStream_t stream_of(const rt3_ctx* ctx, void* stream_) { return stream_ ? (hipStream_t)stream_ : ctx->stream; }

// d_rad, d_accum, the scratch and the counters belong to the context, not to a stream: whatever stream the previous call ran on, this one
// starts behind it (a wait on the device; nothing if it is the same stream).  leave() marks where the next call starts.
inline int enter(rt3_ctx* ctx, void* stream_, hipStream_t* stream) {
    RT3_HIP(hipSetDevice(ctx->device));
    *stream = stream_of(ctx, stream_);
    if (ctx->ev_acc_recorded) RT3_HIP(hipStreamWaitEvent(*stream, ctx->ev_acc, 0));
    return 0;
}
inline int leave(rt3_ctx* ctx, hipStream_t stream) {
    RT3_HIP(hipEventRecord(ctx->ev_acc, stream));
    ctx->ev_acc_recorded = true;
    return 0;
}

// The round trip of a host form — the variant of an entry point that takes host pointers — through ctx->stage.  A StageSeg is one input or one result,
// its host pointer and its bytes: a NULL pointer is an absent optional segment, an empty one (a shard that owns no pixel) is never copied.  staged() sizes
// the buffer ONCE for all of them (DevBuf::ensure frees what it replaces: no segment can be added behind the first copy), queues the inputs' copies on
// ctx->stream, calls device_form(d) — d[i]: segment i's 16-byte-aligned address, NULL for an absent one — then queues the results' copies and waits.
struct StageSeg { const void* src; void* dst; size_t bytes; bool present; };
inline StageSeg stage_in(const void* host, size_t bytes) { return { host, nullptr, bytes, host != nullptr }; }
inline StageSeg stage_out(void* host, size_t bytes) { return { nullptr, host, bytes, host != nullptr }; }
template <size_t N, class DeviceForm>
int staged(rt3_ctx* ctx, const StageSeg (&seg)[N], DeviceForm device_form) {
    RT3_HIP(hipSetDevice(ctx->device));
    size_t first[N], quads = 0;
    for (size_t i = 0; i < N; i++) { first[i] = quads; if (seg[i].present) quads += std::max<size_t>((seg[i].bytes + 15) / 16, 1); }
    int rc;
    if ((rc = ctx->stage.ensure(ctx, std::max<size_t>(quads, 1)))) return rc;
    void* d[N];
    for (size_t i = 0; i < N; i++) {
        d[i] = seg[i].present ? ctx->stage.get() + first[i] : nullptr;
        if (seg[i].src && seg[i].bytes) RT3_HIP(hipMemcpyAsync(d[i], seg[i].src, seg[i].bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = device_form(d))) return rc;
    for (size_t i = 0; i < N; i++)
        if (seg[i].dst && seg[i].bytes) RT3_HIP(hipMemcpyAsync(seg[i].dst, d[i], seg[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
    RT3_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
