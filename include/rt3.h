/* rt3.h — C ABI of the MI355X-native render path (librt3hip.so).
 *
 * Drop-in boundary for the reference's per-pixel ray-trace loop.  The reference's own boundary is the
 * C++ class RayTracer::Renderer (src/lib/renderer/Renderer.hpp:34-63: prerender() / render() /
 * initialize_renderer()); the C++ mirror of that class lives in raytracer-3_amd/host/ and is a thin
 * wrapper over the entry points declared here.  Everything below is plain pointers and sizes so that any
 * FFI (ctypes, cgo, JNI ...) can bind it; INTEGRATION.md shows the binding a reference maintainer adds.
 *
 * Two render modes:
 *   Mode R  ("reference mode")  rt3_render*      — exactly SequentialRenderer::render + ray_color
 *            (src/lib/renderer/SequentialRenderer.cpp:47-109, 269-308): 1 primary ray per pixel,
 *            brute-force nearest indexed triangle, flat baked face colour, sky gradient, RGBA8 pack.
 *   Mode X  ("extension mode")  rt3_render_path* — analytic spheres, materials, spp, depth, counter-based
 *            RNG, as sketched (never finished) by src/lib/shaders/raytracer/raytracer_v4.glsl and
 *            random_v1.glsl; semantics are specified in DESIGN.md and restated on the CPU in oracle/.
 *
 * All functions returning int return 0 on success and a negative code on failure; the message is
 * available from rt3_last_error().  Nothing here falls back to the CPU: without a HIP device every
 * device entry point fails with RT3_E_DEVICE.
 */
#ifndef RT3_H
#define RT3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header: bumped whenever a wire struct changes size or meaning.  A host compares it with what the library
 * it loaded reports before it passes any struct (rt3_stats grew from 56 to 64 bytes between versions 1 and 2; rt3_get_stats writes
 * sizeof(rt3_stats) bytes of THIS version).  History: 1 = round 1; 2 = + mfma_instructions / exact_tests in rt3_stats, progressive
 * accumulation, rt3_gather_rows; 3 = + rt3_abi_version itself, one stream convention (below),
 * filter_tests / bound_tests in rt3_stats (80 bytes).  Still 3 with rt3_update_spheres* / rt3_update_mesh*, with
 * rt3_render_path_adaptive* (one new struct of its own), with rt3_regroup*, with the environment map (rt3_set_environment*), with its
 * importance sampling (RT3_FLAG_ENV_SAMPLING: one flag bit and two test-only functions), with the emitters' (RT3_FLAG_LIGHT_SAMPLING: the same again)
 * with the display transform (rt3_display*: one new struct of its own), with the lens models (rt3_lens_rays*, rt3_render_lens*,
 * rt3_render_lens_aov*: one new struct of its own), with lens sequences (rt3_denoise_temporal_optic*, rt3_motion_optic*), with display
 * sequences (rt3_display_sequence*: two new structs of their own), with image textures (rt3_set_texture*, rt3_bind_*_textures*: no struct) and
 * with specular-chain AOVs (rt3_render_aov_specular*, rt3_render_lens_aov_specular*: one new struct of its own):
 * functions were only added, no existing struct changed. */
#define RT3_ABI_VERSION 3u
uint32_t rt3_abi_version(void);

/* Stream convention of every entry point that takes a `stream` (a hipStream_t): the work is queued on that stream; NULL means the
 * CONTEXT'S OWN stream (rt3_stream()), never the legacy default stream.  Calls on one context are ordered with each other whatever
 * streams they name: a render that continues, overwrites or reads the accumulation waits (on the device) for the event the previous
 * render recorded, rt3_accum_download / rt3_accum_upload wait for it on the host. */

#define RT3_E_ARG     (-1)   /* bad argument */
#define RT3_E_DEVICE  (-2)   /* HIP runtime / device failure (includes "no device") */
#define RT3_E_IO      (-3)   /* file could not be opened / parsed */
#define RT3_E_STATE   (-4)   /* no scene set, etc. */

/* ---------------------------------------------------------------------------------------------------
 * Wire structs
 * ------------------------------------------------------------------------------------------------- */

/* == RayTracer::GFace (src/lib/renderer/Vertex.hpp:39-51; GLSL std430 twin raytracer_v3.glsl:33-45).
 * 48 bytes: u32 v1,v2,v3 @0/4/8; vec3 normal @16; vec3 color @32. */
typedef struct rt3_gface {
    uint32_t v1, v2, v3;
    uint32_t _pad0;
    float    normal[3];
    uint32_t _pad1;
    float    color[3];
    uint32_t _pad2;
} rt3_gface;

/* == the four public vectors of RayTracer::Camera (src/lib/camera/Camera.hpp:27-34), i.e. the
 * GCameraData block the Vulkan backend uploads (src/lib/renderer/VulkanRenderer.hpp:32-37). */
typedef struct rt3_camera {
    float origin[3];
    float horizontal[3];
    float vertical[3];
    float lower_left_corner[3];
} rt3_camera;

/* Material kinds (Mode X).  RT3_MAT_FLAT is the only material the reference has: the hit returns the
 * baked colour and the path ends (SequentialRenderer.cpp:101-103); it doubles as a diffuse emitter. */
#define RT3_MAT_FLAT        0u   /* radiance += throughput * rgb ; path ends                     */
#define RT3_MAT_LAMBERT     1u   /* rgb = albedo                                                  */
#define RT3_MAT_METAL       2u   /* rgb = albedo, param = fuzz in [0,1]                           */
#define RT3_MAT_DIELECTRIC  3u   /* param = index of refraction (rgb ignored, attenuation = 1)    */

typedef struct rt3_material {
    float    rgb[3];
    float    param;
    uint32_t kind;
} rt3_material;

#define RT3_FLAG_GAMMA2            1u   /* sqrt() each channel before packing (book gamma 2)           */
#define RT3_FLAG_BLACK_BACKGROUND  2u   /* a miss contributes nothing (default: the reference's sky)    */
/* The primary ray (ray cast 0) is traced exactly as SequentialRenderer.cpp:289-297 does it: the direction is left
 * UNNORMALISED (:293), faces are tested with the reference's literal formula t = (n.o + n.p1) / (n.d) (:70, sic) and
 * a miss shades sky(d) of that unnormalised d (:105-107).  With spp 1, max_depth 1, flat faces, t_min 0 and no
 * gamma, Mode X then IS Mode R, byte for byte (consequence 1(i)); later ray casts are the
 * normal Mode-X ones.  Triangle-only scenes. */
#define RT3_FLAG_REFERENCE_PRIMARY 4u
/* Keep a per-pixel, per-channel sum of squared sample radiances beside the sums (variance estimates; the
 * "sample storage" half of reduce_v1.glsl's intent).  Read both back with rt3_accum_download(). */
#define RT3_FLAG_VARIANCE          8u
/* Importance sampling of the environment map with one shadow ray per Lambert scatter (next-event estimation): "Environment map: sampling"
 * below.  Needs a map (rt3_set_environment*); without the flag every entry point returns what it returned before the flag existed. */
#define RT3_FLAG_ENV_SAMPLING      16u
/* Importance sampling of the emissive primitives (RT3_MAT_FLAT) with one shadow ray per Lambert scatter: "Emitters: sampling" below.  Not together
 * with RT3_FLAG_ENV_SAMPLING; without the flag every entry point returns what it returned before the flag existed. */
#define RT3_FLAG_LIGHT_SAMPLING    32u

/* Parameters of a Mode-X render.  tile_*: interleaved row-block sharding of the framebuffer
 * (design intent: BlockInfo{x,y,w,h} of raytracer_v4.glsl:70-79).  Row-block b (tile_rows rows) belongs
 * to shard (b mod tile_count); a shard renders only its own rows, into a compact buffer of
 * rt3_rows_owned() rows.  tile_count = 1 renders the whole frame. */
typedef struct rt3_params {
    uint32_t width, height;      /* full frame */
    uint32_t spp;                /* samples per pixel, >= 1 */
    uint32_t max_depth;          /* ray casts per path, >= 1 (book "max_depth") */
    uint32_t seed;
    uint32_t flags;
    float    lens_radius;        /* 0 = pinhole */
    float    t_min;              /* self-intersection cut-off; book value 0.001 */
    uint32_t tile_rows, tile_index, tile_count;
} rt3_params;

/* Counters of the last render on a context (device-side counts, HIP-event timings on the render stream). */
typedef struct rt3_stats {
    uint64_t ray_casts;          /* rays traced (primary + scattered; primary rays traced against the strip lists included) */
    uint64_t prim_tests;         /* ray-primitive tests = ray_casts * (n_spheres + n_faces)          */
    uint64_t samples;            /* pixels * spp rendered by this call                               */
    float    trace_ms;           /* dominant kernel (trace / mode-R) duration, summed over launches  */
    float    total_ms;           /* first launch -> last launch of the call (device time)            */
    uint32_t launches;           /* launches of the dominant kernel                                  */
    uint32_t n_spheres, n_faces;
    uint32_t mfma_flop_per_instruction;   /* 32768 (v_mfma_f32_32x32x16_bf16: k_trace_mfma) or 16384 (v_mfma_f32_16x16x32_bf16: tiled kernels) */
    uint64_t mfma_instructions;  /* bf16 MFMA wave-instructions issued by the candidate filter (0: VALU scan / brute force) */
    uint64_t exact_tests;        /* (ray, primitive) pairs that survived the filter(s) and went through the exact test
                                    (counted by the pair-list kernels; 0 elsewhere); the tests of primary rays against their
                                    strip lists (below) are counted here too                                             */
    uint64_t filter_tests;       /* (ray, row) pairs the matrix filter evaluated = (ray casts that took the filter) * rows.  Every
                                    cast takes it, except in sphere scenes of <= 512 spheres: there the primary rays of 64
                                    consecutive pixels are traced against a short list of the spheres their beam can meet and
                                    skip the filter (RT3_PRIMARY_LISTS=0 turns that off, RT3_PRIMARY_LIST_MAX=n sets the longest
                                    list still traced that way), so filter_tests < ray_casts * rows.  A row is one primitive in the
                                    flat filter and a group of primitives in the two-level filter, so this is what
                                    the matrix cores executed, while prim_tests is the brute-force-equivalent count              */
    uint64_t bound_tests;        /* two-level filter, faces: members of candidate groups checked against their own bounding sphere */
} rt3_stats;

typedef struct rt3_ctx rt3_ctx;

/* ---------------------------------------------------------------------------------------------------
 * Device context   (replaces the Vulkan Instance/GPU/MemoryPool bring-up of VulkanRenderer.cpp:43-94)
 * ------------------------------------------------------------------------------------------------- */
rt3_ctx*    rt3_create(int device_id);
void        rt3_destroy(rt3_ctx* ctx);
/* ctx may be NULL to read the error of a failed rt3_create(). */
const char* rt3_last_error(const rt3_ctx* ctx);
/* Optional: cap (bytes) for the per-sample radiance storage; more spp than fit are rendered in batches. */
int         rt3_set_sample_storage_cap(rt3_ctx* ctx, uint64_t bytes);

/* ---------------------------------------------------------------------------------------------------
 * Scene upload   (replaces Renderer::prerender's upload half: SequentialRenderer.cpp:174-195,246 /
 *                 VulkanRenderer.cpp:210-261,355-387).  Replaces any previous scene of that kind.
 * ------------------------------------------------------------------------------------------------- */
/* faces/vertices are the merged arrays exactly as the reference keeps them (GFace[], vec4[] w=0).
 * face_materials may be NULL: every face is then RT3_MAT_FLAT with its own GFace colour (Mode R). */
int rt3_set_mesh(rt3_ctx* ctx, const rt3_gface* faces, uint32_t n_faces,
                 const float* vertices_xyzw, uint32_t n_vertices,
                 const rt3_material* face_materials);
/* Incremental form of the same upload, mirroring VulkanRenderer::prerender (VulkanRenderer.cpp:266-399): size the two
 * device buffers from the entities' pre-declared counts, then fill them entity by entity at running offsets —
 *   rt3_mesh_put     a CPU-pre-rendered entity; indices are rebased by vertex_offset (transfer_entity, :210-261)
 *   rt3_mesh_sphere  a sphere tessellated ON THE DEVICE straight into the buffers (gpu_pre_render_sphere,
 *                    src/lib/entities/Sphere.cpp:355-491; shaders pre_render_sphere_v2_vertices/faces.glsl)
 * and finally rt3_mesh_commit() de-indexes the merged arrays for the render kernels (face_materials as in rt3_set_mesh).
 * rt3_mesh_download() copies the merged GFace[] / vec4[] back (the check the author left commented out at
 * VulkanRenderer.cpp:329-353). */
int rt3_mesh_begin(rt3_ctx* ctx, uint32_t n_faces, uint32_t n_vertices);
int rt3_mesh_put(rt3_ctx* ctx, const rt3_gface* faces, uint32_t n_faces, const float* vertices_xyzw, uint32_t n_vertices,
                 uint32_t face_offset, uint32_t vertex_offset);
int rt3_mesh_sphere(rt3_ctx* ctx, const float center[3], float radius, uint32_t n_meridians, uint32_t n_parallels,
                    const float color[3], uint32_t face_offset, uint32_t vertex_offset);
int rt3_mesh_commit(rt3_ctx* ctx, const rt3_material* face_materials);
int rt3_mesh_download(rt3_ctx* ctx, rt3_gface* faces, float* vertices_xyzw);

/* center_radius: 4 floats per sphere (cx,cy,cz,r), r > 0.  (Sphere{vec3 center; float radius; vec3 color},
 * raytracer_v4.glsl:42-49.) */
int rt3_set_spheres(rt3_ctx* ctx, const float* center_radius, const rt3_material* materials, uint32_t n);

/* ---------------------------------------------------------------------------------------------------
 * Scene upload from device arrays   (a scene that is made or changes its counts on the device)
 * ------------------------------------------------------------------------------------------------- */
/* rt3_set_spheres_device: after the call the context is in the state that rt3_set_spheres(<the same arrays>) followed by
 * rt3_regroup(RT3_REGROUP_SPHERES) leaves, so every entry point (render, range render, adaptive, query, AOV, motion, Mode R) returns bit
 * for bit what it returns after the host upload, rt3_debug_group_order returns the regroup order of the usable spheres (not on the direct
 * list, a finite centre and a finite r^2), and rt3_update_spheres* / rt3_regroup* work on the result as after a host upload.  A sphere
 * with a non-finite record is left out of the group order as on the host (an update then returns RT3_E_STATE); unlike rt3_regroup the
 * build works with such spheres.  rt3_set_mesh_device: the same against rt3_set_mesh(...) followed by rt3_regroup(RT3_REGROUP_MESH);
 * indices are taken as given (no rebasing), the merged entity buffers afterwards hold the caller's arrays (rt3_mesh_download,
 * rt3_update_mesh* work) and d_face_materials may be NULL as in rt3_set_mesh.
 * d_center_radius: n x (cx, cy, cz, r) floats; d_materials: n rt3_material; d_faces: n_faces rt3_gface; d_vertices_xyzw: n_vertices x 4
 * floats.  The arrays are only read; they must stay valid until the work queued on `stream` has run.
 * The filter centre is rt3_set_spheres' (the component-wise median of the finite coordinates), the direct list its set of at most four
 * spheres whenever there are at most four candidates or the candidates' ratios are pairwise distinct; among more than four candidates
 * with equal ratios any four of the largest are taken (any choice is correct: it changes the filter's work, never a result).
 * Two phases, one wait: phase 1 reads the caller's arrays and writes scratch; the call then waits for the device ONCE, to read back a few
 * dozen bytes (the buffer sizes depend on them); phase 2 allocates and queues the rest on `stream`.  So the device forms can refuse:
 * RT3_E_ARG with the scene untouched for a radius that is not > 0 (NaN included; the message names the lowest such index), a material
 * kind above RT3_MAT_DIELECTRIC, a NULL array with a non-zero count, a pointer that is not 16-byte aligned (4-byte for the material
 * arrays) and a NULL ctx.  A face index out of range returns RT3_E_ARG and leaves the context without a mesh, as rt3_set_mesh does.
 * n == 0 / n_faces == 0 clears that class (the pointers may then be NULL).  Streams follow the convention above and the event chain of
 * the updates.  Not for graph capture (the wait). */
int rt3_set_spheres_device(rt3_ctx* ctx, const void* d_center_radius, const void* d_materials, uint32_t n, void* stream);
int rt3_set_mesh_device(rt3_ctx* ctx, const void* d_faces, uint32_t n_faces, const void* d_vertices_xyzw, uint32_t n_vertices,
                        const void* d_face_materials, void* stream);
/* Tests only.  rt3_debug_sphere_plan: what rt3_set_spheres decides for these records, on the host (no device, no context): the filter
 * centre and the direct list (unused entries 0xFFFFFFFF); returns the length of the list.  rt3_debug_sphere_build: what the context
 * holds after the last sphere upload of either form; RT3_E_STATE without spheres. */
uint32_t rt3_debug_sphere_plan(const float* center_radius, uint32_t n, float centre[3], uint32_t direct[4]);
int rt3_debug_sphere_build(rt3_ctx* ctx, float centre[3], uint32_t direct[4], uint32_t* n_direct);

/* ---------------------------------------------------------------------------------------------------
 * Scene update   (new positions for the scene that is there: a refit on the device)
 * ------------------------------------------------------------------------------------------------- */
/* rt3_update_spheres*: after the call every entry point (render, range render, query, AOV, motion, Mode R) returns bit for bit what it
 * would return after rt3_set_spheres(center_radius, <the materials of the last rt3_set_spheres>, n).  rt3_update_mesh*: the same against
 * rt3_set_mesh(faces', vertices_xyzw, n_vertices, <the face materials of the last commit>), faces' = `faces`, or with faces == NULL the
 * context's own GFace[]: indices, stored normals and colours are kept and only the positions change.  A non-NULL `faces` holds the
 * context's face count of records and is how a caller supplies new normals (the render layout takes the STORED normal, so a deforming mesh
 * that wants correct shading passes them).  Materials, counts and the grouping do not change; only performance may differ from a full
 * upload.  What is kept from the last full upload: the group order and the sphere permutation, the direct-sphere list, and the centres the
 * filter's coordinates are taken about (the spheres' median centre, the vertex box of the mesh) — each affects only how many candidates
 * the filter passes, never the result; re-upload in full when the scene has drifted far.
 * Counts: n must equal the context's sphere count, n_vertices the vertex count of the merged entity buffers (rt3_mesh_download), else
 * RT3_E_ARG.  RT3_E_STATE without a committed scene of that class; while the merged entity buffers are out of sync with the commit
 * (rt3_mesh_begin / rt3_mesh_put / rt3_mesh_sphere without an rt3_mesh_commit); and when the last rt3_set_spheres left a sphere with a
 * non-finite record out of the grouping (an update could make it finite again, and it has no place in the rows).
 * The device forms (16-byte aligned pointers, RT3_E_ARG otherwise) allocate nothing, never wait for the device and cannot refuse a bad
 * record: a sphere record that is not finite, or whose radius is not positive, becomes a sphere nothing can hit (rt3_motion still reports
 * the record as it was passed); a face of a supplied `faces` with a vertex index out of range becomes a face nothing can hit, and the
 * next rt3_synchronize on the context returns RT3_E_ARG for it, once (rt3_get_stats does not report it).  The host forms are synchronous
 * and refuse instead: RT3_E_ARG for a radius that is not positive, with the scene untouched; RT3_E_ARG for a face index out of range, which
 * leaves the context without a mesh, as rt3_set_mesh would.
 * Streams follow the convention above: an update waits for the event the previous render, query or update recorded and records its own,
 * so the next call on any stream sees the new scene.  The accumulation of a progressive render is treated as a full upload treats it: it
 * is left alone, and what continuing it over a changed scene means is the caller's business. */
int rt3_update_spheres(rt3_ctx* ctx, const float* center_radius, uint32_t n);
int rt3_update_spheres_device(rt3_ctx* ctx, const void* d_center_radius, uint32_t n, void* stream);
int rt3_update_mesh(rt3_ctx* ctx, const rt3_gface* faces, const float* vertices_xyzw, uint32_t n_vertices);
int rt3_update_mesh_device(rt3_ctx* ctx, const void* d_faces, const void* d_vertices_xyzw, uint32_t n_vertices, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Regroup   (the group order of the candidate filter again, from the positions on the device)
 * ------------------------------------------------------------------------------------------------- */
/* Updates keep the group order of the last full upload, and a scene whose neighbours have scattered pays for it in candidates.
 * rt3_regroup* reorders the primitives among the positions they already occupy — the median split of a full upload, as a stable sort
 * per part, on the device — and runs the refit's tail.  After it every entry point returns bit for bit what it returned before (and so
 * what it returns after a full upload of the same arrays); only the filter counters of rt3_stats and the time may change.  Counts,
 * materials, the direct-sphere list, the filter centres, every buffer size, the set of primitives in the split region (the spheres that
 * had a slot at rt3_set_spheres; the faces with a bounded hit region at commit), the pads and the unbounded faces' tail are kept.
 * `what`: RT3_REGROUP_SPHERES | RT3_REGROUP_MESH, at least one.  rt3_regroup is synchronous; rt3_regroup_device is queued on `stream`
 * (convention above), takes part in the event chain as an update does, and after its first call for a scene size allocates nothing and
 * never waits for the device.  The accumulation of a progressive render is left alone.
 * Errors: RT3_E_ARG for a NULL ctx, what == 0 or unknown bits; RT3_E_STATE without a committed scene of a named class, with merged
 * entity buffers out of sync with the commit, and when the last rt3_set_spheres left a non-finite sphere out of the group order.  A
 * class without rows (every sphere on the direct list) is a successful no-op. */
#define RT3_REGROUP_SPHERES 1u
#define RT3_REGROUP_MESH    2u
int rt3_regroup(rt3_ctx* ctx, uint32_t what);
int rt3_regroup_device(rt3_ctx* ctx, uint32_t what, void* stream);
/* Tests only: downloads the group order of one class (what = exactly one RT3_REGROUP_* bit): the primitive index at every position,
 * 0xFFFFFFFF for a pad.  n_positions is set whenever a scene of that class exists; RT3_E_ARG if capacity_words is smaller. */
int rt3_debug_group_order(rt3_ctx* ctx, uint32_t what, uint32_t* out, uint64_t capacity_words, uint32_t* n_positions);

/* ---------------------------------------------------------------------------------------------------
 * Render   (replaces Renderer::render, Renderer.hpp:50)
 * ------------------------------------------------------------------------------------------------- */
/* Mode R, synchronous, host output: out_pixels[w*h] in the reference's word layout
 * (0xFF | B<<8 | G<<16 | R<<24, row 0 = top; SequentialRenderer.cpp:297).  All rows are written; row h-1
 * follows the GLSL twin (raytracer_v3.glsl:193-196) because the CPU loop never writes it. */
int rt3_render(rt3_ctx* ctx, const rt3_camera* cam, uint32_t width, uint32_t height, uint32_t* out_pixels);
/* Mode R, asynchronous on `stream` (a hipStream_t; NULL = the context's own stream), device output buffer of w*h words. */
int rt3_render_device(rt3_ctx* ctx, const rt3_camera* cam, uint32_t width, uint32_t height,
                      void* d_out_pixels, void* stream);

/* Mode X, synchronous, host output of rt3_rows_owned(params)*width words (compact tile rows). */
int rt3_render_path(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, uint32_t* out_pixels);
/* Mode X, asynchronous on `stream` (NULL = the context's own stream), device output. */
int rt3_render_path_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params,
                           void* d_out_pixels, void* stream);

/* Progressive / resumable form (design intent reduce_v1.glsl:28-76 + the SampleStorage of
 * raytracer_v4.glsl:107-111): renders samples [sample_begin, sample_begin + sample_count) of the params->spp samples
 * per pixel and adds them, in sample order, to the per-pixel accumulators the context keeps between calls; the output
 * is the frame resolved over the samples accumulated so far (sum / (sample_begin + sample_count)).  sample_begin == 0
 * starts a new accumulation; otherwise it must equal the number of samples already accumulated for the SAME camera and
 * params (RT3_E_STATE if not).  Any partition of [0, spp) into consecutive calls gives the frame of one
 * rt3_render_path*() call, bit for bit.  rt3_render_path_device(p) == rt3_render_path_range_device(p, 0, p->spp). */
int rt3_render_path_range(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params,
                          uint32_t sample_begin, uint32_t sample_count, uint32_t* out_pixels);
int rt3_render_path_range_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params,
                                 uint32_t sample_begin, uint32_t sample_count, void* d_out_pixels, void* stream);
/* Adaptive sampling: params->spp is a BUDGET; a pixel stops receiving samples once it and its neighbours have converged.
 *   Rounds.  Round 0 renders samples [0, min_spp) of the spp-sample law of rt3_render_path (same jitter strata, same RNG keys) for every owned pixel;
 *     round r >= 1 renders the next min(step_spp, spp - done) samples for the ACTIVE pixels only; it ends when done == spp or no pixel is active.  A
 *     pixel that left never returns, so all active pixels share one count.
 *   A pixel's value is the prefix of its own sample law: sums and squares over samples [0, n) in sample order, resolved as sum / (float)n, gamma
 *     and packing as for rt3_render_path.  A pixel with count n therefore equals, bit for bit, the same pixel of
 *     rt3_render_path_range(cam, params, 0, n).
 *   unconverged(q), owned pixel q with count n, sums S and squares Q; all in f32, every operation rounded on its own, in this order:
 *     m_c = S_c / n;  v_c = Q_c / n - m_c * m_c, v_c = v_c > 0 ? v_c : 0;  e2 = ((v_r + v_g) + v_b) / n;  d = ((m_r + m_g) + m_b) + dark;
 *     lim = threshold * d;  unconverged <=> e2 > lim * lim.
 *   After a round p stays active <=> p was active and some pixel q is unconverged, q owned by this shard, inside the frame, |x_q - x_p| <= 1 and
 *     |framerow_q - framerow_p| <= 1 (p itself is such a q).  Pixels of other shards are ignored: with tile_count > 1 the count map may differ from
 *     the whole frame's along row-block edges; the prefix property holds for every pixel regardless.
 * The squares are always kept: RT3_FLAG_VARIANCE in params->flags changes nothing.  min_spp == spp is exactly rt3_render_path.
 * Outputs, both in compact tile rows as rt3_render_path writes them: the pixels, and (out_counts may be NULL) the samples each pixel received.
 * RT3_E_ARG: a NULL pointer that is not allowed; min_spp outside [2, spp], step_spp == 0, a threshold that is not finite and > 0, a dark that is
 * not finite and >= 0; RT3_FLAG_REFERENCE_PRIMARY; a device pointer that is not 16-byte (pixels) / 4-byte (counts) aligned.  RT3_E_STATE without a
 * scene.
 * The call replaces the context's accumulation with an adaptive one: rt3_accum_resolve* then divides each pixel by its own count (what a denoiser
 * reads); rt3_accum_download and a following rt3_render_path_range with sample_begin != 0 return RT3_E_STATE (no checkpoint form); any later
 * ordinary render starts over.
 * Streams follow the convention above.  The device form is NOT fully asynchronous: it waits for the device once per round, to read back one
 * word, the length of the active list.  rt3_get_stats afterwards: samples = the sum of the counts; ray_casts, launches, trace_ms and the filter
 * counters are summed over the rounds.  In sphere scenes of <= 512 spheres only round 0 traces its primary rays against the strip lists: the
 * active pixels of later rounds are not runs of 64 consecutive pixels, and their primary rays take the matrix filter. */
typedef struct rt3_adaptive_params {   /* 16 bytes */
    uint32_t min_spp;     /* samples every owned pixel gets first; 2 <= min_spp <= params->spp */
    uint32_t step_spp;    /* samples per later round, >= 1 */
    float    threshold;   /* relative standard error of the mean at which a pixel stops; finite, > 0 */
    float    dark;        /* added to the mean r+g+b it is relative to; finite, >= 0 (0.01 is a good default) */
} rt3_adaptive_params;
int rt3_render_path_adaptive(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, const rt3_adaptive_params* adaptive,
                             uint32_t* out_pixels, uint32_t* out_counts);
int rt3_render_path_adaptive_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, const rt3_adaptive_params* adaptive,
                                    void* d_out_pixels, void* d_out_counts, void* stream);
/* Checkpoint / resume of that accumulation.  Download: sum (and, when the accumulation runs with
 * RT3_FLAG_VARIANCE and sum_sq != NULL, the sums of squares) as 4 floats per owned pixel (r, g, b, 0), compact tile
 * rows as rt3_render_path writes them; *samples_done = samples accumulated.  Upload: restores such a state for
 * (cam, params) — possibly into another context or process — so that the next rt3_render_path_range() call continues
 * at sample_begin == samples_done.  sum_sq may be NULL when params->flags lacks RT3_FLAG_VARIANCE. */
int rt3_accum_download(rt3_ctx* ctx, float* sum_rgba, float* sum_sq_rgba, uint32_t* samples_done);
int rt3_accum_upload(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params,
                     const float* sum_rgba, const float* sum_sq_rgba, uint32_t samples_done);

/* Multi-GPU gather of final pixels without the host ("hipMemcpyPeerAsync into rank 0's buffer at
 * the right offsets, no de-interleave needed"; tiling intent BlockInfo, raytracer_v4.glsl:70-79).  d_tile holds the
 * compact rows of the shard described by shard_params (as rt3_render_path_device wrote them) on the device of
 * `shard`; they are copied to their interleaved positions inside the full frame d_frame (width*height words) on the
 * device of `root` — one strided 2-D device-to-device copy (peer-to-peer over xGMI when the two contexts sit on
 * different GPUs; peer access is enabled on first use) plus one 1-D copy when the last row block is ragged.  The
 * copies are issued on `stream`, which must be a stream of the SHARD's device (NULL = the shard context's own stream),
 * so that they run behind the shard's resolve kernel.  root == shard is allowed (single GPU). */
int rt3_gather_rows(rt3_ctx* root, void* d_frame, rt3_ctx* shard, const void* d_tile,
                    const rt3_params* shard_params, void* stream);
/* What rt3_gather_rows copies, as plain arithmetic (no device needed: a host can check or re-use it, tests/test_gather_plan.py): at most two
 * strided copies of `rows` pieces of `row_bytes` bytes each, piece i from tile byte src_offset + i * src_pitch to frame byte dst_offset +
 * i * dst_pitch.  Returns the number of copies written to out[0..1] (0: the shard owns no row) or RT3_E_ARG. */
typedef struct rt3_gather_copy {
    uint64_t dst_offset, src_offset;   /* bytes into the frame / into the compact tile */
    uint64_t dst_pitch, src_pitch;     /* bytes between consecutive pieces */
    uint64_t row_bytes;                /* bytes per piece (a whole row block of the shard, or the ragged last one) */
    uint32_t rows;                     /* pieces */
} rt3_gather_copy;
int rt3_gather_plan(const rt3_params* shard_params, rt3_gather_copy out[2]);
/* The context's own stream (a hipStream_t) and a wait for it — what a multi-device host needs around rt3_gather_rows. */
void* rt3_stream(rt3_ctx* ctx);
int   rt3_synchronize(rt3_ctx* ctx);
/* Device frame buffer helpers for hosts that have no other HIP binding: allocate / free n_words uint32 on the
 * context's device, and copy such a buffer to the host (synchronous, after everything queued on the ctx stream). */
void* rt3_device_alloc_words(rt3_ctx* ctx, uint64_t n_words);
void  rt3_device_free(rt3_ctx* ctx, void* d_ptr);
int   rt3_device_read_words(rt3_ctx* ctx, const void* d_ptr, uint64_t n_words, uint32_t* out);

/* Rows of the frame owned by shard tile_index (see rt3_params), and the frame row of local row i. */
uint32_t rt3_rows_owned(const rt3_params* params);
uint32_t rt3_row_of_local(const rt3_params* params, uint32_t local_row);

/* Waits for the last asynchronous render and fills `out` (may be called after the synchronous forms too). */
int rt3_get_stats(rt3_ctx* ctx, rt3_stats* out);

/* ---------------------------------------------------------------------------------------------------
 * Batched ray queries   (the Mode-X nearest-hit engine for rays the caller makes)
 * ------------------------------------------------------------------------------------------------- */
/* One ray: 32 bytes, two 16-byte halves (origin, t_max | direction, pad).  The direction must be a unit vector (below). */
typedef struct rt3_ray {
    float    origin[3];
    float    t_max;              /* hits count only for t < t_max; +inf: no limit */
    float    direction[3];
    uint32_t _pad;
} rt3_ray;
/* One result: 16 bytes. */
typedef struct rt3_hit {
    float    t;                  /* in units of the direction as given; +inf on a miss, NaN for an invalid ray */
    uint32_t kind;               /* RT3_HIT_* */
    uint32_t index;              /* the primitive's position in the caller's arrays (rt3_set_mesh / rt3_mesh_commit face order,
                                    rt3_set_spheres order); 0xFFFFFFFF on a miss or an invalid ray */
    uint32_t _pad;               /* 0 */
} rt3_hit;
#define RT3_HIT_NONE     0u
#define RT3_HIT_FACE     1u
#define RT3_HIT_SPHERE   2u
#define RT3_HIT_INVALID  3u
/* rt3_intersect*: for each ray, against the scene on the context (faces and spheres together), exactly what the Mode-X nearest-hit rule
 * returns when its running best starts at t_max instead of +inf: faces first, then spheres; a face is accepted for t_min <= t, a sphere for
 * t > t_min with the far-root rule; a hit counts only with t < t_max (a hit at exactly t_max is a miss); on equal t the earlier primitive
 * wins, faces before spheres.  Equivalently: the nearest hit with t_max = +inf, kept only if t < t_max.  A miss is {+inf, RT3_HIT_NONE,
 * 0xFFFFFFFF, 0}.
 * rt3_occluded*: one uint32 per ray, 1 where such a hit exists, 0 where none does (exactly kind != RT3_HIT_NONE of rt3_intersect*),
 * 0xFFFFFFFF for an invalid ray.
 * A ray is INVALID when its origin or direction is not finite, when |d.d - 1| > 2^-20 (d.d as the fused chain fma(dz, dz, fma(dy, dy,
 * dx * dx))), when t_max is NaN or when t_max <= t_min: it gets RT3_HIT_INVALID {NaN, 3, 0xFFFFFFFF, 0}, is not traced, not counted, and
 * changes nothing for the other rays.
 * Arguments: t_min finite and >= 0 (as in rt3_params); n <= 2^30; n == 0 does nothing and returns 0; device pointers 16-byte aligned
 * (4-byte for the occlusion words); RT3_E_ARG otherwise; RT3_E_STATE without a scene.
 * Streams follow the convention above: a query waits for the event the previous render or query recorded and records its own, so a
 * later render, rt3_accum_download or query on the same context is ordered after it.  A query does not touch the accumulation of a
 * progressive render (rt3_render_path_range continues bit-exactly across it).  rt3_get_stats afterwards: ray_casts = valid rays,
 * prim_tests = ray_casts * (n_spheres + n_faces), samples = 0, launches, trace_ms and the filter counters.
 * Kernel choice is Mode X's: k_trace_mfma32 for <= 512 spheres, the resident / tiled three-level form while the rows fit in LDS,
 * k_trace_levels beyond, k_trace_brute under rt3_debug_force_brute / RT3_BRUTE; RT3_LEVELS, RT3_NO_RESIDENT, RT3_OLD_GROUPS and
 * RT3_FORCE_TILED act as for renders.  Queries ignore the switches of forms they have none of: RT3_NO_MFMA (VALU k_trace), RT3_MFMA_K64,
 * the flat filter (rt3_debug_force_flat_filter / RT3_NO_GROUPS) and RT3_FLAG_REFERENCE_PRIMARY. */
/* Host arrays, synchronous. */
int rt3_intersect(rt3_ctx* ctx, const rt3_ray* rays, uint32_t n, float t_min, rt3_hit* hits);
int rt3_occluded(rt3_ctx* ctx, const rt3_ray* rays, uint32_t n, float t_min, uint32_t* out);
/* Device arrays (n rt3_ray in, n rt3_hit | n uint32 out), asynchronous on `stream` (NULL = the context's own stream). */
int rt3_intersect_device(rt3_ctx* ctx, const void* d_rays, uint32_t n, float t_min, void* d_hits, void* stream);
int rt3_occluded_device(rt3_ctx* ctx, const void* d_rays, uint32_t n, float t_min, void* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Camera rays, first-hit AOVs and the linear frame   (what a denoiser or compositor reads)
 * ------------------------------------------------------------------------------------------------- */
/* One pixel's first-hit AOVs: 48 bytes, three 16-byte halves.  Averages over the pixel's spp primary rays (summed in sample order, then
 * divided by spp), except depth (over the samples that hit) and kind / index (sample 0's hit). */
typedef struct rt3_aov {
    float    albedo[3];          /* FLAT / LAMBERT / METAL: the material's rgb; DIELECTRIC: (1, 1, 1); miss: sky(d), or 0 under
                                    RT3_FLAG_BLACK_BACKGROUND (the render's miss radiance); invalid ray: 0 */
    float    coverage;           /* samples that hit / spp */
    float    normal[3];          /* the shading normal of the hit, flipped to face the ray (d.n < 0); 0 on a miss */
    float    depth;              /* mean t of the samples that hit (distance from the lens point); +inf when none did */
    uint32_t kind, index;        /* sample 0's hit, as in rt3_hit (RT3_HIT_INVALID if its ray was invalid) */
    uint32_t _pad[2];            /* 0 */
} rt3_aov;
/* Mode X's primary rays as rt3_ray records: for samples [sample_begin, sample_begin + sample_count) of params->spp, record
 * (s - sample_begin) * npix + pix, npix = rt3_rows_owned(params) * width (the render's item order, compact tile rows).  Bit for bit the ray
 * that ray cast 0 of rt3_render_path* traces (jitter, strata, thin lens), unit direction, t_max = +inf, _pad = 0.  No scene needed.
 * RT3_FLAG_REFERENCE_PRIMARY is refused (RT3_E_ARG): its directions are not unit vectors.  Owned pixels x samples <= 2^31 - 2^16. */
int rt3_camera_rays(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, uint32_t sample_begin, uint32_t sample_count,
                    rt3_ray* out_rays);
int rt3_camera_rays_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, uint32_t sample_begin, uint32_t sample_count,
                           void* d_out_rays, void* stream);
/* First-hit AOVs of every owned pixel (compact tile rows, as rt3_render_path writes them): the camera rays above, each traced with
 * rt3_intersect's rule (t_min from params, t_max = +inf), reduced per pixel as rt3_aov describes.  AOVs are linear: RT3_FLAG_GAMMA2 does
 * not apply; max_depth is not used; RT3_FLAG_REFERENCE_PRIMARY is refused (RT3_E_ARG).  The call never touches the accumulation of a
 * progressive render.  Streams as for queries.  rt3_get_stats afterwards: ray_casts = valid primary rays, samples = pixels x spp,
 * launches / trace_ms / filter counters summed over the sample batches (sized by rt3_set_sample_storage_cap at 48 bytes per pixel and
 * sample).  RT3_E_STATE without a scene; device pointers 16-byte aligned. */
int rt3_render_aov(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, rt3_aov* out_aov);
int rt3_render_aov_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, void* d_out_aov, void* stream);
/* The accumulation as a linear float frame: (sum.r / n, sum.g / n, sum.b / n, 0) per owned pixel, n = samples accumulated — the division
 * the RGBA8 resolve does, before any gamma (packing it gives the frame of a render without RT3_FLAG_GAMMA2).  Compact tile rows of the
 * last rt3_render_path* / rt3_accum_upload; RT3_E_STATE without an accumulation; d_out_rgba 16-byte aligned. */
int rt3_accum_resolve(rt3_ctx* ctx, float* out_rgba);
int rt3_accum_resolve_device(rt3_ctx* ctx, void* d_out_rgba, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Denoiser   (the spatial part of SVGF: an edge-avoiding a-trous filter guided by the AOVs)
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt3_denoise_params {      /* 16 bytes */
    uint32_t iterations;                 /* a-trous passes N, 1..8 (steps 1, 2, 4, ...); default 5 */
    uint32_t normal_power;               /* exponent P of the normal weight, a power of two in 1..1024; default 128 */
    float    sigma_luminance;            /* sigma_l, finite and > 0; default 4 */
    float    sigma_depth;                /* sigma_z, finite and > 0; default 1 */
} rt3_denoise_params;
/* One whole frame of width x height pixels, row 0 on top: colour_rgba is (r, g, b, ignored) per pixel as rt3_accum_resolve writes it,
 * aov one rt3_aov per pixel as rt3_render_aov writes it; out_rgba gets (r, g, b, 0) per pixel and must not overlap either input.  No scene
 * is needed.  The call never touches the accumulation of a progressive render and leaves rt3_get_stats as it was.  Streams as for
 * queries; the host form is synchronous.  RT3_E_ARG for a NULL pointer, width or height 0, width x height > 2^26, a parameter outside
 * the ranges above, a device pointer that is not 16-byte aligned, or a device output that overlaps an input.  Scratch (52 bytes per
 * pixel) belongs to the context. */
int rt3_denoise(rt3_ctx* ctx, uint32_t width, uint32_t height, const float* colour_rgba, const rt3_aov* aov,
                const rt3_denoise_params* p, float* out_rgba);
int rt3_denoise_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const void* d_colour_rgba, const void* d_aov,
                       const rt3_denoise_params* p, void* d_out_rgba, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Temporal denoiser   (SVGF's temporal half: reprojected history, blended, temporal variance)
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt3_history {             /* 48 bytes, one per pixel, row 0 on top */
    float colour[3];                     /* demodulated colour after the first a-trous pass */
    float length;                        /* frames integrated (1 = no usable history) */
    float moments[2];                    /* integrated L and L*L */
    float depth;                         /* this frame's depth (+inf = miss) */
    float _pad0;
    float normal[3];                     /* this frame's normal (the AOV's) */
    float _pad1;
} rt3_history;
typedef struct rt3_temporal_params {     /* 32 bytes */
    rt3_denoise_params spatial;          /* the a-trous passes, as for rt3_denoise */
    float alpha;                         /* blend floor of the colour, in (0, 1]; default 0.2 */
    float moments_alpha;                 /* blend floor of the moments, in (0, 1]; default 0.2 */
    float depth_tolerance;               /* finite and > 0; default 2 */
    float normal_tolerance;              /* in [-1, 1]; default 0.9 */
} rt3_temporal_params;
/* One frame of a sequence: colour_rgba and aov as for rt3_denoise, cam the camera they were rendered with; prev_cam and prev_history the
 * previous frame's camera and the history the previous call wrote (both NULL for the first frame of a sequence, or both non-NULL).  Writes
 * the denoised frame to out_rgba ((r, g, b, 0) per pixel) and the history for the next frame to out_history.  The caller owns the history:
 * the context keeps no state between calls.  The call never touches the accumulation and leaves rt3_get_stats as it was; streams as for
 * queries; the host form is synchronous.  RT3_E_ARG for a NULL pointer that is not allowed, width or height below 2, width x height > 2^26,
 * a parameter outside the ranges above, a non-finite camera field, a degenerate camera (horizontal x vertical = 0, or an image plane through
 * its origin), a device pointer that is not 16-byte aligned, or an output that overlaps an input or the other output (prev_history and
 * out_history are two buffers, used ping-pong). */
int rt3_denoise_temporal(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_camera* cam, const float* colour_rgba, const rt3_aov* aov,
                         const rt3_camera* prev_cam, const rt3_history* prev_history, const rt3_temporal_params* p,
                         float* out_rgba, rt3_history* out_history);
int rt3_denoise_temporal_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_camera* cam, const void* d_colour_rgba,
                                const void* d_aov, const rt3_camera* prev_cam, const void* d_prev_history, const rt3_temporal_params* p,
                                void* d_out_rgba, void* d_out_history, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Motion plane   (per-pixel world-space motion of the scene's primitives for the temporal denoiser)
 * ------------------------------------------------------------------------------------------------- */
/* One float4 per pixel of a whole frame, row 0 on top: (mx, my, mz, moved).  m is the world-space displacement from the point the pixel
 * shows now to where that surface point was in the previous frame; moved is 1.0f or 0.0f ((0, 0, 0, 0): a miss, a primitive that is byte
 * for byte where it was, a class without a previous array, a degenerate face).  The scene on the context is THIS frame's, the one aov was
 * rendered from with cam.  The previous frame's geometry comes from the caller, in the caller's order and layout: 4 floats per sphere as
 * rt3_set_spheres takes them, vec4 vertices as rt3_set_mesh takes them (same topology: the face list is the context's).  Either pointer
 * may be NULL with a count of 0: that class of primitive did not move.  A non-NULL array's count must equal the context's (the sphere
 * count; the vertex count of the merged entity buffers that rt3_mesh_download returns), else RT3_E_ARG.  RT3_E_STATE when a non-NULL
 * array names a class the context has no committed scene of, or when the merged entity buffers were changed after the last commit
 * (rt3_mesh_begin / rt3_mesh_put / rt3_mesh_sphere without an rt3_mesh_commit).  The previous arrays' values are not validated: a non-finite m
 * is written as it comes and costs that pixel its history in rt3_denoise_temporal_motion.  Spheres move by translation and uniform
 * scaling about the centre; a face carries the point's barycentric coordinates to its previous vertices, whatever moved them.
 * The call never touches the accumulation and leaves rt3_get_stats as it was; streams as for queries; the host form is synchronous.
 * RT3_E_ARG also for a NULL cam / aov / out_motion, width or height below 2, width x height > 2^26, a camera rt3_denoise_temporal would
 * refuse, a device pointer that is not 16-byte aligned, or an output that overlaps an input. */
int rt3_motion(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_camera* cam, const rt3_aov* aov,
               const float* prev_center_radius, uint32_t n_prev_spheres,
               const float* prev_vertices_xyzw, uint32_t n_prev_vertices, float* out_motion);
int rt3_motion_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_camera* cam, const void* d_aov,
                      const void* d_prev_center_radius, uint32_t n_prev_spheres,
                      const void* d_prev_vertices_xyzw, uint32_t n_prev_vertices, void* d_out_motion, void* stream);
/* rt3_denoise_temporal with one more input: motion, the plane rt3_motion wrote for this frame (width x height float4), or NULL.  A pixel
 * that hit and whose moved is not 0 is reprojected from its previous position (the world point plus m) and is always projected into the
 * previous camera, also when *prev_cam equals *cam; every other pixel comes out bit for bit as from rt3_denoise_temporal, which is this
 * call with motion == NULL.  motion takes part in the alignment and overlap checks; without a previous frame it is not read. */
int rt3_denoise_temporal_motion(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_camera* cam, const float* colour_rgba,
                                const rt3_aov* aov, const rt3_camera* prev_cam, const rt3_history* prev_history, const float* motion,
                                const rt3_temporal_params* p, float* out_rgba, rt3_history* out_history);
int rt3_denoise_temporal_motion_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_camera* cam, const void* d_colour_rgba,
                                       const void* d_aov, const rt3_camera* prev_cam, const void* d_prev_history, const void* d_motion,
                                       const rt3_temporal_params* p, void* d_out_rgba, void* d_out_history, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Radiance along caller-supplied rays   (the Mode-X path loop for rays the caller makes)
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt3_radiance_params {   /* 24 bytes */
    uint32_t max_depth;      /* ray casts per path, >= 1, as rt3_params */
    uint32_t seed;
    uint32_t flags;          /* RT3_FLAG_BLACK_BACKGROUND, RT3_FLAG_ENV_SAMPLING (not both), RT3_FLAG_LIGHT_SAMPLING (not with ENV_SAMPLING); any other bit: RT3_E_ARG */
    uint32_t sample_begin;   /* first sample index */
    uint32_t sample_count;   /* samples per ray, >= 1; sample_begin + sample_count <= 2^31 */
    float    t_min;          /* finite, >= 0 */
} rt3_radiance_params;
/* Path law.  Ray i has key k_i = keys ? keys[i] : i.  For each sample s in [sample_begin, sample_begin + sample_count), one Mode-X path is
 * traced: it starts at the ray's origin and direction with throughput 1, depth 0 and base = hash2(k_i, hash2(s, seed)); the rest is the path
 * loop of DESIGN.md 4 with nothing changed: the nearest-hit rule, the materials, the RNG counters 1 + 8 (depth + 1) + k, max_depth, t_min, and
 * the sky or black on a miss.  L(i, s) is the radiance record a render would store for that sample.
 * Output.  16 bytes per ray: (S.r / n_s, S.g / n_s, S.b / n_s, 0), S the f32 sum of L(i, s) in sample order starting from +0,
 * n_s = (float)sample_count, each operation rounded on its own (the render's accumulation followed by rt3_accum_resolve's division).
 * Defining property.  Take any whole-frame rt3_params P, a pixel (x, y) and a sample s.  Query that (pixel, sample)'s ray from
 * rt3_camera_rays(cam, P, s, 1) with key y * P.width + x, seed = P.seed, max_depth = P.max_depth, t_min = P.t_min, the BLACK_BACKGROUND bit
 * of P.flags, sample_begin = s and sample_count = 1: the result is, bit for bit, the radiance rt3_render_path_range(cam, P, s, 1)
 * accumulates for that pixel.  For a shard, the key is the frame pixel index and the ray is the shard's record.
 * Valid rays.  rt3_intersect's rule, plus one more: t_max must be +inf.  A finite t_max is reserved and is not silently ignored.  An
 * invalid ray gets (NaN, NaN, NaN, 0); it is not traced, is not counted in ray_casts, and changes nothing for any other ray.
 * Arguments.  n <= 2^27 (keys make it seamless for a caller to split a larger batch); n == 0 returns 0 and does nothing; keys may be NULL;
 * device pointers are 16-byte aligned (rays, output) and 4-byte aligned (keys); the output must not overlap the inputs; RT3_E_ARG and
 * RT3_E_STATE are returned as for queries.
 * Context state.  The call never touches the accumulation of a progressive or adaptive render: rt3_render_path_range continues bit-exactly
 * across it.  Streams and the event chain work as for queries.  The device form never waits for the device and allocates only when the
 * sample storage must grow.  Samples are batched by rt3_set_sample_storage_cap at 12 B per (ray, sample); the result does not depend on the
 * batching.
 * rt3_get_stats afterwards: samples = n * sample_count; ray_casts, prim_tests, launches, trace_ms and the filter counters are summed over
 * the batches.
 * Kernel choice is that of a query on the same scene (the RAYS form of that kernel); the switches queries ignore are ignored here too. */
/* Host arrays, synchronous. */
int rt3_radiance(rt3_ctx* ctx, const rt3_ray* rays, const uint32_t* keys, uint32_t n, const rt3_radiance_params* p, float* out_rgba);
/* Device arrays (n rt3_ray and, or NULL, n uint32 in; n float4 out), asynchronous on `stream` (NULL = the context's own stream). */
int rt3_radiance_device(rt3_ctx* ctx, const void* d_rays, const void* d_keys, uint32_t n, const rt3_radiance_params* p, void* d_out_rgba,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Lens models  (DESIGN.md 4.23, 5.2r): equirectangular, fisheye, orthographic and cube frames, generated and rendered on the device
 * ------------------------------------------------------------------------------------------------- */
#define RT3_LENS_EQUIRECT 1u   /* the whole sphere; column W/2 looks along `forward`, row 0 is `up` */
#define RT3_LENS_FISHEYE  2u   /* equidistant: angle from `forward` proportional to the distance from the image centre */
#define RT3_LENS_ORTHO    3u   /* parallel rays along `forward` from a window of 2 half_extent[0] x 2 half_extent[1] */
#define RT3_LENS_CUBE     4u   /* W = N, H = 6 N: the six faces of rt3_set_environment's layout, stacked +X -X +Y -Y +Z -Z */
typedef struct rt3_lens {      /* 80 bytes */
    uint32_t model;
    float    half_fov_turns;   /* FISHEYE: half the field of view across the shorter image side, in turns (degrees / 720); in (0, 0.5] */
    float    half_extent[2];   /* ORTHO: finite, > 0 */
    float    origin[3];  float _pad0;
    float    right[3];   float _pad1;   /* an orthonormal, right-handed frame: right x up = -forward ... */
    float    up[3];      float _pad2;
    float    forward[3]; float _pad3;   /* ... the local axes are (X, Y, Z) = (right, up, -forward) */
} rt3_lens;
/* Fields of other models are ignored.  A lens is refused (RT3_E_ARG) for: an unknown model; a non-finite origin or axis; an axis whose d.d, taken
 * as the fused chain of the ray validity rule (fma(dz, dz, fma(dy, dy, dx * dx))), is further than 2^-20 from 1; two axes whose dot product (the same
 * chain) exceeds 2^-20 in magnitude; half_fov_turns outside (0, 0.5] for FISHEYE; a half_extent that is not finite and > 0 for ORTHO;
 * height != 6 * width for CUBE.
 * The ray law.  Every operation is an IEEE f32 operation rounded on its own, nothing fused except inside sincos2pi (the (cos, sin)(2 pi u) of the
 * path law's scatter).  For frame pixel (x, y), row 0 on top, and sample s of params->spp, with W = width, H = height:
 *     base = hash2(y * W + x, hash2(s, seed));  (jx, jy) = exactly the jitter of rt3_render_path's ray cast 0: counters 1 and 2 of base, the same
 *     strata (spp a perfect square > 1), none at spp == 1;
 *     px = ((float)x + 0.5f) + jx;  py = ((float)y + 0.5f) - jy;  a = px / (float)W;  b = py / (float)H.
 * The local direction l:
 *     EQUIRECT  (ct, st) = sincos2pi(b * 0.5f);  (cp, sp) = sincos2pi(a);  l = (-sp * st, ct, -cp * st)
 *     FISHEYE   m = 0.5f * (float)min(W, H);  nx = (px - 0.5f * (float)W) / m;  ny = (0.5f * (float)H - py) / m;  r = sqrtf(nx * nx + ny * ny);
 *               tau = fminf(r * half_fov_turns, 0.5f);  (c, sn) = sincos2pi(tau);  k = r > 0 ? sn / r : 0;  l = (nx * k, ny * k, c).
 *               Pixels outside the image circle continue the mapping up to the pole behind the lens: no ray is invalid.
 *     ORTHO     nx = a * 2.0f - 1.0f;  ny = 1.0f - b * 2.0f;  e1 = nx * half_extent[0];  e2 = ny * half_extent[1];
 *               the origin per component is (origin_c + e1 * right_c) + e2 * up_c;  l = (0, 0, 1)
 *     CUBE      N = W;  f = y / N;  j = y - f * N;  sc = a * 2.0f - 1.0f;  tc = ((((float)j + 0.5f) - jy) / (float)N) * 2.0f - 1.0f;
 *               (vx, vy, vz) = the row of face f in the table of "Environment map: sampling" below (+X (1, -t, -s) ...) with s = sc, t = tc;
 *               l = (vx, vy, -vz): under the identity frame (right +X, up +Y, forward -Z) texel (f, j, i)'s ray is the direction the lookup law
 *               maps back to that texel, so the frame, reshaped to (6, N, N, 4), is a map of the scene's surroundings.
 * World direction per component: w_c = (l.x * right_c + l.y * up_c) + l.z * forward_c; then d = w * (1.0f / sqrtf(w.x * w.x + w.y * w.y + w.z * w.z)).
 * The record is (origin, +inf | d, 0).  Every generated ray passes the validity rule of queries and radiance.
 * rt3_lens_rays*: the twin of rt3_camera_rays*: for samples [sample_begin, sample_begin + sample_count) of params->spp, record
 * (s - sample_begin) * npix + pix over the owned pixels (compact tile rows).  No scene needed; max_depth, t_min, lens_radius and flags are checked as
 * rt3_params always is and otherwise not used.  Owned pixels x samples <= 2^31 - 2^16.  Unlike the camera's frames a lens frame may be one pixel wide
 * or high (width, height >= 1: a cube of N = 1).
 * rt3_render_lens*: linear float4 per owned pixel.  Defining property: the value of owned pixel pix (frame pixel index q = y * W + x) is
 * (S.r / n, S.g / n, S.b / n, 0), n = (float)sample_count, S the f32 sum from +0, in sample order, over s in [sample_begin, sample_begin +
 * sample_count), of what rt3_radiance returns for record (s, pix) of rt3_lens_rays under keys = q, seed / max_depth / t_min from params,
 * sample_begin = s, sample_count = 1 and the bits RT3_FLAG_BLACK_BACKGROUND | RT3_FLAG_ENV_SAMPLING | RT3_FLAG_LIGHT_SAMPLING of params->flags.  Every
 * rule of those flags carries over (the map, the sampling tables, their mutual refusals).  RT3_FLAG_GAMMA2 is accepted and ignored: the output is
 * linear, rt3_display* packs it.  RT3_FLAG_REFERENCE_PRIMARY, RT3_FLAG_VARIANCE, a lens_radius that is not 0 and unknown bits are refused
 * (RT3_E_ARG).  Owned pixels <= 2^27.  RT3_E_STATE without a scene.  Tiles as in rt3_params: a shard writes its compact rows, which equal the same
 * rows of the whole frame bit for bit.
 * rt3_render_lens_aov*: the twin of rt3_render_aov*: the lens rays of all spp samples, each traced with rt3_intersect's rule (t_min from params,
 * t_max = +inf), reduced per pixel exactly as rt3_aov describes; the miss albedo is the sky's or the map's as there.  max_depth is not used;
 * RT3_FLAG_REFERENCE_PRIMARY and a lens_radius that is not 0 are refused.
 * Context.  As rt3_radiance*: the accumulation of a progressive or adaptive render is never touched; streams and the event chain work as for
 * queries; rt3_get_stats afterwards reports samples = owned pixels x sample_count (x spp for the AOVs) with casts, launches, times and filter counters
 * summed — a render traces every sample with a launch of its own (the Rays form maps an item to ray item % npix, and here each sample has its own
 * rays); scratch belongs to the context (32 B per ray of a batch, plus 4 B per pixel of keys for a shard); batches are sized by
 * rt3_set_sample_storage_cap at 44 B per (pixel, sample) and the result does not depend on them; the device forms never wait for the device.  Device
 * pointers are 16-byte aligned.
 * Out of scope: thin-lens depth of field for these models and the adaptive render.  (The temporal denoiser and the motion plane of a lens frame:
 * "Lens sequences", below.) */
/* Host: origin = from and the frame that looks from `from` towards `at` with `vup` up (forward = unit(at - from), right = unit(forward x vup),
 * up = right x forward); sets model, leaves half_fov_turns and half_extent, zeroes the pads. */
void rt3_lens_look_at(rt3_lens* lens, uint32_t model, const float from[3], const float at[3], const float vup[3]);
int  rt3_lens_rays(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, uint32_t sample_begin, uint32_t sample_count, rt3_ray* out_rays);
int  rt3_lens_rays_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, uint32_t sample_begin, uint32_t sample_count,
                          void* d_out_rays, void* stream);
int  rt3_render_lens(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, uint32_t sample_begin, uint32_t sample_count, float* out_rgba);
int  rt3_render_lens_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, uint32_t sample_begin, uint32_t sample_count,
                            void* d_out_rgba, void* stream);
int  rt3_render_lens_aov(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, rt3_aov* out_aov);
int  rt3_render_lens_aov_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, void* d_out_aov, void* stream);
/* Host only, no device and no context: the law above in C for one (pixel, sample) of the whole frame.  RT3_E_ARG for a NULL pointer, a lens the
 * entry points refuse, width or height 0, spp 0, x >= width, y >= height or s >= spp.  tests/lens_ref.py restates it bit for bit. */
int  rt3_debug_lens_ray(const rt3_lens* lens, const rt3_params* params, uint32_t x, uint32_t y, uint32_t s, rt3_ray* out);

/* ---------------------------------------------------------------------------------------------------
 * Specular-chain AOVs  (DESIGN.md 4.27, 5.2v): guides taken at the first rough surface behind mirrors and glass
 * ------------------------------------------------------------------------------------------------- */
/* rt3_render_aov_specular* / rt3_render_lens_aov_specular* are rt3_render_aov* / rt3_render_lens_aov* with every sample's ray followed through ideal
 * mirrors and glass.  Per sample, from the primary ray, throughput T = (1, 1, 1), length L = 0, bounces used b = 0:
 *   trace with rt3_intersect's rule (t_min from params, t_max = +inf); an invalid primary ray is what it is there (albedo 0, no hit).
 *   miss: the chain ends, albedo = T x the miss colour of rt3_render_aov (sky, map, or 0 under RT3_FLAG_BLACK_BACKGROUND), one rounded multiply per
 *     channel; normal and L stay those of the last surface the chain hit (a primary miss: 0 and nothing).
 *   hit: point, normal, material record and texture modulation as rt3_render_aov takes them; L = L + t; front = d.n < 0 before the normal is flipped
 *     to face the ray.  The chain FOLLOWS when b < max_bounces and the material is RT3_MAT_METAL with param <= max_fuzz, or RT3_MAT_DIELECTRIC; else it
 *     ENDS here: albedo = T x rgb (a dielectric: T x 1), normal = this normal.
 *     metal: k = 2 (d.n); m = fma(-k, n, d); r = m * (1 / sqrt(m.m)); if !(r.n > 0) the chain ends here (the render's "absorbed"), else T = T x rgb
 *       and the next direction is r * (1 / sqrt(r.r)).  The fuzz is ignored: a followed metal is an ideal mirror.
 *     dielectric: ri = front ? 1 / ior : ior; c = min(-(d.n), 1); s = sqrt(max(fma(-c, c, 1), 0)); if ri s > 1 the direction is m (total internal
 *       reflection), else e = fma(c, n, d) * ri, q = -sqrt(|1 - e.e|), direction fma(q, n, e); either is scaled by 1 / sqrt(of its own dot).  The chain
 *       refracts whenever it can (no Fresnel choice); T is unchanged.
 *     the next ray starts at the hit point with t_max = +inf, b = b + 1; were it INVALID under rt3_intersect's rule, the chain ends at this surface.
 *   (a.b is the fused chain fma(az, bz, fma(ay, by, ax * bx)) throughout.)
 * Per pixel the sums are rt3_render_aov's, in sample order: albedo and normal over all samples, L over the samples whose PRIMARY ray hit, coverage =
 * those samples / spp (geometric); kind / index stay sample 0's FIRST hit, so an id mask still names the object on screen.  The output is an ordinary
 * rt3_aov: albedo is what demodulation should divide by, normal the end surface's normal, depth the path length to it (the "virtual depth").
 * max_bounces = 0 is rt3_render_aov* / rt3_render_lens_aov* byte for byte.
 * Checks, streams, the event chain, shards and the refusal of RT3_FLAG_REFERENCE_PRIMARY are those of the first-hit twins; additionally RT3_E_ARG, with
 * the context's state untouched, for chain == NULL, max_bounces > 16, a max_fuzz that is NaN, negative or infinite, flags != 0 and _pad != 0.
 * rt3_get_stats afterwards: ray_casts = valid rays traced over all bounces, samples = pixels x spp, launches / trace_ms summed over the at most
 * max_bounces + 1 queries of each sample batch (batches sized by rt3_set_sample_storage_cap at 96 bytes per pixel and sample; the result does not depend
 * on them).  The device forms are ordered on `stream` like their twins but wait for it once per bounce: one word, the chains still running, is
 * read back and the loop stops at 0.  The temporal denoisers and rt3_motion* rebuild the first-hit point from depth: give them first-hit AOVs, not
 * these. */
typedef struct rt3_aov_chain_params {   /* 16 bytes */
    uint32_t max_bounces;   /* 0..16; 0: rt3_render_aov exactly */
    float    max_fuzz;      /* finite, >= 0: metals with param <= max_fuzz are followed (as ideal mirrors) */
    uint32_t flags;         /* 0 */
    uint32_t _pad;          /* 0 */
} rt3_aov_chain_params;
/* RT3_CHECK_RESULT: the compiler warns where the caller drops the return code (a refused chain struct leaves out_aov unwritten). */
#if defined(__GNUC__) || defined(__clang__)
#define RT3_CHECK_RESULT __attribute__((warn_unused_result))
#else
#define RT3_CHECK_RESULT
#endif
int  rt3_render_aov_specular(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, const rt3_aov_chain_params* chain, rt3_aov* out_aov)
     RT3_CHECK_RESULT;
int  rt3_render_aov_specular_device(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* params, const rt3_aov_chain_params* chain,
                                    void* d_out_aov, void* stream) RT3_CHECK_RESULT;
int  rt3_render_lens_aov_specular(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, const rt3_aov_chain_params* chain, rt3_aov* out_aov)
     RT3_CHECK_RESULT;
int  rt3_render_lens_aov_specular_device(rt3_ctx* ctx, const rt3_lens* lens, const rt3_params* params, const rt3_aov_chain_params* chain,
                                         void* d_out_aov, void* stream) RT3_CHECK_RESULT;
/* Host only, no device and no context; for the tests: one hit of the law above in C.  d: the ray's unit direction, p: the hit point, n: the surface's
 * normal before the flip, mat_kind / mat: the material's kind and DEVICE record (metal: rgb, fuzz; dielectric: 1 / ior, r0, r0', ior — only [0] and
 * [3] are read), T: the throughput, bounces_used: b.  Writes *follow (1: the chain goes on), out_rgb (follow: the new throughput; else the end's albedo),
 * out_normal (flipped to face the ray) and out_direction (follow: the next unit direction; else 0).  RT3_E_ARG for a NULL pointer or chain params the
 * entry points refuse.  tests/aov_chain_ref.py restates it bit for bit. */
int  rt3_debug_aov_bounce(const float d[3], const float p[3], const float n[3], uint32_t mat_kind, const float mat[4], const float T[3],
                          uint32_t bounces_used, const rt3_aov_chain_params* chain, float out_rgb[3], float out_normal[3], float out_direction[3],
                          uint32_t* follow);

/* ---------------------------------------------------------------------------------------------------
 * Lens sequences  (DESIGN.md 4.24, 5.2s): the temporal denoiser and the motion plane for frames rendered through a lens
 * ------------------------------------------------------------------------------------------------- */
/* rt3_denoise_temporal_optic* is rt3_denoise_temporal_motion* and rt3_motion_optic* is rt3_motion* with a lens where those take a camera: the frame is
 * the whole W x H frame of rt3_render_lens* / rt3_render_lens_aov* for `lens`, prev_lens the lens of the previous frame (NULL with prev_history for the
 * first frame).  Everything that does not involve the view is unchanged: the records, the parameters, the consistency tests, the blend, the variance,
 * the passes, the history, the streams, the scratch, the errors.  What changes (every operation an IEEE f32 one rounded on its own, nothing fused;
 * dot(a, b) = (ax bx + ay by) + az bz):
 * The centre ray of pixel (x, y) is the lens law's ray for spp == 1 (no jitter: px = x + 0.5, py = y + 0.5): origin o_p (per pixel for ORTHO) and unit
 * direction d.  The shown point of a hit is P = o_p + z d per component, z the AOV depth.
 * turns(c, s), the angle of (c, s) in turns, in [0, 1):
 *     ac = |c|, as = |s|, hi = max(ac, as), lo = min(ac, as);  NaN unless ac and as are finite and hi > 0;
 *     t = lo / hi;  z = t * t;  p = a16;  for k in (a14, a12, a10, a8, a6, a4, a2): p = p * z, p = p + k;  p = p * z;  p = p + 1.0f;
 *     u = (t * p) * 0.159154937f;  if (as > ac) u = 0.25f - u;  if (c < 0) u = 0.5f - u;  if (s < 0) u = 1.0f - u;  if (u >= 1.0f) u = 0.0f
 *     a2 ... a16 = -0.3333314528, 0.1999355085, -0.1420889944, 0.1065626393, -0.0752896400, 0.0429096138, -0.0161657367, 0.0028662257
 *     (Abramowitz & Stegun 4.4.49); within 2^-23 turns of atan2.
 * The previous position.  r = P - o' for a hit ((P + m) - o' for a moved pixel), r = d for a miss, o' the previous lens's origin; an ORTHO miss is not
 * projected (x' = x, y' = y).  lx = dot(r, right'), ly = dot(r, up'), lz = dot(r, forward');  the depth the history's is compared with is
 * zhat = sqrtf(dot(r, r)), for ORTHO lz.  Then the frame position (px, py) and x' = px - 0.5f, y' = py - 0.5f:
 *     EQUIRECT  hxz = sqrtf(lx * lx + lz * lz);  a = turns(-lz, -lx);  b = 2.0f * turns(ly, hxz);  px = a * W;  py = b * H
 *     FISHEYE   hxy = sqrtf(lx * lx + ly * ly);  tau = turns(lz, hxy);  rr = tau / half_fov_turns';  if hxy > 0: nx = rr * (lx / hxy), ny = rr * (ly / hxy);
 *               else if tau == 0: nx = ny = 0;  else no history (the pole behind the lens);
 *               m = 0.5f * (float)min(W, H);  px = nx * m + 0.5f * W;  py = 0.5f * H - ny * m
 *     ORTHO     nx = lx / half_extent'[0];  ny = ly / half_extent'[1];  px = ((nx + 1.0f) * 0.5f) * W;  py = ((1.0f - ny) * 0.5f) * H
 *     CUBE      v = (lx, ly, -lz);  (f, m, sc, tc) by the face cases of the environment lookup law;  N = W;
 *               px = ((sc / m) * 0.5f + 0.5f) * N;  py = (float)(f * N) + ((tc / m) * 0.5f + 0.5f) * N
 * A NaN x' or y' (r = 0) is no history.  The bilinear taps are the camera's with two changes: EQUIRECT wraps columns (-1 -> W - 1, W -> 0); CUBE skips a
 * tap outside rows [f N, (f + 1) N) (no filtering across faces, as in the environment map).
 * Shortcut: when prev_lens equals lens bit for bit in model, origin, the three axes and the model's own parameter (half_fov_turns for FISHEYE,
 * half_extent for ORTHO; pads and other models' fields are ignored), a pixel that has not moved takes x' = x, y' = y.  A moved pixel is always projected.
 * Errors: those of rt3_denoise_temporal_motion* and rt3_motion*, with "a camera they refuse" replaced by "a lens the lens entry points refuse for this
 * W x H" (CUBE needs H = 6 W); prev_lens must have the model of lens.  W, H >= 2.  No scene is needed for the denoiser; rt3_motion_optic reads the
 * scene on the context as rt3_motion does.
 * Out of scope: the spatial passes cross the face edges of a stacked cube frame and do not wrap an equirectangular frame's columns (rt3_denoise's
 * behaviour on those frames); sharded lens frames. */
int   rt3_denoise_temporal_optic(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_lens* lens, const float* colour_rgba, const rt3_aov* aov,
                                 const rt3_lens* prev_lens, const rt3_history* prev_history, const float* motion,
                                 const rt3_temporal_params* p, float* out_rgba, rt3_history* out_history);
int   rt3_denoise_temporal_optic_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_lens* lens, const void* d_colour_rgba,
                                        const void* d_aov, const rt3_lens* prev_lens, const void* d_prev_history, const void* d_motion,
                                        const rt3_temporal_params* p, void* d_out_rgba, void* d_out_history, void* stream);
int   rt3_motion_optic(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_lens* lens, const rt3_aov* aov,
                       const float* prev_center_radius, uint32_t n_prev_spheres,
                       const float* prev_vertices_xyzw, uint32_t n_prev_vertices, float* out_motion);
int   rt3_motion_optic_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const rt3_lens* lens, const void* d_aov,
                              const void* d_prev_center_radius, uint32_t n_prev_spheres,
                              const void* d_prev_vertices_xyzw, uint32_t n_prev_vertices, void* d_out_motion, void* stream);
/* Host only, no device and no context: turns, and the previous position of r in prev_lens's W x H frame: out_xy_depth = (x', y', zhat), *face the
 * cube face (0 otherwise), *valid = 0 for no history.  An ORTHO miss (is_hit == 0) is not projected: (NaN, NaN, zhat), *valid = 1.  RT3_E_ARG for a
 * NULL pointer, width or height below 2, or a lens the entry points refuse.  tests/optic_ref.py restates both bit for bit. */
float rt3_debug_turns(float c, float s);
int   rt3_debug_optic_pixel(const rt3_lens* prev_lens, uint32_t width, uint32_t height, const float r[3], uint32_t is_hit,
                            float out_xy_depth[3], uint32_t* face, uint32_t* valid);

/* ---------------------------------------------------------------------------------------------------
 * Environment map  (DESIGN.md 4.19, 5.2n): a cube map answers every Mode-X ray that leaves the scene
 * ------------------------------------------------------------------------------------------------- */
/* The map.  6 faces of N x N texels, 1 <= N <= RT3_ENV_MAX_FACE, each texel a float4 (r, g, b, ignored).  Faces in the order +X, -X, +Y, -Y, +Z, -Z,
 * row 0 first: the texel of face f, row j, column i is at index (f * N + j) * N + i.
 * The lookup law.  For a direction d = (x, y, z) with ax = |x|, ay = |y|, az = |z|, the face f, the major-axis length m and the in-face
 * coordinates sc (columns) and tc (rows) are
 *     if (ax >= ay && ax >= az)  f = x < 0 ? 1 : 0,  m = ax,  sc = x < 0 ? z : -z,  tc = -y
 *     else if (ay >= az)         f = y < 0 ? 3 : 2,  m = ay,  sc = x,               tc = y < 0 ? -z : z
 *     else                       f = z < 0 ? 5 : 4,  m = az,  sc = z < 0 ? -x : x,  tc = -y
 * and then, for sc (giving x0, wx, i0, i1) and in the same way for tc (giving y0, wy, j0, j1), every operation an IEEE f32 one rounded on its
 * own, nothing fused:
 *     q = sc / m;  u = q * 0.5f + 0.5f;  fx = u * (float)N - 0.5f;  x0 = floorf(fx);  wx = fx - x0;
 *     x0 = fminf(fmaxf(x0, -1), N - 1)      (in float, the NaN-dropping min / max: a NaN gives -1), only then converted to an integer
 *     i0 = max(x0, 0);  i1 = min(x0 + 1, N - 1)
 * With cAB the texel at column iA, row jB, per channel:
 *     top = c00 + wx * (c10 - c00);  bot = c01 + wx * (c11 - c01);  c = top + wy * (bot - top)
 * So: filtering stays inside one face (clamp to edge, no seam handling); a face of one colour returns that colour exactly; on the four side
 * faces row 0 is up (+Y); and whatever d holds, non-finite values included, a lookup reads inside the map.
 * The miss of the Mode-X path law, in this order: under RT3_FLAG_BLACK_BACKGROUND nothing; otherwise, when a map is set, L = fma(T, c, L) per
 * channel with c = the lookup of the ray's direction; otherwise the sky.
 * Who reads the map: rt3_render_path*, rt3_render_path_range*, rt3_render_path_adaptive* and rt3_radiance* (the defining property of
 * rt3_radiance holds with a map set as without); rt3_render_aov* in its miss albedo (env(d) in place of sky(d)).  Mode R, queries, the denoisers
 * and rt3_camera_rays do not.  A render with RT3_FLAG_REFERENCE_PRIMARY while a map is set returns RT3_E_ARG (its primary direction is not a
 * unit vector, and it exists to reproduce the reference).  While a map is set the trace kernel is chosen as for a query: RT3_NO_MFMA,
 * RT3_MFMA_K64 and the flat filter (RT3_NO_GROUPS, rt3_debug_force_flat_filter) are ignored.  With no map set every entry point returns what it
 * returned before these functions existed, bit for bit.
 * State.  The map belongs to the context: it survives every scene upload, update and regroup and never touches the accumulation (a progressive
 * render continues across rt3_set_environment; what it continues WITH is the caller's business).
 * Errors.  n_face == 0 clears the map (the pointer may then be NULL).  RT3_E_ARG, with the previous map left in place: a NULL ctx or array,
 * n_face > RT3_ENV_MAX_FACE, a misaligned device pointer, and — host form only, the device form does not validate texels — a texel whose r, g
 * or b is not finite (the message names the lowest such texel index).
 * Out of scope: seamless filtering across face edges, mip levels, rotation.  (Importance sampling of the map: RT3_FLAG_ENV_SAMPLING, below.) */
#define RT3_ENV_MAX_FACE 2048u
/* Host array of 6 * n_face * n_face float4; the context copies it and owns the copy.  Synchronous. */
int      rt3_set_environment(rt3_ctx* ctx, const float* rgba, uint32_t n_face);
/* The same from a device array (16-byte aligned), queued on `stream` (the stream convention above); it takes part in the event chain as an update
 * does.  The caller's array is only read until the queued work has run. */
int      rt3_set_environment_device(rt3_ctx* ctx, const void* d_rgba, uint32_t n_face, void* stream);
int      rt3_clear_environment(rt3_ctx* ctx);
/* N, or 0 when no map is set. */
uint32_t rt3_environment_size(rt3_ctx* ctx);
/* Host only, no device and no context: the lookup law above in C, out_rgb = env(d).  RT3_E_ARG for a NULL pointer, n_face == 0 or
 * n_face > RT3_ENV_MAX_FACE.  The tests compare it and the device with tests/environment_ref.py bit for bit. */
int      rt3_debug_environment_lookup(const float* rgba, uint32_t n_face, const float d[3], float out_rgb[3]);

/* ---------------------------------------------------------------------------------------------------
 * Environment map: sampling  (DESIGN.md 4.20, 5.2o): RT3_FLAG_ENV_SAMPLING in rt3_params.flags / rt3_radiance_params.flags
 * ------------------------------------------------------------------------------------------------- */
/* Without the flag a path receives the map only where a scattered ray happens to leave the scene; a small bright region (a sun of a few texels)
 * is then found by a vanishing share of the bounces.  With it every Lambert scatter also draws a direction from the map's own brightness and
 * casts one shadow ray (next-event estimation).  Opt-in per call; rt3_render_path*, rt3_render_path_range* (shards included) and rt3_radiance*
 * accept it (the defining property of rt3_radiance holds with it).
 * The table.  Integers wherever something is added up, so it does not depend on the order it is built in.  M = min(N, 256) cells per face
 * edge; cell c of an axis is the interval [c / M, (c + 1) / M) of the face coordinate u of the lookup law.  A texel's brightness is
 * l = (max(r, 0) + max(g, 0)) + max(b, 0), the NaN-dropping max (a NaN counts as 0), +inf clamped to FLT_MAX.  A cell's weight is w = lmax * sa:
 * lmax the largest l among the texels the bilinear lookup can read inside the cell — per axis the texels floor(c N / M - 0.5) to
 * floor((c + 1) N / M - 0.5) + 1, clamped inside the face; for N <= 256 the cell's own texel and a ring of one around it — so w > 0 wherever
 * the lookup can be positive (negative radiance is not sampled: a texel such as (-1, -1, -1) has brightness 0, and on a map with negative
 * channels the flagged estimator differs from the plain one where only such texels are read); sa = 1 / (g * sqrtf(g)) with g = (s * s + t * t) + 1 at the cell's centre s = ((col + 0.5f) / M) * 2 - 1, t
 * likewise from the row; every operation f32, rounded on its own.  With W the largest w of the map, q = 0 if w == 0 and otherwise
 * max(1, (uint32_t)floorf(w / W * 16777216.0f)); cdf is the inclusive uint64 prefix sum of q in cell order (face, row, column), total its last
 * entry.  The table (at most 6 * 256^2 * 12 bytes) is built on the device by the first call that carries the flag, queued on that call's stream
 * inside the event chain as an update is, and kept until the map is set or cleared again; rt3_set_environment* costs what it cost.
 * The sampling law.  At a Lambert scatter of a path with RNG base `base` at depth d let ctr = 1 + 8 (d + 1) and w_k = hash_u32(base ^
 * hash_u32(ctr + k)), k = 3..6 (the scatter itself draws k = 0..2).  x = (uint64_t)w3 << 32 | w4, T = the high 64 bits of x * total; the cell
 * is the first index with cdf[index] > T (a cell with q = 0 is never drawn).  a = u01(w5), b = u01(w6);
 * s = ((col + a) / M) * 2 - 1, t = ((row + b) / M) * 2 - 1 in f32.  The direction is the lookup's face cases inverted,
 *     +X (1, -t, -s)   -X (-1, -t, s)   +Y (s, 1, t)   -Y (s, -1, -t)   +Z (s, -t, 1)   -Z (-s, -t, -1)
 * times 1 / sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx))), and its density per solid angle is
 *     pdf = ((float)q / (float)total) * ((float)(M * M) * 0.25f) * (g * sqrtf(g)),   g = (s * s + t * t) + 1 at the sampled (s, t).
 * The path law with the flag.  A Lambert hit that scatters (depth + 1 < max_depth) scatters exactly as without it — the continuation rays are
 * the plain render's — and draws w by the law above.  With T' = throughput * albedo and c = n.w (n the normal turned towards the ray, the dot
 * product as two fused multiply-adds): when total == 0 or not c > 0 nothing more happens; otherwise one shadow ray (hit point, w) is traced
 * with the nearest-hit rule (t_min, t_max = +inf) and, if it meets nothing, L = fma(T' * (c / (3.14159274f * pdf)), env(w), L) per channel;
 * if it meets something L is left as it is.  A later miss of that path adds nothing while its most recent scatter was a Lambert scatter (the
 * shadow ray has accounted for the map); after a metal or glass scatter, and for a primary ray, a miss reads the map as always.  FLAT, metal,
 * dielectric and the depth cut-off are unchanged.  Shadow rays are not a depth; they count in ray_casts and in the filter's counters.
 * Multiple importance sampling is not done: on a smooth map the estimator can be noisier per sample than the plain one.
 * Errors.  RT3_E_STATE: the flag with no map set.  RT3_E_ARG: together with RT3_FLAG_BLACK_BACKGROUND or RT3_FLAG_REFERENCE_PRIMARY;
 * rt3_render_path_adaptive* with the flag (its later rounds would need a list form of the sampling kernels: none is built).
 * rt3_render_aov*, rt3_camera_rays* and the accumulation calls accept the bit and ignore it. */
/* A declaration that exists for the test suite alone (no render calls it).  The macro is empty.  Why it follows the declarator: the test that
 * came with the environment map (tests/test_environment_abi.py) pins the exact set of `int|uint32_t rt3_*environment*(...);` declarations of
 * this header by a pattern that ends in `);`, and the two functions below carry "environment" in their names; with the marker between `)` and
 * `;` that pinned set stays what it was.  Once that test's list is extended the marker can go. */
#define RT3_TEST_ONLY
/* Host only, no device and no context: the table built serially and the sampling law above in C for one (base, depth).  *cell = the cell drawn,
 * dir = the unit direction, *pdf = its density; a map whose table has total == 0 gives *cell = 0xFFFFFFFF, dir = 0 and *pdf = 0 (nothing is
 * sampled).  RT3_E_ARG for a NULL pointer, n_face == 0 or n_face > RT3_ENV_MAX_FACE.  tests/environment_sample_ref.py restates it bit for bit.
 * Cost, as befits a debug function: the calling thread keeps a copy of the last map and its table for the thread's life (96 n_face^2 bytes plus
 * the table: about 400 MB at n_face = 2048) and every call compares the whole map with that copy before it reuses the table. */
int      rt3_debug_environment_sample(const float* rgba, uint32_t n_face, uint32_t base, uint32_t depth, uint32_t* cell, float dir[3],
                                      float* pdf) RT3_TEST_ONLY;
/* The device's table of the map the context holds (built first if no call with the flag has built it): q_out and cdf_out take 6 M^2 entries,
 * capacity_cells is what they can hold, *cells_per_edge = M (set whenever a map is set).  RT3_E_STATE without a map, RT3_E_ARG for a NULL
 * pointer or a capacity below 6 M^2.  Synchronous. */
int      rt3_debug_environment_table(rt3_ctx* ctx, uint32_t* q_out, uint64_t* cdf_out, uint64_t capacity_cells,
                                     uint32_t* cells_per_edge) RT3_TEST_ONLY;

/* ---------------------------------------------------------------------------------------------------
 * Emitters: sampling  (DESIGN.md 4.21, 5.2p): RT3_FLAG_LIGHT_SAMPLING in rt3_params.flags / rt3_radiance_params.flags
 * ------------------------------------------------------------------------------------------------- */
/* A RT3_MAT_FLAT primitive emits: a hit adds throughput * rgb and ends the path.  Without the flag a path receives that light only where a scattered
 * ray happens to run into the emitter; a small lamp is then found by a vanishing share of the bounces.  With it every Lambert scatter also draws a
 * point on one emitter and casts one shadow ray towards it (next-event estimation).  Opt-in per call; rt3_render_path*, rt3_render_path_range*
 * (shards included) and rt3_radiance* accept it, with or without RT3_FLAG_BLACK_BACKGROUND, with or without a map (the defining property of
 * rt3_radiance holds with it).
 * The table.  One entry per primitive in the caller's order, faces first and then spheres: entry i < n_faces is face i, otherwise sphere
 * i - n_faces (the order of rt3_hit.index).  Integers wherever something is added up.  Brightness l = (max(r, 0) + max(g, 0)) + max(b, 0) of the
 * material's rgb, the NaN-dropping max, +inf clamped to FLT_MAX; l = 0 for any kind but RT3_MAT_FLAT.  Area of a face: e1 = p2 - p1, e2 = p3 - p1,
 * x = e1 x e2 with every product and difference rounded on its own, g2 = fmaf(x.z, x.z, fmaf(x.y, x.y, x.x * x.x)), a = 0.5f * sqrtf(g2); of a
 * sphere: a = 12.566371f * (r * r).  Weight w = l * a; a NaN w, or an a that is not finite and > 0 (a degenerate face, a sphere record nothing can
 * hit), gives w = 0; +inf is clamped to FLT_MAX.  With W the largest w, q = 0 where w == 0 and otherwise max(1, (uint32_t)floorf(w / W *
 * 16777216.0f)); cdf is the inclusive uint64 prefix sum of q, total its last entry.  The table (12 bytes per primitive) is built on the device by
 * the first call that carries the flag, queued on that call's stream inside the event chain, and kept until the scene changes: rt3_set_spheres*,
 * rt3_set_mesh*, rt3_mesh_commit, rt3_update_spheres* and rt3_update_mesh* invalidate it, rt3_regroup* and the environment calls do not.
 * The sampling law.  At a Lambert scatter of a path with RNG base `base` at depth d: ctr = 1 + 8 (d + 1), w_k = hash_u32(base ^ hash_u32(ctr + k)),
 * k = 3..6 (the counters of RT3_FLAG_ENV_SAMPLING, which the flag excludes; the scatter keeps k = 0..2).  x = (uint64_t)w3 << 32 | w4, T = the
 * high 64 bits of x * total; the light is the first index with cdf[index] > T.  a = u01(w5), b = u01(w6).
 *   A face: if a + b > 1 then a = 1 - a, b = 1 - b; per component y = fmaf(b, e2, fmaf(a, e1, p1)); the light's normal is x * (1 / sqrtf(g2)).
 *   A sphere: v = the scatter's own random unit vector of (a, b); per component y = fmaf(r, v, c); the light's normal is v.
 * With p the hit point the continuation starts from: D = y - p, d2 = D.D (every dot product here is fmaf(z, z', fmaf(y, y', x * x'))),
 * w = D * (1 / sqrtf(d2)), cl = |n_light . w|, c = n . w with n the surface normal turned towards the ray.  The sample is dropped — no shadow ray —
 * when total == 0; when d2 is not finite and > 0; when not cl > 0; when not c > 0; and when the light is a sphere, p lies outside it (|p - c|^2 >
 * r * r) and v . w >= 0: the far side, which the near side hides (from inside every point counts: FLAT emits on both sides).  Otherwise
 * pl = (float)q / (float)total, k = ((c * cl) * a_light) / ((3.14159274f * d2) * pl), and the lane parks E = T' * k, T' = throughput * albedo,
 * with the light's index and the continuation's direction; the shadow ray (p, w) takes the next cast with the nearest-hit rule (t_min,
 * t_max = +inf).  If its nearest hit is that very primitive (same class and index), L = fma(E, rgb_light, L) per channel; anything else, a miss
 * included, leaves L as it is.  The lane then goes on with the continuation.
 * The path law with the flag.  The scatter draws what it always drew: the continuation rays are the plain render's.  A hit on a FLAT primitive whose
 * q > 0 adds nothing while the path's most recent scatter was a Lambert scatter (the shadow ray has accounted for it; the path ends there as
 * always); a FLAT primitive with q == 0 keeps adding, and so does every FLAT hit of a primary ray or behind a metal or glass scatter.  A miss is
 * the plain render's (sky, black, or the map's plain lookup); the depth cut-off, metal and glass are unchanged.  Shadow rays are not a depth; they
 * count in ray_casts and in the filter's counters.  Multiple importance sampling is not done: a large emitter close to a surface can be noisier
 * per sample than in the plain render.
 * Errors.  RT3_E_ARG, each with a message of its own that comes before any older refusal: together with RT3_FLAG_ENV_SAMPLING (two shadow rays per
 * scatter: not built); together with RT3_FLAG_REFERENCE_PRIMARY; rt3_render_path_adaptive* with the flag (no list form of the sampling kernels).
 * rt3_render_aov*, rt3_camera_rays* and the accumulation calls accept the bit and ignore it. */
/* Host only, no device and no context; for the tests.  The table built serially from the caller's arrays (faces and vertices as rt3_set_mesh takes
 * them, spheres as rt3_set_spheres does), then the law above for one (base, depth): *light = the entry drawn, point = y, light_normal, *area = the
 * light's, *pl = q / total.  An empty table (total == 0) gives *light = 0xFFFFFFFF and zeros.  RT3_E_ARG for a NULL pointer with a non-zero count,
 * a NULL result pointer, or a face index out of range.  tests/light_sample_ref.py restates it bit for bit. */
int      rt3_debug_light_sample(const rt3_gface* faces, uint32_t n_faces, const float* vertices_xyzw, uint32_t n_vertices,
                                const rt3_material* face_materials, const float* center_radius, const rt3_material* sphere_materials,
                                uint32_t n_spheres, uint32_t base, uint32_t depth, uint32_t* light, float point[3], float light_normal[3],
                                float* area, float* pl);
/* The device's table of the scene the context holds (built first if no call with the flag has built it): q_out and cdf_out take n_faces + n_spheres
 * entries, capacity is what they can hold, *n_entries that count.  RT3_E_STATE without a scene, RT3_E_ARG for a NULL pointer or a short capacity
 * (*n_entries is set).  Synchronous; for the tests. */
int      rt3_debug_light_table(rt3_ctx* ctx, uint32_t* q_out, uint64_t* cdf_out, uint64_t capacity, uint32_t* n_entries);

/* ---------------------------------------------------------------------------------------------------
 * Display transform  (DESIGN.md 4.22, 5.2q): a linear float frame -> RGBA8 words: exposure, a tone curve, a transfer function
 * ------------------------------------------------------------------------------------------------- */
#define RT3_DISPLAY_CLAMP          0u   /* curve: none; values above 1 clip */
#define RT3_DISPLAY_REINHARD       1u   /* curve: extended Reinhard on the luminance, `white` is mapped to 1 */
#define RT3_DISPLAY_FILMIC         2u   /* curve: the rational filmic fit (2.51, 0.03, 2.43, 0.59, 0.14) per channel */
#define RT3_DISPLAY_LINEAR         0u   /* transfer: none: the pack of a render without RT3_FLAG_GAMMA2 */
#define RT3_DISPLAY_GAMMA2         1u   /* transfer: a square root: the pack of a render with RT3_FLAG_GAMMA2 */
#define RT3_DISPLAY_SRGB           2u   /* transfer: the sRGB encoding, from a table of 4096 bytes */
#define RT3_DISPLAY_AUTO_EXPOSURE  1u   /* flags: the gain follows the frame's trimmed log-average luminance */
typedef struct rt3_display_params {      /* 32 bytes */
    uint32_t curve;                      /* RT3_DISPLAY_CLAMP 0 | RT3_DISPLAY_REINHARD 1 | RT3_DISPLAY_FILMIC 2 */
    uint32_t transfer;                   /* RT3_DISPLAY_LINEAR 0 | RT3_DISPLAY_GAMMA2 1 | RT3_DISPLAY_SRGB 2 */
    uint32_t flags;                      /* RT3_DISPLAY_AUTO_EXPOSURE 1; any other bit: RT3_E_ARG */
    uint32_t trim_low;                   /* auto: share of the counted pixels dropped from the dark end, in 1/1024; default 102 */
    uint32_t trim_high;                  /* ... from the bright end; trim_low + trim_high <= 1023; default 51 */
    float    exposure;                   /* linear gain, finite and > 0; default 1 */
    float    key;                        /* auto: the value the trimmed log-average luminance is mapped to; finite and > 0; default 0.18 */
    float    white;                      /* REINHARD: luminance mapped to 1; finite and >= 2^-10, or +inf (plain Reinhard); default 4 */
} rt3_display_params;
/* width x height pixels of (r, g, b, ignored) floats, as rt3_accum_resolve / rt3_denoise write them, to one word per pixel in the layout of
 * rt3_render_path's frame, 0xFF | B << 8 | G << 16 | R << 24.  Geometry does not matter: a whole frame and a shard's compact rows are both accepted.
 * trim_*, key and white are checked even where they are not used.  No transcendental function and no floating-point sum over pixels: every statistic
 * is an integer, every per-pixel step is + - * /, sqrtf, fmaf, a comparison or a table lookup, each an IEEE f32 operation rounded on its own.
 * The gain.  Without RT3_DISPLAY_AUTO_EXPOSURE, gain = exposure.  With it, per pixel y_c = c > 0 ? fminf(c, FLT_MAX) : 0 (NaN and negatives become 0),
 * Y = fmaf(0.0722f, y_b, fmaf(0.7152f, y_g, 0.2126f * y_r)), k = (int32_t)(bits(Y) >> 19) - 1776.  k < 0 (Y < 2^-16): the pixel is dark; it is counted
 * in `dark` and not in the histogram.  Otherwise hist[min(k, 511)] += 1: 512 bins, 16 per octave, 2^-16 up to 2^16; +inf lands in bin 511.  With
 * n = sum(hist): lo = (n * trim_low) >> 10 and hi = (n * trim_high) >> 10 in uint64; the ranks [lo, n - hi) are kept, ranks assigned in bin order:
 * kept_k = max(0, min(end_k, n - hi) - max(begin_k, lo)).  m = n - lo - hi, S = sum(kept_k * k), P = (S << 19) / m as a uint64 floor division,
 * Lavg = float_from_bits((111u << 23) + (uint32_t)P + (1u << 18)) — the bin centre; the float's bit pattern serves as its piecewise-linear log2 —
 * and gain = exposure * (key / Lavg).  n == 0 gives gain = exposure.
 * Per pixel and channel.  x = g > 0 ? fminf(g, 65504.0f) : 0 with g = gain * c (NaN, negatives and 0 * inf become 0).  The curve: CLAMP y = x;
 * REINHARD Yx = fmaf(0.0722f, x_b, fmaf(0.7152f, x_g, 0.2126f * x_r)), s = (1.0f + Yx / (white * white)) / (1.0f + Yx), y = x * s; FILMIC
 * y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f), nothing fused.  z = fminf(y, 1.0f).  The transfer: LINEAR byte = pack(z), the
 * channel pack of rt3_render_path (round(z * 255), half away from zero); GAMMA2 byte = pack(sqrtf(z)); SRGB byte = table[(uint32_t)roundf(z * 4095.0f)],
 * table[i] = the number of k in 1 .. 255 with (k - 0.5) / 255 at or below the sRGB encoding of i / 4095 (4096 bytes; monotone, every code, steps of 1).
 * Anchor.  CLAMP, exposure 1, no flag: applied to rt3_accum_resolve's frame it returns, word for word, what rt3_render_path returned for that render —
 * LINEAR for a render without RT3_FLAG_GAMMA2, GAMMA2 for one with it.
 * No scene is needed.  The call never touches the accumulation of a progressive render and leaves rt3_get_stats as it was.  Streams as for queries;
 * the host form is synchronous; the device form never waits for the device, with the flag neither: the gain stays in device memory between the
 * kernels.  The device form allocates only on a context's first call with the flag (516 words of state).  RT3_E_ARG for a NULL pointer, width or
 * height 0, width x height > 2^26, a parameter outside the ranges above (unknown curve, transfer or flag bits included), a device input that is not
 * 16-byte aligned or a device output that is not 4-byte aligned, or an output that overlaps the input; a refused call writes nothing.  Out of scope:
 * one exposure shared by the shards of a multi-device frame (gather first, or pass the gain as `exposure`), local operators other than the bloom of
 * rt3_display_sequence (below, with eye adaptation over a sequence), dither. */
int      rt3_display(rt3_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const rt3_display_params* p, uint32_t* out_pixels);
int      rt3_display_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const void* d_rgba, const rt3_display_params* p, void* d_out_pixels,
                            void* stream);
/* Tests only: the histogram, the dark count and the gain of the context's last call with RT3_DISPLAY_AUTO_EXPOSURE (any of them may be NULL).
 * RT3_E_STATE if there was none.  Synchronous. */
int      rt3_debug_display_state(rt3_ctx* ctx, uint32_t hist[512], uint32_t* dark, float* gain);
/* Host only, no device and no context; for the tests: the law above in C.  *bin = 0 .. 511, 0xFFFFFFFF for a dark pixel; the gain of a histogram
 * under p's exposure, key and trims (flags are not looked at); one pixel's word for a given gain; the table.  RT3_E_ARG for a NULL pointer or
 * parameters rt3_display would refuse.  tests/display_ref.py restates them bit for bit. */
int      rt3_debug_display_bin(const float rgb[3], uint32_t* bin);
int      rt3_debug_display_gain(const uint32_t hist[512], const rt3_display_params* p, float* gain);
int      rt3_debug_display_pixel(const float rgb[3], float gain, const rt3_display_params* p, uint32_t* word);
int      rt3_debug_display_srgb_table(uint8_t out[4096]);

/* ---------------------------------------------------------------------------------------------------
 * Display sequences  (DESIGN.md 4.25, 5.2t): rt3_display with an exposure that follows a sequence of frames and a bloom pyramid
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt3_exposure {            /* 16 bytes; one per sequence, owned by the caller, host or device */
    uint32_t level;                      /* P: the adapted log-luminance, in 2^-19 of a histogram bin; 0 .. 511 << 19 */
    uint32_t frames;                     /* frames that have set it; 0 = no level yet */
    float    gain;                       /* the gain the call applied */
    uint32_t _pad;                       /* 0 */
} rt3_exposure;
typedef struct rt3_display_sequence_params {   /* 64 bytes */
    rt3_display_params display;          /* as for rt3_display; its refusals unchanged */
    uint32_t adapt_brighter;             /* share of the way to a BRIGHTER target per frame, in 1/1024; 1 .. 1024; default 256 */
    uint32_t adapt_darker;               /* ... to a darker target; 1 .. 1024; default 64 */
    uint32_t bloom_levels;               /* L: 0 = no bloom, else 1 .. 8 */
    float    bloom_threshold;            /* T: finite, >= 0; default 1 */
    float    bloom_intensity;            /* finite, >= 0; default 0.25 */
    uint32_t _pad[3];                    /* 0, else RT3_E_ARG */
} rt3_display_sequence_params;
/* rt3_display (above: the frame, the words, the histogram, the curve and the transfer are its) with two additions: the gain follows the sequence
 * through a state the caller keeps between the frames, and a bloom pyramid is added to the frame before the tone curve.  The frame is a real
 * width x height image (a shard's compact rows are not: gather first).
 * The exposure.  hist, n, the trim, m and S as for rt3_display; the frame's target is P_t = (S << 19) / m (uint64 floor division).
 *   Without RT3_DISPLAY_AUTO_EXPOSURE: gain = display.exposure; prev_exposure must be NULL; out_exposure, if given, gets {0, 0, gain, 0}.
 *   With it and no usable history (prev_exposure NULL, or prev.frames == 0): n > 0 gives level = P_t, frames = 1; n == 0 gives
 *   {0, 0, display.exposure, 0} (an all-dark first frame sets nothing).
 *   With it and prev.frames > 0: n == 0 gives level = prev.level (a black frame does not move the eye).  Otherwise d = P_t - prev.level,
 *   rate = d > 0 ? adapt_brighter : adapt_darker, d == 0 gives level = prev.level, else step = max(1, (|d| * rate) >> 10) in uint64 and
 *   level = prev.level + step for d > 0, prev.level - step for d < 0: step <= |d|, so the level moves monotonically and lands on P_t exactly.
 *   frames = min(prev.frames + 1, 0xFFFFFFFF).
 *   The gain, wherever a level was set: gain = exposure * (key / float_from_bits((111u << 23) + level + (1u << 18))), rt3_display's expression:
 *   rates of 1024 (and a first frame) reproduce rt3_display.  prev.gain and prev._pad are not read.
 *   A prev.level above 511 << 19: the host form refuses it (RT3_E_ARG); the device form, which cannot look without waiting, reads it as 511 << 19.
 * The bloom (bloom_levels = L >= 1; every operation an IEEE f32 operation rounded on its own, nothing fused but the luminance's two fmaf).
 *   With x_c = g > 0 ? fminf(g, 65504.0f) : 0, g = gain * c, as rt3_display forms it, on planes of (r, g, b):
 *   Bright pass: Y = fmaf(0.0722f, x_b, fmaf(0.7152f, x_g, 0.2126f * x_r)), k = Y > T ? (Y - T) / Y : 0, b0_c = x_c * k.
 *   Down, l = 1 .. L: W_l = (W_{l-1} + 1) >> 1, H_l likewise (W_0 x H_0 is the frame); D_l(i, j) = ((s(2i, 2j) + s(2i+1, 2j)) + (s(2i, 2j+1) +
 *   s(2i+1, 2j+1))) * 0.25f with s = D_{l-1}, D_0 = b0, source indices clamped to the last column and row.
 *   Up: up(U)(i, j) onto a w x h plane from a Wc x Hc plane: ia = i >> 1, ib = i odd ? min(ia + 1, Wc - 1) : max(ia - 1, 0), ja and jb likewise
 *   from j and Hc; r(jr) = 0.75f * U(ia, jr) + 0.25f * U(ib, jr); the value is 0.75f * r(ja) + 0.25f * r(jb).  U_L = D_L; for l = L-1 .. 1
 *   U_l = D_l + up(U_{l+1}); B = up(U_1) * (1.0f / (float)L) at the frame's size.
 *   Composite: x'_c = fminf(x_c + bloom_intensity * B_c, 65504.0f); the curve and the transfer run on x' as rt3_display runs them on x.  The
 *   histogram reads the input frame, never the bloom.  A frame with no pixel above T, and an intensity of 0, give the words without bloom.
 * Streams and the event chain as for rt3_display; the host form is synchronous, the device form never waits for the device.  The pyramid
 * (width x height / 3 texels of 16 bytes, a little more for odd sizes) is the context's, grows on demand and is kept after the call.  The call
 * never touches the accumulation and leaves rt3_get_stats as it was.  d_prev_exposure == d_out_exposure is allowed (one 16-byte record serves a
 * sequence; prev_exposure == out_exposure likewise).  RT3_E_ARG, nothing written: a NULL ctx, p, input or output pixels; whatever rt3_display
 * refuses in p->display; a rate outside 1 .. 1024; bloom_levels > 8; a threshold or an intensity that is not finite and >= 0 (checked with
 * bloom_levels == 0 too); a non-zero pad; prev_exposure without the flag; a host prev.level above 511 << 19; width or height 0 or
 * width x height > 2^26; a device input that is not 16-byte aligned, device words or exposure records that are not 4-byte aligned; any overlap
 * among the four buffers other than prev == out.  Out of scope: bloom and one exposure across the shards of a multi-device frame. */
int      rt3_display_sequence(rt3_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const rt3_display_sequence_params* p,
                              const rt3_exposure* prev_exposure, rt3_exposure* out_exposure, uint32_t* out_pixels);
int      rt3_display_sequence_device(rt3_ctx* ctx, uint32_t width, uint32_t height, const void* d_rgba, const rt3_display_sequence_params* p,
                                     const void* d_prev_exposure, void* d_out_exposure, void* d_out_pixels, void* stream);
/* Tests only: U_1 (W_1 x H_1 float4, the fourth float 0) of the context's last call with bloom_levels >= 1, and B (width x height float4), formed
 * from U_1 by the device function the composite uses.  Either output may be NULL; capacity_pixels is what out_bloom can hold (out_u1 needs no more);
 * *w and *h are set to that call's frame size whenever the context has one.  RT3_E_STATE if there was no such call, RT3_E_ARG for NULL w / h or a
 * short capacity.  Synchronous. */
int      rt3_debug_display_bloom(rt3_ctx* ctx, float* out_u1, float* out_bloom, uint64_t capacity_pixels, uint32_t* w, uint32_t* h);
/* Host only, no device and no context; for the tests: the laws above in C, serially.  rt3_debug_exposure_step: the state after a frame with this
 * histogram (prev may be NULL).  rt3_debug_bloom: U_1 (W_1 x H_1 float4) and B (w x h float4) of a w x h float4 frame under a given gain; either
 * output may be NULL; levels 1 .. 8.  RT3_E_ARG for what the entry points refuse; a refused call writes nothing.
 * tests/display_sequence_ref.py restates them bit for bit. */
int      rt3_debug_exposure_step(const rt3_exposure* prev, const uint32_t hist[512], const rt3_display_sequence_params* p, rt3_exposure* out);
int      rt3_debug_bloom(uint32_t w, uint32_t h, const float* rgba, float gain, float threshold, uint32_t levels, float* out_u1, float* out_bloom);

/* ---------------------------------------------------------------------------------------------------
 * Image textures: albedo maps on spheres and mesh faces in Mode X
 * ------------------------------------------------------------------------------------------------- */
/* The law, written out (raytracer-3_amd/csrc/rt3_texture_law.hpp states it once for the device and the host; tests/texture_ref.py restates it in
 * numpy).  Every operation is an IEEE f32 one rounded on its own, nothing is fused except where the path law already fuses (the sphere's hit point);
 * dot(a, b) = (ax bx + ay by) + az bz.
 *
 * Texture: W x H float4 texels (r, g, b, ignored), row 0 on top, texel (i, j) at j * W + i; 1 <= W, H <= RT3_TEX_MAX_SIDE and W * H <= 2^26.  Wrap is
 * RT3_TEX_REPEAT or RT3_TEX_CLAMP, one mode for both axes.
 *
 * Lookup of (u, v) — for u with W, and in the same way for v with H:
 *   REPEAT: u = u - floorf(u) first.
 *   fx = u * (float)W - 0.5f; x0 = floorf(fx); wx = fx - x0;
 *   x0 is clamped in float to [-1, W - 1] with the NaN-dropping min / max (a NaN becomes -1), and only then converted.
 *   Taps i0 = x0, i1 = x0 + 1.  REPEAT wraps them (-1 -> W - 1, W -> 0); CLAMP takes i0 = max(x0, 0), i1 = min(x0 + 1, W - 1).
 *   top = c00 + wx * (c10 - c00); bot = c01 + wx * (c11 - c01); c = top + wy * (bot - top)   (c10: tap i1 of row j0, c01: tap i0 of row j1)
 * A texture of one colour returns that colour exactly.  Whatever (u, v) holds, non-finite values included, a lookup reads inside the image.
 *
 * Sphere (u, v), from the unit outward normal n = (p - C) * (1 / r) as the path law computes it, before the flip towards the ray:
 *   hxz = sqrtf(nx * nx + nz * nz); u = hxz > 0 ? turns(-nx, nz) : 0; v = 2.0f * turns(ny, hxz)          (turns: rt3_debug_turns)
 * — the book's u = (atan2(-z, x) + pi) / 2 pi, with v = 0 at the north pole (+y): an equirectangular image sits the way the book's does.
 *
 * Face (u, v), from the hit point p = o + t d (unfused), the face's vertices p1, p2, p3 and its six floats (u1, v1, u2, v2, u3, v3):
 *   e1 = p2 - p1; e2 = p3 - p1; q = p - p1;
 *   d11 = dot(e1, e1); d12 = dot(e1, e2); d22 = dot(e2, e2); q1 = dot(q, e1); q2 = dot(q, e2);
 *   den = d11 * d22 - d12 * d12;
 *   b2 = (d22 * q1 - d12 * q2) / den; b3 = (d11 * q2 - d12 * q1) / den;   (both 0 when den == 0)
 *   b1 = (1.0f - b2) - b3;
 *   u = (b1 * u1 + b2 * u2) + b3 * u3, and v likewise.
 *
 * Shading: at a hit of a primitive bound to a texture the material's rgb is multiplied per channel by the texel (rgb[0] * c.r, and so on) for
 * RT3_MAT_FLAT, RT3_MAT_LAMBERT and RT3_MAT_METAL; everything after that is the path law as it stands.  A dielectric ignores its binding.  So a
 * texture whose texels are all (1, 1, 1) changes no bit of any result, and a texture of one colour c gives exactly the scene whose materials were
 * multiplied by c in f32 on the host.
 *
 * State.  Slots hold copies that the context owns.  Bindings are per primitive in the caller's order — the order of rt3_hit.index —, RT3_TEX_NONE
 * means untextured.  Textures survive everything except rt3_clear_textures and the freeing of their slot.  A class's binding survives
 * rt3_update_* and rt3_regroup*, and is dropped by a full upload of that class (rt3_set_spheres*, rt3_set_mesh*, rt3_mesh_commit).  A context is
 * TEXTURED while some binding names a slot; with no binding every entry point returns what it returned before textures existed, bit for bit.
 * The device forms follow the stream convention and the event chain of the updates; the binding forms wait once for the device's check of the slots.
 *
 * Who reads the textures: rt3_render_path*, rt3_render_path_range*, rt3_render_path_adaptive*, rt3_radiance*, rt3_render_lens* — and
 * rt3_render_aov* / rt3_render_lens_aov*, whose albedo is the modulated one.  Mode R, the queries, rt3_motion* and the denoisers do not.  Those
 * readers return RT3_E_STATE while a binding names an empty slot and, while textured, refuse RT3_FLAG_REFERENCE_PRIMARY (as with a map),
 * RT3_FLAG_ENV_SAMPLING and RT3_FLAG_LIGHT_SAMPLING (the tables' weights would have to see the texels) with RT3_E_ARG.
 *
 * Errors.  RT3_E_ARG, with the state untouched, for a slot >= RT3_TEX_MAX_TEXTURES, a side or area over the limit, an unknown wrap, a slot index
 * in a binding that is neither RT3_TEX_NONE nor < RT3_TEX_MAX_TEXTURES, a count that is not the class's count, a NULL or misaligned pointer
 * (device arrays: texels 16-byte, slots and uv 4-byte aligned), or — host forms only — a non-finite texel (r, g or b) or uv; the message names
 * the lowest such index.  RT3_E_STATE when binding a class that has no scene.
 *
 * Out of scope: mip levels and any filtering beyond bilinear; 8-bit or compressed texels; normal, roughness and emission-only maps; `vt` from OBJ
 * files and SceneLang syntax; textures under the two sampling flags; a per-axis wrap mode. */
#define RT3_TEX_MAX_TEXTURES 256u
#define RT3_TEX_MAX_SIDE     8192u
#define RT3_TEX_NONE         0xFFFFFFFFu
#define RT3_TEX_REPEAT       0u
#define RT3_TEX_CLAMP        1u
/* w == 0 or h == 0 frees the slot (bindings that name it stay, and make the readers return RT3_E_STATE until it is set again). */
int      rt3_set_texture(rt3_ctx* ctx, uint32_t slot, const float* rgba, uint32_t w, uint32_t h, uint32_t wrap);
int      rt3_set_texture_device(rt3_ctx* ctx, uint32_t slot, const void* d_rgba, uint32_t w, uint32_t h, uint32_t wrap, void* stream);
/* Every slot and every binding. */
int      rt3_clear_textures(rt3_ctx* ctx);
/* (0, 0) for an empty slot; NULL outputs are skipped. */
int      rt3_texture_size(rt3_ctx* ctx, uint32_t slot, uint32_t* w, uint32_t* h, uint32_t* wrap);
/* n = the sphere count; slots == NULL or n == 0 unbinds the class. */
int      rt3_bind_sphere_textures(rt3_ctx* ctx, const uint32_t* slots, uint32_t n);
int      rt3_bind_sphere_textures_device(rt3_ctx* ctx, const void* d_slots, uint32_t n, void* stream);
/* n_faces = the committed face count, uv6: 6 floats per face (u1, v1, u2, v2, u3, v3); slots == NULL or n_faces == 0 unbinds the class. */
int      rt3_bind_mesh_textures(rt3_ctx* ctx, const uint32_t* slots, const float* uv6, uint32_t n_faces);
int      rt3_bind_mesh_textures_device(rt3_ctx* ctx, const void* d_slots, const void* d_uv6, uint32_t n_faces, void* stream);
/* Tests only — host only, no device, no context: the law in C.  RT3_E_ARG for a NULL pointer, a side or area outside the limits, an unknown wrap. */
int      rt3_debug_texture_lookup(const float* rgba, uint32_t w, uint32_t h, uint32_t wrap, const float uv[2], float out_rgb[3]);
int      rt3_debug_texture_sphere_uv(const float n[3], float uv[2]);
int      rt3_debug_texture_face_uv(const float p1[3], const float p2[3], const float p3[3], const float uv6[6], const float p[3], float uv[2]);

/* ---------------------------------------------------------------------------------------------------
 * Host-side scene API  (the step before the path: entities -> GFace[]/vec4[]; plain CPU code)
 * ------------------------------------------------------------------------------------------------- */
/* cpu_pre_render_triangle (src/lib/entities/Triangle.cpp:28-76): 1 face, 3 vertices (xyzw). */
void     rt3_prerender_triangle(const float p1[3], const float p2[3], const float p3[3], const float color[3],
                                rt3_gface* faces, float* vertices_xyzw);
/* create_sphere counts (src/lib/entities/Sphere.cpp:101-102). */
uint32_t rt3_sphere_face_count(uint32_t n_meridians, uint32_t n_parallels);
uint32_t rt3_sphere_vertex_count(uint32_t n_meridians, uint32_t n_parallels);
/* cpu_pre_render_sphere (src/lib/entities/Sphere.cpp:120-261). */
void     rt3_prerender_sphere(const float center[3], float radius, uint32_t n_meridians, uint32_t n_parallels,
                              const float color[3], rt3_gface* faces, float* vertices_xyzw);
/* create_object's counting pass (src/lib/entities/Object.cpp:84-119). */
int      rt3_object_count(const char* path, uint32_t* n_faces, uint32_t* n_vertices);
/* cpu_pre_render_object (src/lib/entities/Object.cpp:131-199). */
int      rt3_prerender_object(const char* path, const float center[3], float scale, const float color[3],
                              rt3_gface* faces, uint32_t n_faces, float* vertices_xyzw, uint32_t n_vertices);
/* SequentialRenderer::transfer_entity (SequentialRenderer.cpp:174-195): append with index rebasing.
 * dst_* must have room; *dst_nf / *dst_nv are advanced. */
void     rt3_transfer_entity(rt3_gface* dst_faces, uint32_t* dst_nf, float* dst_vertices_xyzw, uint32_t* dst_nv,
                             const rt3_gface* faces, uint32_t nf, const float* vertices_xyzw, uint32_t nv);

/* Camera::update (src/lib/camera/Camera.cpp:77-96). */
void     rt3_camera_update(rt3_camera* cam, float focal_length, float viewport_width, float viewport_height);
/* Extension (the reference camera cannot look-from/look-at): book camera, vfov in degrees. */
void     rt3_camera_look_at(rt3_camera* cam, const float from[3], const float at[3], const float vup[3],
                            float vfov_deg, float aspect, float focus_dist);

/* Frame::to_ppm bytes (src/lib/camera/Frame.cpp:109-148): header + 3*w*h bytes.  Returns bytes written to
 * `out` (capacity cap) or the required size when out == NULL. */
uint64_t rt3_frame_ppm_bytes(const uint32_t* pixels, uint32_t width, uint32_t height, uint8_t* out, uint64_t cap);
int      rt3_frame_to_ppm(const uint32_t* pixels, uint32_t width, uint32_t height, const char* path);
/* Portable float map of a float image: "PF" (channels 3) or "Pf" (channels 1) header, scale -1.0 (little-endian), rows bottom to top.
 * Pixel (x, y), row 0 on top, is data[(y * width + x) * stride_floats + c]; stride_floats >= channels (an rt3_aov frame is read with
 * stride 12: albedo at offset 0, normal at 4, depth at 7).  Returns the bytes written to `out` (capacity cap), the required size when
 * out == NULL, 0 for bad arguments or a short buffer.  rt3_frame_to_pfm: RT3_E_ARG / RT3_E_IO. */
uint64_t rt3_frame_pfm_bytes(const float* data, uint32_t width, uint32_t height, uint32_t channels, uint32_t stride_floats,
                             uint8_t* out, uint64_t cap);
int      rt3_frame_to_pfm(const float* data, uint32_t width, uint32_t height, uint32_t channels, uint32_t stride_floats, const char* path);

/* Benchmark scenes (build-owned).  Each returns the sphere count of the scene — the count REQUIRED, whatever
 * cap is (snprintf convention) — and writes at most cap spheres; NULL outputs write nothing.  All randomness comes from the reference's hash RNG
 * (src/lib/shaders/random_v1.glsl:22-52) keyed by (seed, slot, dimension). */
uint32_t rt3_scene_three_spheres(float* center_radius, rt3_material* materials, uint32_t cap);
uint32_t rt3_scene_weekend(uint32_t seed, float* center_radius, rt3_material* materials, uint32_t cap);
uint32_t rt3_scene_stress(uint32_t n, uint32_t seed, float* center_radius, rt3_material* materials, uint32_t cap);
/* Cornell-style box tessellated into triangles (grid x grid quads per wall) with one emissive quad.
 * Returns the scene's face count (required, as above; at most cap_faces are written); vertices = 3 per face (unindexed).
 * NULL outputs -> counts only. */
uint32_t rt3_scene_cornell(uint32_t grid, rt3_gface* faces, float* vertices_xyzw, rt3_material* face_materials,
                           uint32_t cap_faces);

/* Reference hash RNG, exported for known-answer tests (random_v1.glsl:22-52). */
uint32_t rt3_hash_u32(uint32_t x);
float    rt3_random_float(uint32_t m);

/* Debug probe used by the parity tests only: element-wise DEVICE arithmetic on n inputs —
 * div = a/b, sq = sqrt(|a|), fm = fma(a,b,a), (cs,sn) = sincos2pi(frac bits of a), sk3 = sky(a,b,-2) (3 per
 * element), pk = pack(a,b,u).  Lets the tests prove the device's IEEE behaviour matches the host's. */
/* Debug switch used by the parity tests only: non-zero makes rt3_render* always take the plain brute-force Mode-R kernel
 * instead of the bounding-sphere-filtered one (both must give identical pixels). */
int      rt3_debug_force_plain_mode_r(rt3_ctx* ctx, int on);
/* Debug switch used by the parity tests and the fuzzers only: non-zero makes rt3_render_path* take k_trace_brute, the
 * UNFILTERED Mode-X kernel (every ray against every primitive in index order, no bounding spheres, no matrix cores) —
 * the on-GPU arbiter for the candidate filters.  Same effect: environment variable RT3_BRUTE=1. */
int      rt3_debug_force_brute(rt3_ctx* ctx, int on);
/* Debug switch (tests, A/B): non-zero makes the tiled matrix-filter kernel scan one row per primitive (the flat filter) instead of the
 * two-level filter's group rows.  Same pixels.  Same effect: environment variable RT3_NO_GROUPS=1. */
int      rt3_debug_force_flat_filter(rt3_ctx* ctx, int on);
int      rt3_debug_arith(rt3_ctx* ctx, const float* a, const float* b, uint32_t n, float* div, float* sq, float* fm,
                         float* cs, float* sn, float* sk3, uint32_t* pk);
/* Debug probe used by the tests only: builds the strip lists of the current scene (sphere-only, <= 512 spheres) for this camera and
 * these params and downloads them: n_groups x n_blocks words, group g = owned pixels 64 g .. 64 g + 63, bit b of word k of a group =
 * sphere 32 k + b may be met by a primary ray of the group.  RT3_E_ARG (with n_groups / n_blocks set) if capacity_words is too small. */
int      rt3_debug_primary_lists(rt3_ctx* ctx, const rt3_camera* cam, const rt3_params* p, uint32_t* out_masks, uint64_t capacity_words,
                                 uint32_t* n_groups, uint32_t* n_blocks);
/* Debug probe used by the tests only (no device needed): the counter-hash table k_trace_mfma32's render form builds in LDS, computed on the host by the
 * function the kernel fills it with.  Writes min(rows, capacity_rows) rows of 4 words — row d, word k = hash(1 + 8 (d + 1) + k), the inner hash of
 * the random numbers a path of depth d draws when it scatters — and returns rows, the depth below which shade_lane reads the table. */
uint32_t rt3_debug_ctr_table(uint32_t* out, uint32_t capacity_rows);

#ifdef __cplusplus
}
#endif
#endif /* RT3_H */
