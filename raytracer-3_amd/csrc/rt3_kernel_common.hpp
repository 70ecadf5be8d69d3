// rt3_kernel_common.hpp — constants, arithmetic helpers (hash RNG, sky, pixel packing, sin/cos), Mode-X launch arguments and start_path()
// No kernel.  Included by rt3_device.hip (all of it) and by rt3_scene.hip (the constants and the arithmetic helpers its kernels use), gfx950 only.
#pragma once

namespace {

constexpr int      kBlock       = 256;     // 4 wavefronts of 64
constexpr int      kCandSlots   = 16;      // deferred sphere candidates per lane (LDS), flushed when full
constexpr uint32_t kWorkChunk   = 256;     // samples a wave takes from the global queue per atomic
constexpr uint32_t kSphLdsMax   = 2048;    // spheres mirrored in LDS for the exact-evaluation gathers (32 KiB)
constexpr uint32_t kModeRTile   = 512;     // faces per LDS tile in k_mode_r (32 KiB)

// filler for the tail of a sphere tile: r^2 = -1e30 makes the discriminant negative for every ray
#define kPadSphere make_float4(0.0f, 0.0f, 0.0f, -1e30f)

struct CamDev { float ox, oy, oz, hx, hy, hz, vx, vy, vz, lx, ly, lz; };

// ------------------------------------------------------------------------------------------------------
// Small device helpers
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// dot3 of SequentialRenderer.cpp:32-33 / glm::dot: unfused, left to right.
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return ax * bx + ay * by + az * bz;
}
// Mode-X dot: z*z' + (y*y' + x*x') as two fused multiply-adds.
__device__ __forceinline__ float dotf(float ax, float ay, float az, float bx, float by, float bz) {
    return fma_(az, bz, fma_(ay, by, ax * bx));
}
__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
// number of set bits of a 64-bit lane mask below the calling lane (exclusive prefix count)
__device__ __forceinline__ uint32_t prefix_count(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// n / d for a divisor fixed per launch: multiply-high by a precomputed magic (branch-free round-up method of
// Granlund & Montgomery as used by libdivide); exact for every 32-bit n.  d == 1 is encoded as shift == 0xFFFFFFFF.
struct FastDiv { uint32_t magic, shift; };
__device__ __forceinline__ uint32_t fdiv(uint32_t n, FastDiv f) {
    if (f.shift == 0xFFFFFFFFu) return n;                           // wave-uniform
    const uint32_t q = __umulhi(f.magic, n);
    return (((n - q) >> 1) + q) >> f.shift;
}

// random_v1.glsl:22-31, :37-52
__host__ __device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
    x += x << 10; x ^= x >> 6; x += x << 3; x ^= x >> 11; x += x << 15;
    return x;
}
__device__ __forceinline__ uint32_t hash2(uint32_t a, uint32_t b) { return hash_u32(a ^ hash_u32(b)); }
__device__ __forceinline__ float u01(uint32_t m) { return __uint_as_float((m & 0x007FFFFFu) | 0x3F800000u) - 1.0f; }
__device__ __forceinline__ float rnd(uint32_t base, uint32_t ctr) { return u01(hash2(base, ctr)); }
// Counter-hash table of k_trace_mfma32's render form (built in its prologue, read by shade_lane): row d holds hash_u32(1 + 8 (d + 1) + k), k = 0..3 —
// the inner hashes of the rnd(base, ctr + k) a path of depth d draws when it scatters.  Paths at or beyond the cap compute them.
constexpr uint32_t kCtrDepthCap = 64;
constexpr uint32_t kCtrTableBytes = kCtrDepthCap * 16;
__host__ __device__ __forceinline__ uint32_t ctr_table_word(uint32_t k) { return hash_u32(1u + 8u * ((k >> 2) + 1u) + (k & 3u)); }   // word k of the table: row k / 4, column k % 4

// sky gradient, SequentialRenderer.cpp:105-107 (float form of raytracer_v3.glsl:139-141; same bits)
__device__ __forceinline__ void sky(float dx, float dy, float dz, float& r, float& g, float& b) {
    const float len = __builtin_sqrtf(dot3(dx, dy, dz, dx, dy, dz));
    const float uy = dy / len;
    const float t = 0.5f * (uy + 1.0f);
    const float a = 1.0f - t;
    r = a * 1.0f + t * 0.5f;
    g = a * 1.0f + t * 0.7f;
    b = a * 1.0f + t * 1.0f;
}
// Environment map lookup (rt3.h): the cube-map face of the direction's major axis, then a bilinear read inside that face, clamped to
// its edge.  Every operation is an IEEE f32 add, subtract, multiply, divide, compare or floor, rounded on its own (no fma_: tests/environment_ref.py and
// rt3_debug_environment_lookup restate it bit for bit).  env_axis: one in-face coordinate c of major-axis length m -> the two texel indices and the weight.
// A NaN floor becomes -1 before the conversion, so whatever the direction holds the four 16-byte loads stay inside the map.
__device__ __forceinline__ void env_axis(float c, float m, uint32_t n, uint32_t& i0, uint32_t& i1, float& w) {
    const float q = c / m;
    const float u = q * 0.5f + 0.5f;
    const float f = u * (float)n - 0.5f;
    const float f0 = __builtin_floorf(f);
    w = f - f0;
    const int k = (int)__builtin_fminf(__builtin_fmaxf(f0, -1.0f), (float)n - 1.0f);
    i0 = (uint32_t)(k > 0 ? k : 0);
    i1 = (uint32_t)(k + 1 < (int)n - 1 ? k + 1 : (int)n - 1);
}
__device__ __forceinline__ void env_lookup(const float4* __restrict__ env, uint32_t n, float x, float y, float z, float& r, float& g, float& b) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y), az = __builtin_fabsf(z);
    uint32_t f; float m, sc, tc;
    if (ax >= ay && ax >= az) { f = x < 0.0f ? 1u : 0u; m = ax; sc = x < 0.0f ? z : -z; tc = -y; }
    else if (ay >= az)        { f = y < 0.0f ? 3u : 2u; m = ay; sc = x; tc = y < 0.0f ? -z : z; }
    else                      { f = z < 0.0f ? 5u : 4u; m = az; sc = z < 0.0f ? -x : x; tc = -y; }
    uint32_t i0, i1, j0, j1; float wx, wy;
    env_axis(sc, m, n, i0, i1, wx);
    env_axis(tc, m, n, j0, j1, wy);
    const float4* row0 = env + ((size_t)f * n + j0) * n;
    const float4* row1 = env + ((size_t)f * n + j1) * n;
    const float4 c00 = row0[i0], c10 = row0[i1], c01 = row1[i0], c11 = row1[i1];
    const float tr = c00.x + wx * (c10.x - c00.x), br = c01.x + wx * (c11.x - c01.x);
    const float tg = c00.y + wx * (c10.y - c00.y), bg = c01.y + wx * (c11.y - c01.y);
    const float tb = c00.z + wx * (c10.z - c00.z), bb = c01.z + wx * (c11.z - c01.z);
    r = tr + wy * (br - tr);
    g = tg + wy * (bg - tg);
    b = tb + wy * (bb - tb);
}
// glm::packUnorm4x8(vec4(1, b, g, r)), glm/detail/func_packing.inl:67-83
__device__ __forceinline__ uint32_t pack_channel(float c) {
    float m = c < 0.0f ? 0.0f : c;
    m = 1.0f < m ? 1.0f : m;
    return (uint32_t)(__builtin_roundf(m * 255.0f)) & 0xFFu;
}
__device__ __forceinline__ uint32_t pack_pixel(float r, float g, float b) {
    return 0xFFu | (pack_channel(b) << 8) | (pack_channel(g) << 16) | (pack_channel(r) << 24);
}

// (cos, sin)(2*pi*u), u in [0,1): quadrant + Taylor/Horner in fma
__device__ __forceinline__ void sincos2pi(float u, float& c_out, float& s_out) {
    const float a = u * 4.0f;
    const int k = (int)a;
    const float f = a - (float)k;
    const float x = f * 1.57079637f;
    const float x2 = x * x;
    float p = fma_(x2, -2.50521084e-8f, 2.75573192e-6f);
    p = fma_(x2, p, -1.98412698e-4f);
    p = fma_(x2, p, 8.33333333e-3f);
    p = fma_(x2, p, -1.66666667e-1f);
    const float s = fma_(x * x2, p, x);
    float q = fma_(x2, 2.08767570e-9f, -2.75573192e-7f);
    q = fma_(x2, q, 2.48015873e-5f);
    q = fma_(x2, q, -1.38888889e-3f);
    q = fma_(x2, q, 4.16666667e-2f);
    q = fma_(x2, q, -0.5f);
    const float c = fma_(x2, q, 1.0f);
    const int kk = k & 3;
    c_out = kk == 0 ? c : kk == 1 ? -s : kk == 2 ? -c : s;
    s_out = kk == 0 ? s : kk == 1 ? c : kk == 2 ? -s : -c;
}
__device__ __forceinline__ void unit_vector(float xi0, float xi1, float& x, float& y, float& z) {
    z = fma_(-2.0f, xi0, 1.0f);
    const float rr = fma_(-z, z, 1.0f);
    const float r = __builtin_sqrtf(rr > 0.0f ? rr : 0.0f);
    float c, s;
    sincos2pi(xi1, c, s);
    x = r * c;
    y = r * s;
}

// ------------------------------------------------------------------------------------------------------
// Mode X
// ------------------------------------------------------------------------------------------------------
struct Rgb { float r, g, b; };   // one radiance record of the sample storage (three dwords: a quarter less HBM traffic than float4)
// The form of a trace kernel: where its work items come from and where a finished one goes.  One template parameter of every trace kernel and of the
// refill helpers; each kernel static_asserts the forms it has, plan_trace (rt3_device.hip) is the one place that picks one.
//   Render     item = (sample, owned pixel) through the camera, shaded into the sample storage: rt3_render_path*, the first round of the adaptive render
//   RenderRef  the same with RT3_FLAG_REFERENCE_PRIMARY (the reference's unnormalised primary direction; face-only scenes): rt3_render_path*
//   Query      item = one of the caller's rays, the nearest hit or the occlusion word stored: rt3_intersect*, rt3_occluded*, the AOV pass
//   List       Render over a list of pixels (TraceArgs::active): the later rounds of rt3_render_path_adaptive*
//   Rays       item = (sample, one of the caller's rays), shaded as a render's (TraceArgs::ray_keys): rt3_radiance*
//   RenderEnv, ListEnv, RaysEnv   Render, List and Rays while an environment map is set (rt3_set_environment*): the same kernel with
//              ONE difference, the miss of shade_lane reads the map where the twin evaluates the sky.  Their launch argument is an EnvTraceArgs (below).
//   RenderEnvNee, RaysEnvNee      RenderEnv and RaysEnv under RT3_FLAG_ENV_SAMPLING: a Lambert scatter also draws a direction from the
//              map's sampling table and casts one shadow ray through the lane's own cast slot (shade_lane); the lane carries a NeePath, the launch
//              argument is a NeeTraceArgs (both below).  No list form: the adaptive render refuses the flag.
//   RenderLight, RaysLight        Render and Rays under RT3_FLAG_LIGHT_SAMPLING: a Lambert scatter also draws a point on an emissive
//              primitive from the emitters' sampling table and casts one shadow ray towards it through the lane's own cast slot; the lane carries a
//              LightPath, the launch argument is a LightTraceArgs (both below).  With or without a map: env_n == 0 there means none, and the miss then
//              evaluates the sky — a branch at run time, not two more forms.  No list form: the adaptive render refuses the flag.
//   RenderTex, ListTex, RaysTex   Render, List and Rays while the context is textured (rt3_bind_*_textures*): the same kernel with ONE
//              difference, shade_lane multiplies the material's rgb by the bound texture's texel where it has just fetched the material (tex_modulate,
//              below).  The launch argument is a TexTraceArgs (below).  With or without a map: env_n == 0 there means none, and the miss then evaluates
//              the sky — a branch at run time, as in the light forms.  (New forms go to the END of the enum: a kernel's name carries its form's number.)
enum class Form : uint32_t { Render, RenderRef, Query, List, Rays, RenderEnv, ListEnv, RaysEnv, RenderEnvNee, RaysEnvNee, RenderLight, RaysLight,
                             RenderTex, ListTex, RaysTex };
constexpr bool is_nee(Form f) { return f == Form::RenderEnvNee || f == Form::RaysEnvNee; }
constexpr bool is_light(Form f) { return f == Form::RenderLight || f == Form::RaysLight; }
constexpr bool is_tex(Form f) { return f == Form::RenderTex || f == Form::ListTex || f == Form::RaysTex; }
constexpr bool has_shadow(Form f) { return is_nee(f) || is_light(f); }                 // a lane's cast may be a shadow ray: no stock entry can hold one
constexpr bool is_env(Form f) { return f == Form::RenderEnv || f == Form::ListEnv || f == Form::RaysEnv || is_nee(f) || is_light(f) || is_tex(f); }
// The twin of an environment form, and every other form itself: what a kernel body and the refill helpers branch on.
constexpr Form base_form(Form f) {
    return f == Form::RenderEnv || f == Form::RenderEnvNee || f == Form::RenderLight || f == Form::RenderTex ? Form::Render
         : f == Form::ListEnv || f == Form::ListTex ? Form::List
         : f == Form::RaysEnv || f == Form::RaysEnvNee || f == Form::RaysLight || f == Form::RaysTex ? Form::Rays : f;
}
// Batched ray queries (the QUERY forms of the trace kernels; rt3_intersect* / rt3_occluded*): item k of a launch is ray k
// of the caller's rt3_ray[] (q_rays: two float4 per ray, origin, t_max | direction, pad); its result goes to q_out[k], an rt3_hit (16 bytes), or with
// q_occluded one word.  They share the places of fields only the path kernels read (the VALU scan's face bounds, the sample storage, the render
// flags), so that the layout of the struct — and with it the code of every path kernel — stays what it was.
struct TraceArgs {
    const float4* sph;       const float* sph_invr;  const float4* sph_mat;  const uint32_t* sph_kind;  uint32_t n_sph;
    const float4* tri;       const float4* tri_mat;  const uint32_t* tri_kind;
    union { const float4* tri_bound; const float4* q_rays; const uint32_t* prim_masks; };   // prim_masks: k_trace_mfma32's render form (sphere-only: no face bounds), below
    uint32_t n_tri;
    CamDev cam;
    float lens_radius, lux, luy, luz, lvx, lvy, lvz;
    uint32_t width, height, spp, max_depth, seed;
    union { uint32_t flags; uint32_t q_occluded; };
    uint32_t edge;
    FastDiv div_npix, div_width, div_edge, div_tile_rows;
    float t_min;
    uint32_t tile_rows, tile_index, tile_count;
    uint32_t npix;           // pixels owned by this shard
    uint32_t s0;             // first sample of this batch
    uint32_t total;          // npix * samples in this batch
    union { Rgb* rad; void* q_out; };   // per-sample radiance, [sample in batch][owned pixel], 12 B each | QUERY: the results
    // Centres the matrix filter's coordinates are taken about: the filter's margin is eps (|C|^2 + r^2 + |o|^2), so a scene far from the
    // world origin would otherwise drown in candidates.  Spheres: the median of their centres; faces: the centre of the vertices' box.
    float fcx, fcy, fcz;     // spheres (k_trace_mfma, the K = 32 pass of k_trace_mfma_tiled)
    float tcx, tcy, tcz;     // faces (the faces' pass of k_trace_mfma_tiled)
    // Spheres that nearly every ray is a candidate for (a ground sphere; a sphere around the middle of the scene) gain nothing from the
    // filter and cost the pair list 64 entries per ray cast each: they are tested directly, every lane its own ray, and their fragment
    // rows can never be candidates (sphere_direct_list, rt3_sphere_plan.hpp).  Matrix-filter kernels only.
    uint32_t n_direct; uint32_t direct[4];
    // Two-level filter of k_trace_mfma_tiled: with a group size G > 1 a row of the matrix filter is the bounding sphere of G
    // primitives, grouped in the order of a spatial median split (rt3_set_spheres / rt3_mesh_commit): *_grp holds the members' (cx, cy, cz, r^2)
    // records — the spheres themselves, the faces' bounding spheres — in GROUP order (row g = entries [g G, (g + 1) G)), *_perm the primitive
    // index of each (0xFFFFFFFF: padding; the direct spheres are in no group).  *_rows: rows the pass scans (= primitives when G is 1).
    const float4* sph_grp; const uint32_t* sph_perm; const float4* tri_grp; const uint32_t* tri_perm; uint32_t n_sph_rows, n_tri_rows;
    // Three levels (kSuper > 1): a row bounds kSuper consecutive LEAF groups; *_leaf holds the leaves' bounding spheres (cx, cy, cz, R_eff^2), which a
    // candidate row's rays are tested against in f32 before the leaves' members are.  n_*_leaves: leaf groups (= rows x kSuper).
    const float4* sph_leaf; const float4* tri_leaf; uint32_t n_sph_leaves, n_tri_leaves;
    const float4* sph_rowb; const float4* tri_rowb;                 // three-level filter: the rows' own bounds (C, R_eff^2) in f32, or null
    const float4* tri_rec;                                          // the faces' 64-byte records once more, in GROUP order (a leaf's 8 faces: 512 contiguous bytes)
    const float4* sph_topb; const float4* tri_topb; uint32_t n_sph_top;              // k_trace_levels: what the matrix cores scan (rows, or super-rows of 8 rows) and its bounds in f32
    // Strip lists of k_trace_mfma32's render form (rt3_primary_lists.hpp; they share the places of fields that kernel never reads): prim_masks holds, per
    // aligned group of 64 owned pixels, one bit per sphere row ([group][row block] dwords) — the spheres a primary ray of the group can meet — or null
    // (lists off); a restock whose groups list more than prim_list_max spheres sends its primary rays through the matrix filter instead.
    union { uint32_t n_tri_top; uint32_t prim_list_max; };
    uint32_t* pair_strips;   // [wave of the grid][kStripPairs]: candidate (ray lane, row) pairs set aside for the end of a pass (deferred member tests)
    uint32_t* work_counter;
    unsigned long long* cast_counter;
    // List form of a work item (the later rounds of rt3_render_path_adaptive*): non-null, item j is (sample s0 + j / npix, pixel
    // active[j % npix]) with npix = the length of the list, and the strip lists are off (prim_masks null).  Only the LIST instantiations of the trace
    // kernels read it.  It is the LAST field: every slot above is read by some render form, and a field behind them moves none of them.
    // Rays form of a work item (rt3_radiance*): item j is (sample s0 + j / npix, ray j % npix of q_rays) with npix = the number of rays;
    // ray_keys[ray] — or, null, the ray's index — takes the pixel index's place in the path's RNG base.  Only the RAYS instantiations read it, and they
    // have no list: it shares the list's place.  (A field of its own behind `active` moves no field either, but it moves the kernel arguments that follow
    // the struct, and the list forms, which load `active` next to them, changed their scalar register allocation: DESIGN.md 5.2l.)
    union { const uint32_t* active; const uint32_t* ray_keys; };
};
// The launch argument of the environment forms: TraceArgs with the map behind it.  A struct of their own, so that TraceArgs — and with it the argument
// layout and the code of every other kernel — stays what it was.  The helpers keep taking a TraceArgs&; shade_lane, the one reader,
// gets the map back with env_of().  env: 6 faces of env_n x env_n float4 texels (+X, -X, +Y, -Y, +Z, -Z; row 0 first), 1 <= env_n <= 2048.
struct EnvTraceArgs : TraceArgs { const float4* env; uint32_t env_n; uint32_t env_pad; };
// The launch argument of the sampling forms (RT3_FLAG_ENV_SAMPLING): EnvTraceArgs with the map's sampling table behind it, again a struct
// of its own.  nee_q: the cells' quantised weights, nee_cdf: their inclusive prefix sums, both [6 nee_m nee_m] in (face, row, column) order; the
// table's total is nee_cdf[nee_cells - 1], read from device memory (the host never waits for the build).
struct NeeTraceArgs : EnvTraceArgs { const uint32_t* nee_q; const uint64_t* nee_cdf; uint32_t nee_m; uint32_t nee_cells; };
// The launch argument of the light sampling forms (RT3_FLAG_LIGHT_SAMPLING): EnvTraceArgs (env_n == 0: no map is set) with the emitters'
// sampling table behind it, a struct of its own once more.  lt_q: the entries' quantised weights, lt_cdf: their inclusive prefix sums, both [lt_n], faces
// first and then spheres in the caller's order (lt_n = n_tri + n_sph); the total is lt_cdf[lt_n - 1], read from device memory.  lt_sph_cr: the spheres'
// (C, r) as the caller gave them — the law samples with r, the trace kernels keep r^2 and 1 / r.
struct LightTraceArgs : EnvTraceArgs { const uint32_t* lt_q; const uint64_t* lt_cdf; const float4* lt_sph_cr; uint32_t lt_n; uint32_t lt_pad; };
// Image textures (rt3.h "Image textures").  TexTable: what a lookup at a hit needs — the slot table (one 16-byte descriptor per slot:
// the texel pointer, W | H << 16, the wrap mode; a null pointer: an empty slot), the two binding arrays in the caller's primitive order (RT3_TEX_NONE:
// untextured; null: the class has no binding) and the faces' six uv floats.  The launch argument of the texture forms: EnvTraceArgs (env_n == 0: no map
// is set) with the table behind it, a struct of its own once more; k_aov_accumulate takes the table as an argument of its own.
struct TexTable { const uint4* slots; const uint32_t* sph_tex; const uint32_t* tri_tex; const float2* tri_uv; };
struct TexTraceArgs : EnvTraceArgs { TexTable tex; };
template <Form F> using trace_args = std::conditional_t<is_tex(F), TexTraceArgs, std::conditional_t<is_light(F), LightTraceArgs,
                                     std::conditional_t<is_nee(F), NeeTraceArgs, std::conditional_t<is_env(F), EnvTraceArgs, TraceArgs>>>>;
__device__ __forceinline__ const EnvTraceArgs& env_of(const TraceArgs& A) { return static_cast<const EnvTraceArgs&>(A); }   // only where A IS one: an environment form
__device__ __forceinline__ const NeeTraceArgs& nee_of(const TraceArgs& A) { return static_cast<const NeeTraceArgs&>(A); }   // only where A IS one: a sampling form
__device__ __forceinline__ const LightTraceArgs& light_of(const TraceArgs& A) { return static_cast<const LightTraceArgs&>(A); }   // only where A IS one: a light sampling form
__device__ __forceinline__ const TexTraceArgs& tex_of(const TraceArgs& A) { return static_cast<const TexTraceArgs&>(A); }         // only where A IS one: a texture form
// The shading rule of a textured hit (rt3.h): m.xyz *= texel for a flat, Lambert or metal primitive that is bound to a slot.  face: the hit is face idx
// (tri: the faces' records, four float4 each) at the point p = o + t d, else sphere idx with the unit outward normal n, before the flip.  The slot differs
// from lane to lane: its descriptor comes with one 16-byte vector load, then the four taps as four independent 16-byte loads behind one wait.  A slot the
// host would have refused (out of range, empty) leaves m alone: no address is formed from it.
__device__ __forceinline__ void tex_modulate(const TexTable& X, bool face, uint32_t idx, const float4* __restrict__ tri, float px, float py, float pz,
                                             float nx, float ny, float nz, uint32_t mk, float4& m) {
    const uint32_t* bind = face ? X.tri_tex : X.sph_tex;
    if (mk == RT3_MAT_DIELECTRIC || bind == nullptr) return;
    const uint32_t slot = bind[idx];
    if (slot >= RT3_TEX_MAX_TEXTURES) return;                       // (RT3_TEX_NONE among them)
    const uint4 d = X.slots[slot];
    const float4* texels = reinterpret_cast<const float4*>(((uint64_t)d.y << 32) | d.x);
    if (texels == nullptr) return;
    float u, v;
    if (face) {
        const float4 a = tri[(size_t)idx * 4 + 1], b = tri[(size_t)idx * 4 + 2], c = tri[(size_t)idx * 4 + 3];
        const float2 t1 = X.tri_uv[(size_t)idx * 3], t2 = X.tri_uv[(size_t)idx * 3 + 1], t3 = X.tri_uv[(size_t)idx * 3 + 2];
        const float p1[3] = { a.x, a.y, a.z }, p2[3] = { b.x, b.y, b.z }, p3[3] = { c.x, c.y, c.z }, p[3] = { px, py, pz };
        const float uv6[6] = { t1.x, t1.y, t2.x, t2.y, t3.x, t3.y };
        rt3tex::face_uv(p1, p2, p3, uv6, p, u, v);
    } else {
        rt3tex::sphere_uv(nx, ny, nz, u, v);
    }
    float r, g, b;
    rt3tex::lookup(texels, d.z & 0xFFFFu, d.z >> 16, d.w, u, v, r, g, b);
    m.x = m.x * r; m.y = m.y * g; m.z = m.z * b;
}

struct Path {
    float ox, oy, oz, dx, dy, dz;
    float tr, tg, tb, lr, lg, lb;
    uint32_t slot, base, depth;
    float tmax;              // QUERY forms: the ray's t_max (the path kernels never touch it)
};
// The lane state of the sampling forms (is_nee): a Path plus what a shadow ray in flight needs — it travels in the lane's own cast slot
// (origin and direction of P), so the continuation's direction waits in c*, the contribution a miss of the shadow ray adds per unit of map radiance in e*.
// nee: kNeeShadow, the cast in flight is the shadow ray; kNeeLambert, the path's most recent scatter was a Lambert scatter, whose light the shadow ray
// accounted for (a later miss adds nothing).  The helpers keep taking a Path&; shade_lane, the one reader, gets the rest back with nee_path().
struct NeePath : Path { float cx = 0.0f, cy = 0.0f, cz = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f; uint32_t nee = 0u; };
constexpr uint32_t kNeeShadow = 1u, kNeeLambert = 2u;
// The lane state of the light sampling forms (is_light): a NeePath — e* is then the contribution per unit of the light's radiance — plus
// the table entry of the light the shadow ray in flight was aimed at: the ray adds only where its nearest hit IS that primitive.
struct LightPath : NeePath { uint32_t light = 0u; };
template <Form F> using path_of = std::conditional_t<is_light(F), LightPath, std::conditional_t<is_nee(F), NeePath, Path>>;
__device__ __forceinline__ NeePath& nee_path(Path& P) { return static_cast<NeePath&>(P); }                                  // only where P IS one: a sampling form
__device__ __forceinline__ LightPath& light_path(Path& P) { return static_cast<LightPath&>(P); }                            // only where P IS one: a light sampling form

// The reference's plane + three-edge test of one face (SequentialRenderer.cpp:53-98; hit_vertex, raytracer_v4.glsl:116-153), in
// its own operation order.  n = (normal, n.p1) as k_commit_mesh stores it.
//   face_t       the ray parameter of the plane: (n.p1 - n.o) / n.d — Mode X, sign of n.o corrected — or, `literal`, the
//                reference's own (n.o + n.p1) / n.d (:70, sic), which only means the plane for an origin of 0; false if n.d == 0 (:56)
//   face_inside  the three edge functions at the point o + t d (:77-98)
__device__ __forceinline__ bool face_t(const float4 n, float ox, float oy, float oz, float dx, float dy, float dz, bool literal, float& t) {
    const float nd = dot3(dx, dy, dz, n.x, n.y, n.z);
    if (nd == 0.0f) return false;
    const float no = dot3(n.x, n.y, n.z, ox, oy, oz);
    t = (literal ? no + n.w : n.w - no) / nd;
    return true;
}
__device__ __forceinline__ bool face_inside(const float4 n, const float4 p1, const float4 p2, const float4 p3, float ox, float oy, float oz,
                                            float dx, float dy, float dz, float t) {
    const float hx = ox + t * dx, hy = oy + t * dy, hz = oz + t * dz;
    float ex, ey, ez, qx, qy, qz, cx, cy, cz;
    ex = p2.x - p1.x; ey = p2.y - p1.y; ez = p2.z - p1.z; qx = hx - p1.x; qy = hy - p1.y; qz = hz - p1.z;
    cx = ey * qz - qy * ez; cy = ez * qx - qz * ex; cz = ex * qy - qx * ey;
    if (!(-dot3(n.x, n.y, n.z, cx, cy, cz) >= 0.0f)) return false;
    ex = p3.x - p2.x; ey = p3.y - p2.y; ez = p3.z - p2.z; qx = hx - p2.x; qy = hy - p2.y; qz = hz - p2.z;
    cx = ey * qz - qy * ez; cy = ez * qx - qz * ex; cz = ex * qy - qx * ey;
    if (!(-dot3(n.x, n.y, n.z, cx, cy, cz) >= 0.0f)) return false;
    ex = p1.x - p3.x; ey = p1.y - p3.y; ez = p1.z - p3.z; qx = hx - p3.x; qy = hy - p3.y; qz = hz - p3.z;
    cx = ey * qz - qy * ez; cy = ez * qx - qz * ex; cz = ex * qy - qx * ey;
    return -dot3(n.x, n.y, n.z, cx, cy, cz) >= 0.0f;
}
// Both, with the vertices fetched only when t lies in [t_lo, t_hi) (STRICT) or [t_lo, t_hi].
template <bool STRICT>
__device__ __forceinline__ bool face_hit(const float4 n, const float4* __restrict__ f, float ox, float oy, float oz, float dx, float dy, float dz,
                                         float t_lo, float t_hi, bool literal, float& t_out) {
    float t;
    if (!face_t(n, ox, oy, oz, dx, dy, dz, literal, t)) return false;
    if (!(t >= t_lo && (STRICT ? t < t_hi : t <= t_hi))) return false;
    if (!face_inside(n, f[1], f[2], f[3], ox, oy, oz, dx, dy, dz, t)) return false;
    t_out = t;
    return true;
}
// Exact ray-sphere test of Mode X (hit_sphere, raytracer_v4.glsl:157-178, unit direction, the book's far-root rule):
// s = (centre, r^2); true with the accepted root in t when t_min < t.
__device__ __forceinline__ bool sphere_root(const float4 s, float ox, float oy, float oz, float dx, float dy, float dz, float t_min, float& t_out) {
    const float cx = s.x - ox, cy = s.y - oy, cz = s.z - oz;
    const float h = fma_(cz, dz, fma_(cy, dy, cx * dx));
    const float c = fma_(cz, cz, fma_(cy, cy, fma_(cx, cx, -s.w)));
    const float disc = fma_(h, h, -c);
    if (!((c < 0.0f) | ((disc > 0.0f) & (h > 0.0f)))) return false;
    const float sq = __builtin_sqrtf(disc);
    float t = h - sq;
    if (!(t > t_min)) t = h + sq;
    t_out = t;
    return t > t_min;
}

__device__ __forceinline__ uint32_t frame_row(const TraceArgs& A, uint32_t local_row) {
    if (A.tile_count <= 1) return local_row;
    const uint32_t lb = fdiv(local_row, A.div_tile_rows), in = local_row - lb * A.tile_rows;
    return (lb * A.tile_count + A.tile_index) * A.tile_rows + in;
}

// sample -> primary ray (raytracer_v4.glsl:190-214 with the jitter in pixel units), unit direction.
// REF (RT3_FLAG_REFERENCE_PRIMARY): the direction stays unnormalised, as SequentialRenderer.cpp:293 leaves it.
// Form::List: the list form of a work item (TraceArgs::active).  A compile-time choice, not a test of the pointer: the dense kernels' code stays what it was
// (a wave-uniform test cost two of them scratch, profiles/adaptive_kernel_resources.log).
// start_path_at: the part behind the index arithmetic — item `item` is sample s of the pixel (x, y) of the frame.  HS: hs is hash2(s, A.seed), worked
// out by the caller (refill_from_traced_stock, once per wave where the 64 items of a restock share their sample).
template <bool REF = false, bool HS = false>
__device__ __forceinline__ void start_path_at(const TraceArgs& A, uint32_t item, uint32_t s, uint32_t x, uint32_t y, uint32_t hs, Path& P) {
    const uint32_t base = hash2(y * A.width + x, HS ? hs : hash2(s, A.seed));
    float jx = 0.0f, jy = 0.0f;
    if (A.spp > 1) {
        const float xi0 = rnd(base, 1), xi1 = rnd(base, 2);
        if (A.edge != 0) {
            const uint32_t sy = fdiv(s, A.div_edge), sx = s - sy * A.edge;
            jx = ((float)sx + xi0) / (float)A.edge - 0.5f;
            jy = ((float)sy + xi1) / (float)A.edge - 0.5f;
        } else { jx = xi0 - 0.5f; jy = xi1 - 0.5f; }
    }
    const float u = ((float)x + jx) / ((float)A.width - 1.0f);
    const float v = ((float)(A.height - 1 - y) + jy) / ((float)A.height - 1.0f);
    const CamDev& c = A.cam;
    float rx = ((c.lx + u * c.hx) + v * c.vx) - c.ox;
    float ry = ((c.ly + u * c.hy) + v * c.vy) - c.oy;
    float rz = ((c.lz + u * c.hz) + v * c.vz) - c.oz;
    float ox = c.ox, oy = c.oy, oz = c.oz;
    if (A.lens_radius > 0.0f) {
        const float xi2 = rnd(base, 3), xi3 = rnd(base, 4);
        const float r = A.lens_radius * __builtin_sqrtf(xi2);
        float cs, sn;
        sincos2pi(xi3, cs, sn);
        const float a = r * cs, b = r * sn;
        const float fx = a * A.lux + b * A.lvx, fy = a * A.luy + b * A.lvy, fz = a * A.luz + b * A.lvz;
        ox = ox + fx; oy = oy + fy; oz = oz + fz;
        rx = rx - fx; ry = ry - fy; rz = rz - fz;
    }
    P.ox = ox; P.oy = oy; P.oz = oz;
    if (REF) { P.dx = rx; P.dy = ry; P.dz = rz; }
    else {
        const float inv = 1.0f / __builtin_sqrtf(dot3(rx, ry, rz, rx, ry, rz));
        P.dx = rx * inv; P.dy = ry * inv; P.dz = rz * inv;
    }
    P.tr = P.tg = P.tb = 1.0f;
    P.lr = P.lg = P.lb = 0.0f;
    P.slot = item; P.base = base; P.depth = 0;
}
template <Form F>
__device__ __forceinline__ void start_path(const TraceArgs& A, uint32_t item, Path& P) {
    static_assert(F == Form::Render || F == Form::RenderRef || F == Form::List, "start_path: the forms whose items are samples of pixels");
    const uint32_t sb = fdiv(item, A.div_npix);
    uint32_t pix = item - sb * A.npix;
    if constexpr (F == Form::List) pix = A.active[pix];
    const uint32_t s = A.s0 + sb;
    const uint32_t lrow = fdiv(pix, A.div_width), x = pix - lrow * A.width;
    const uint32_t y = frame_row(A, lrow);
    start_path_at<F == Form::RenderRef>(A, item, s, x, y, 0u, P);
}

}  // namespace
