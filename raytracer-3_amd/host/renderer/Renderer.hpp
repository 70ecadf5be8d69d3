// renderer/Renderer.hpp — the backend boundary of the reference (src/lib/renderer/Renderer.hpp:34-63): an abstract
// Renderer with prerender() / render() and the link-time factory initialize_renderer().  HipRenderer is the
// MI355X backend; it drives librt3hip.so through the C ABI of include/rt3.h.
#ifndef RT3_HOST_RENDERER_HPP
#define RT3_HOST_RENDERER_HPP
#include <cstdint>
#include <vector>
#include "camera/Camera.hpp"
#include "entities/RenderEntity.hpp"
#include "tools/Array.hpp"
#include "Vertex.hpp"
#include "rt3.h"

namespace RayTracer {
class Renderer {
public:
    virtual ~Renderer() = default;
    virtual void prerender(const Tools::Array<ECS::RenderEntity*>& entities) = 0;
    virtual void render(Camera& camera) const = 0;
};

// The caller-owned state of a temporal denoising sequence (rt3_denoise_temporal*): the last frame's history records and camera; empty
// records = the first frame.
struct History {
    std::vector<rt3_history> records;
    rt3_camera camera{};
};
// The same for a sequence of lens frames (rt3_denoise_temporal_optic): the last frame's history records and lens.
struct LensHistory {
    std::vector<rt3_history> records;
    rt3_lens lens{};
};

// Mode-X knobs the reference API has no place for (spp / depth / seed ...); spp == 0 means Mode R.
struct PathOptions {
    uint32_t spp = 0, max_depth = 50, seed = 1, flags = 0;          // flags: RT3_FLAG_* of rt3.h; RT3_FLAG_ENV_SAMPLING needs set_environment() first, RT3_FLAG_LIGHT_SAMPLING excludes it
    float lens_radius = 0.0f, t_min = 0.001f;
    uint32_t tile_rows = 8;
};

class HipRenderer : public Renderer {
public:
    explicit HipRenderer(const std::vector<int>& devices = { 0 });
    ~HipRenderer() override;
    void prerender(const Tools::Array<ECS::RenderEntity*>& entities) override;   // flatten in entity order + upload
    void render(Camera& camera) const override;                                  // fills camera.get_frame().d()
    void configure(const PathOptions& options) { path = options; }
    // Mode X only: render() with path.spp as a budget (rt3_render_path_adaptive on every device shard).  Fills
    // camera.get_frame().d() and returns the samples each pixel received, a full frame, row 0 on top.  hdr(), aov() and the denoisers follow it
    // as they follow render().  With several devices every shard decides over its own rows (the count map may differ along row-block edges).
    std::vector<uint32_t> render_adaptive(Camera& camera, const rt3_adaptive_params& adaptive) const;
    void set_gpu_prerender(bool on) { gpu_prerender = on; }         // tessellate eprmf_gpu entities on the device (default: host)
    // scenes that are not entity lists (benchmark sphere fields)
    void set_spheres(const std::vector<float>& center_radius, const std::vector<rt3_material>& materials);
    void set_mesh(const std::vector<rt3_gface>& faces, const std::vector<float>& vertices_xyzw, const std::vector<rt3_material>& face_materials);
    // the same scene with new positions (rt3_update_spheres / rt3_update_mesh): counts, materials and the grouping stay; faces: empty keeps
    // the indices, normals and colours, else the mesh's face count of records (new normals)
    void update_spheres(const std::vector<float>& center_radius);
    void update_mesh(const std::vector<float>& vertices_xyzw, const std::vector<rt3_gface>& faces = {});
    // the classes that have a scene get the group order of a full upload back after updates (rt3_regroup): nothing a render returns changes
    void regroup(bool spheres = true, bool mesh = true);
    // Mode X: the cube map every ray that leaves the scene reads, on every device (rt3_set_environment): 6 faces of n_face x n_face texels,
    // 4 floats each (r, g, b, ignored), faces +X, -X, +Y, -Y, +Z, -Z, row 0 first; it stays until it is replaced or cleared
    void set_environment(const std::vector<float>& rgba, uint32_t n_face);
    void clear_environment();
    // Mode X: image textures on every device (rt3_set_texture, rt3_bind_*_textures).  A slot holds w x h texels of 4 floats (r, g, b,
    // ignored), row 0 on top, wrap RT3_TEX_REPEAT or RT3_TEX_CLAMP; a binding names one slot per primitive in the upload's order (RT3_TEX_NONE: none),
    // for faces with 6 uv floats each.  Slots stay until they are replaced; a binding goes with the next full upload of its class.  Empty slots: unbinds.
    void set_texture(uint32_t slot, const std::vector<float>& rgba, uint32_t w, uint32_t h, uint32_t wrap = RT3_TEX_REPEAT);
    void bind_sphere_textures(const std::vector<uint32_t>& slots);
    void bind_mesh_textures(const std::vector<uint32_t>& slots, const std::vector<float>& uv6);
    rt3_stats stats() const;                                                     // of device 0's last render
    // Mode X only, full frames (row 0 on top) assembled from the device shards: the first-hit AOVs of the current options (rt3_render_aov),
    // and the linear (r, g, b, 0) frame of the last render (rt3_accum_resolve)
    std::vector<rt3_aov> aov(Camera& camera) const;
    // ... and the specular-chain AOVs (rt3_render_aov_specular): every ray followed through glass and the metals `chain` admits to the
    // first rough surface; guides for denoise(width, height, colour, guides, params), not for the temporal denoisers or motion()
    std::vector<rt3_aov> aov_specular(Camera& camera, const rt3_aov_chain_params& chain) const;
    std::vector<float> hdr() const;
    // Mode X only: the linear frame of the last render denoised on device 0 (rt3_denoise), guided by aov(camera); (r, g, b, 0) per pixel
    std::vector<float> denoise(Camera& camera, const rt3_denoise_params& params) const;
    // Mode X only: the same frame through the temporal denoiser (rt3_denoise_temporal) with `history` as the previous frame's, which the
    // call replaces by this frame's; (r, g, b, 0) per pixel
    // motion: empty, or the plane motion() returned for this frame (rt3_denoise_temporal_motion): what moved keeps its history
    std::vector<float> denoise_temporal(Camera& camera, const rt3_temporal_params& params, History& history,
                                        const std::vector<float>& motion = {}) const;
    // Mode X only: the motion plane of the current scene on device 0 (rt3_motion), (mx, my, mz, moved) per pixel of aov(camera); the previous
    // frame's spheres (4 floats each) and merged vertices (xyzw), an empty vector for a class that did not move
    std::vector<float> motion(Camera& camera, const std::vector<float>& prev_center_radius, const std::vector<float>& prev_vertices_xyzw) const;
    // A linear (r, g, b, .) frame of the camera's size — hdr()'s, a denoiser's — through the display transform on device 0 (rt3_display): exposure,
    // tone curve, transfer function; fills camera.get_frame().d() with the words render() would pack
    void display(Camera& camera, const std::vector<float>& rgba, const rt3_display_params& params) const;
    // The same for one frame of a sequence (rt3_display_sequence): with auto-exposure the gain follows the sequence through `state` —
    // zeroed before the first frame, replaced by every call —, and params.bloom_levels adds a bloom pyramid before the tone curve
    void display_sequence(Camera& camera, const std::vector<float>& rgba, const rt3_display_sequence_params& params, rt3_exposure& state) const;
    // Mode X only: path-traced radiance along the caller's rays on device 0 (rt3_radiance), (r, g, b, 0) per ray: path.spp samples from sample_begin
    // on, path.max_depth, path.seed, path.t_min and the BLACK_BACKGROUND, ENV_SAMPLING and LIGHT_SAMPLING bits of path.flags; keys: empty (a ray's index is its key) or one per ray
    std::vector<float> radiance(const std::vector<rt3_ray>& rays, const std::vector<uint32_t>& keys = {}, uint32_t sample_begin = 0) const;
    // Mode X only: a whole lens frame of width x height on device 0 (rt3_render_lens), linear (r, g, b, 0) per pixel: path.spp samples,
    // path.max_depth, path.seed, path.t_min and the BLACK_BACKGROUND, ENV_SAMPLING and LIGHT_SAMPLING bits of path.flags; and its first-hit AOVs
    // (rt3_render_lens_aov).  A cube lens's frame (width N, height 6 N) is the array set_environment takes.
    std::vector<float> render_lens(const rt3_lens& lens, uint32_t width, uint32_t height) const;
    std::vector<rt3_aov> lens_aov(const rt3_lens& lens, uint32_t width, uint32_t height) const;
    std::vector<rt3_aov> lens_aov_specular(const rt3_lens& lens, uint32_t width, uint32_t height, const rt3_aov_chain_params& chain) const;   // (rt3_render_lens_aov_specular)
    // One frame of a sequence of lens frames through the temporal denoiser on device 0 (rt3_denoise_temporal_optic): colour and guides
    // are render_lens's and lens_aov's for `lens`; `history` is the previous frame's and is replaced by this frame's; motion: empty, or motion_lens's plane
    std::vector<float> denoise_temporal_lens(const rt3_lens& lens, uint32_t width, uint32_t height, const std::vector<float>& colour,
                                             const std::vector<rt3_aov>& guides, const rt3_temporal_params& params, LensHistory& history,
                                             const std::vector<float>& motion = {}) const;
    // The motion plane of the current scene on device 0 for a lens frame (rt3_motion_optic): guides are lens_aov's for `lens`; the previous arrays as motion()
    std::vector<float> motion_lens(const rt3_lens& lens, uint32_t width, uint32_t height, const std::vector<rt3_aov>& guides,
                                   const std::vector<float>& prev_center_radius, const std::vector<float>& prev_vertices_xyzw) const;
    // rt3_denoise on device 0 for frames the caller holds (a lens frame and its AOVs)
    std::vector<float> denoise(uint32_t width, uint32_t height, const std::vector<float>& colour, const std::vector<rt3_aov>& guides,
                               const rt3_denoise_params& params) const;
    size_t faces() const { return n_faces; }
    size_t spheres() const { return n_spheres; }

private:
    std::vector<rt3_ctx*> ctx;                      // one device context per GPU; frame rows are sharded over them
    PathOptions path;
    bool gpu_prerender = false;
    size_t n_faces = 0, n_spheres = 0;
    mutable uint32_t last_w = 0, last_h = 0;        // frame size of the last Mode-X render (hdr())
    rt3_params shard_params(uint32_t w, uint32_t h, uint32_t i) const;
};

Renderer* initialize_renderer();                    // Renderer.hpp:63 — always the HIP backend here
}  // namespace RayTracer
#endif
