// device_stubs.cpp — the device half of the C ABI (raytracer-3_amd/csrc/rt3_device.hip, for the scene calls rt3_scene.hip and, for the post-process calls,
// rt3_denoise.hip, rt3_display.hip and rt3_display_sequence.hip) as "no device" stubs, for the SANITIZER BUILD ONLY
// (make -C raytracer-3_amd asan): the host code under test — rt3_host.cpp, SceneParser.cpp, HostApi.cpp, Main.cpp — is compiled with g++
// -fsanitize=address,undefined and linked against these instead of librt3hip.so, so that it runs on a machine without a GPU and without the
// HIP runtime inside the sanitizer.  Nothing in the product links this file; every entry point fails the way the library does when no
// device is present (rt3_create returns NULL, the rest RT3_E_DEVICE).
#include "rt3.h"

extern "C" {
uint32_t rt3_abi_version(void) { return RT3_ABI_VERSION; }
rt3_ctx* rt3_create(int) { return nullptr; }
void rt3_destroy(rt3_ctx*) {}
const char* rt3_last_error(const rt3_ctx*) { return "sanitizer build: no HIP device (tools/asan/device_stubs.cpp)"; }
int rt3_set_sample_storage_cap(rt3_ctx*, uint64_t) { return RT3_E_DEVICE; }
int rt3_set_mesh(rt3_ctx*, const rt3_gface*, uint32_t, const float*, uint32_t, const rt3_material*) { return RT3_E_DEVICE; }
int rt3_mesh_begin(rt3_ctx*, uint32_t, uint32_t) { return RT3_E_DEVICE; }
int rt3_mesh_put(rt3_ctx*, const rt3_gface*, uint32_t, const float*, uint32_t, uint32_t, uint32_t) { return RT3_E_DEVICE; }
int rt3_mesh_sphere(rt3_ctx*, const float*, float, uint32_t, uint32_t, const float*, uint32_t, uint32_t) { return RT3_E_DEVICE; }
int rt3_mesh_commit(rt3_ctx*, const rt3_material*) { return RT3_E_DEVICE; }
int rt3_mesh_download(rt3_ctx*, rt3_gface*, float*) { return RT3_E_DEVICE; }
int rt3_set_spheres(rt3_ctx*, const float*, const rt3_material*, uint32_t) { return RT3_E_DEVICE; }
int rt3_update_spheres(rt3_ctx*, const float*, uint32_t) { return RT3_E_DEVICE; }
int rt3_update_spheres_device(rt3_ctx*, const void*, uint32_t, void*) { return RT3_E_DEVICE; }
int rt3_update_mesh(rt3_ctx*, const rt3_gface*, const float*, uint32_t) { return RT3_E_DEVICE; }
int rt3_update_mesh_device(rt3_ctx*, const void*, const void*, uint32_t, void*) { return RT3_E_DEVICE; }
int rt3_set_spheres_device(rt3_ctx*, const void*, const void*, uint32_t, void*) { return RT3_E_DEVICE; }
int rt3_set_mesh_device(rt3_ctx*, const void*, uint32_t, const void*, uint32_t, const void*, void*) { return RT3_E_DEVICE; }
int rt3_debug_sphere_build(rt3_ctx*, float*, uint32_t*, uint32_t*) { return RT3_E_DEVICE; }     // (rt3_debug_sphere_plan is host code: csrc/rt3_host.cpp)
int rt3_regroup(rt3_ctx*, uint32_t) { return RT3_E_DEVICE; }
int rt3_regroup_device(rt3_ctx*, uint32_t, void*) { return RT3_E_DEVICE; }
int rt3_debug_group_order(rt3_ctx*, uint32_t, uint32_t*, uint64_t, uint32_t*) { return RT3_E_DEVICE; }
int rt3_render(rt3_ctx*, const rt3_camera*, uint32_t, uint32_t, uint32_t*) { return RT3_E_DEVICE; }
int rt3_render_device(rt3_ctx*, const rt3_camera*, uint32_t, uint32_t, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_path(rt3_ctx*, const rt3_camera*, const rt3_params*, uint32_t*) { return RT3_E_DEVICE; }
int rt3_render_path_device(rt3_ctx*, const rt3_camera*, const rt3_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_path_range(rt3_ctx*, const rt3_camera*, const rt3_params*, uint32_t, uint32_t, uint32_t*) { return RT3_E_DEVICE; }
int rt3_render_path_range_device(rt3_ctx*, const rt3_camera*, const rt3_params*, uint32_t, uint32_t, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_path_adaptive(rt3_ctx*, const rt3_camera*, const rt3_params*, const rt3_adaptive_params*, uint32_t*, uint32_t*) { return RT3_E_DEVICE; }
int rt3_render_path_adaptive_device(rt3_ctx*, const rt3_camera*, const rt3_params*, const rt3_adaptive_params*, void*, void*, void*) { return RT3_E_DEVICE; }
int rt3_accum_download(rt3_ctx*, float*, float*, uint32_t*) { return RT3_E_DEVICE; }
int rt3_accum_upload(rt3_ctx*, const rt3_camera*, const rt3_params*, const float*, const float*, uint32_t) { return RT3_E_DEVICE; }
int rt3_gather_rows(rt3_ctx*, void*, rt3_ctx*, const void*, const rt3_params*, void*) { return RT3_E_DEVICE; }
int rt3_gather_plan(const rt3_params*, rt3_gather_copy*) { return RT3_E_DEVICE; }
void* rt3_stream(rt3_ctx*) { return nullptr; }
int rt3_synchronize(rt3_ctx*) { return RT3_E_DEVICE; }
void* rt3_device_alloc_words(rt3_ctx*, uint64_t) { return nullptr; }
void rt3_device_free(rt3_ctx*, void*) {}
int rt3_device_read_words(rt3_ctx*, const void*, uint64_t, uint32_t*) { return RT3_E_DEVICE; }
int rt3_get_stats(rt3_ctx*, rt3_stats*) { return RT3_E_DEVICE; }
int rt3_set_environment(rt3_ctx*, const float*, uint32_t) { return RT3_E_DEVICE; }      // (rt3_debug_environment_lookup is host code: csrc/rt3_host.cpp)
int rt3_set_environment_device(rt3_ctx*, const void*, uint32_t, void*) { return RT3_E_DEVICE; }
int rt3_clear_environment(rt3_ctx*) { return RT3_E_DEVICE; }
uint32_t rt3_environment_size(rt3_ctx*) { return 0; }
int rt3_debug_environment_table(rt3_ctx*, uint32_t*, uint64_t*, uint64_t, uint32_t*) { return RT3_E_DEVICE; }     // (rt3_debug_environment_sample is host code too)
int rt3_debug_light_table(rt3_ctx*, uint32_t*, uint64_t*, uint64_t, uint32_t*) { return RT3_E_DEVICE; }                 // (rt3_debug_light_sample is host code too)
int rt3_debug_force_plain_mode_r(rt3_ctx*, int) { return RT3_E_DEVICE; }
int rt3_debug_force_brute(rt3_ctx*, int) { return RT3_E_DEVICE; }
int rt3_debug_force_flat_filter(rt3_ctx*, int) { return RT3_E_DEVICE; }
int rt3_debug_arith(rt3_ctx*, const float*, const float*, uint32_t, float*, float*, float*, float*, float*, float*, uint32_t*) { return RT3_E_DEVICE; }
int rt3_debug_primary_lists(rt3_ctx*, const rt3_camera*, const rt3_params*, uint32_t*, uint64_t, uint32_t*, uint32_t*) { return RT3_E_DEVICE; }
uint32_t rt3_debug_ctr_table(uint32_t* out, uint32_t capacity_rows) {       // host code in the library too: the same table, from random_v1.glsl's hash
    const uint32_t rows = 64;
    for (uint32_t k = 0; out && k < (capacity_rows < rows ? capacity_rows : rows) * 4u; k++) {
        uint32_t x = 1u + 8u * ((k >> 2) + 1u) + (k & 3u);
        x += x << 10; x ^= x >> 6; x += x << 3; x ^= x >> 11; x += x << 15;
        out[k] = x;
    }
    return rows;
}
int rt3_intersect(rt3_ctx*, const rt3_ray*, uint32_t, float, rt3_hit*) { return RT3_E_DEVICE; }
int rt3_occluded(rt3_ctx*, const rt3_ray*, uint32_t, float, uint32_t*) { return RT3_E_DEVICE; }
int rt3_intersect_device(rt3_ctx*, const void*, uint32_t, float, void*, void*) { return RT3_E_DEVICE; }
int rt3_occluded_device(rt3_ctx*, const void*, uint32_t, float, void*, void*) { return RT3_E_DEVICE; }
int rt3_radiance(rt3_ctx*, const rt3_ray*, const uint32_t*, uint32_t, const rt3_radiance_params*, float*) { return RT3_E_DEVICE; }
int rt3_radiance_device(rt3_ctx*, const void*, const void*, uint32_t, const rt3_radiance_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_lens_rays(rt3_ctx*, const rt3_lens*, const rt3_params*, uint32_t, uint32_t, rt3_ray*) { return RT3_E_DEVICE; }     // (rt3_debug_lens_ray / rt3_lens_look_at are host code)
int rt3_lens_rays_device(rt3_ctx*, const rt3_lens*, const rt3_params*, uint32_t, uint32_t, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_lens(rt3_ctx*, const rt3_lens*, const rt3_params*, uint32_t, uint32_t, float*) { return RT3_E_DEVICE; }
int rt3_render_lens_device(rt3_ctx*, const rt3_lens*, const rt3_params*, uint32_t, uint32_t, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_lens_aov(rt3_ctx*, const rt3_lens*, const rt3_params*, rt3_aov*) { return RT3_E_DEVICE; }
int rt3_render_lens_aov_device(rt3_ctx*, const rt3_lens*, const rt3_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_camera_rays(rt3_ctx*, const rt3_camera*, const rt3_params*, uint32_t, uint32_t, rt3_ray*) { return RT3_E_DEVICE; }
int rt3_camera_rays_device(rt3_ctx*, const rt3_camera*, const rt3_params*, uint32_t, uint32_t, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_aov(rt3_ctx*, const rt3_camera*, const rt3_params*, rt3_aov*) { return RT3_E_DEVICE; }
int rt3_render_aov_device(rt3_ctx*, const rt3_camera*, const rt3_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_aov_specular(rt3_ctx*, const rt3_camera*, const rt3_params*, const rt3_aov_chain_params*, rt3_aov*) { return RT3_E_DEVICE; }     // (rt3_debug_aov_bounce is host code)
int rt3_render_aov_specular_device(rt3_ctx*, const rt3_camera*, const rt3_params*, const rt3_aov_chain_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_render_lens_aov_specular(rt3_ctx*, const rt3_lens*, const rt3_params*, const rt3_aov_chain_params*, rt3_aov*) { return RT3_E_DEVICE; }
int rt3_render_lens_aov_specular_device(rt3_ctx*, const rt3_lens*, const rt3_params*, const rt3_aov_chain_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_accum_resolve(rt3_ctx*, float*) { return RT3_E_DEVICE; }
int rt3_accum_resolve_device(rt3_ctx*, void*, void*) { return RT3_E_DEVICE; }
int rt3_denoise(rt3_ctx*, uint32_t, uint32_t, const float*, const rt3_aov*, const rt3_denoise_params*, float*) { return RT3_E_DEVICE; }
int rt3_denoise_device(rt3_ctx*, uint32_t, uint32_t, const void*, const void*, const rt3_denoise_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_denoise_temporal(rt3_ctx*, uint32_t, uint32_t, const rt3_camera*, const float*, const rt3_aov*, const rt3_camera*, const rt3_history*,
                         const rt3_temporal_params*, float*, rt3_history*) { return RT3_E_DEVICE; }
int rt3_denoise_temporal_device(rt3_ctx*, uint32_t, uint32_t, const rt3_camera*, const void*, const void*, const rt3_camera*, const void*,
                                const rt3_temporal_params*, void*, void*, void*) { return RT3_E_DEVICE; }
int rt3_motion(rt3_ctx*, uint32_t, uint32_t, const rt3_camera*, const rt3_aov*, const float*, uint32_t, const float*, uint32_t, float*) { return RT3_E_DEVICE; }
int rt3_motion_device(rt3_ctx*, uint32_t, uint32_t, const rt3_camera*, const void*, const void*, uint32_t, const void*, uint32_t, void*, void*) { return RT3_E_DEVICE; }
int rt3_denoise_temporal_motion(rt3_ctx*, uint32_t, uint32_t, const rt3_camera*, const float*, const rt3_aov*, const rt3_camera*, const rt3_history*,
                                const float*, const rt3_temporal_params*, float*, rt3_history*) { return RT3_E_DEVICE; }
int rt3_denoise_temporal_motion_device(rt3_ctx*, uint32_t, uint32_t, const rt3_camera*, const void*, const void*, const rt3_camera*, const void*,
                                       const void*, const rt3_temporal_params*, void*, void*, void*) { return RT3_E_DEVICE; }
int rt3_denoise_temporal_optic(rt3_ctx*, uint32_t, uint32_t, const rt3_lens*, const float*, const rt3_aov*, const rt3_lens*, const rt3_history*,
                               const float*, const rt3_temporal_params*, float*, rt3_history*) { return RT3_E_DEVICE; }     // (rt3_debug_turns / rt3_debug_optic_pixel are host code)
int rt3_denoise_temporal_optic_device(rt3_ctx*, uint32_t, uint32_t, const rt3_lens*, const void*, const void*, const rt3_lens*, const void*,
                                      const void*, const rt3_temporal_params*, void*, void*, void*) { return RT3_E_DEVICE; }
int rt3_motion_optic(rt3_ctx*, uint32_t, uint32_t, const rt3_lens*, const rt3_aov*, const float*, uint32_t, const float*, uint32_t, float*) { return RT3_E_DEVICE; }
int rt3_motion_optic_device(rt3_ctx*, uint32_t, uint32_t, const rt3_lens*, const void*, const void*, uint32_t, const void*, uint32_t, void*, void*) { return RT3_E_DEVICE; }
int rt3_display(rt3_ctx*, uint32_t, uint32_t, const float*, const rt3_display_params*, uint32_t*) { return RT3_E_DEVICE; }     // (rt3_debug_display_bin / _gain / _pixel / _srgb_table are host code)
int rt3_display_device(rt3_ctx*, uint32_t, uint32_t, const void*, const rt3_display_params*, void*, void*) { return RT3_E_DEVICE; }
int rt3_debug_display_state(rt3_ctx*, uint32_t*, uint32_t*, float*) { return RT3_E_DEVICE; }
int rt3_display_sequence(rt3_ctx*, uint32_t, uint32_t, const float*, const rt3_display_sequence_params*, const rt3_exposure*, rt3_exposure*, uint32_t*) { return RT3_E_DEVICE; }     // (rt3_debug_exposure_step / rt3_debug_bloom are host code)
int rt3_display_sequence_device(rt3_ctx*, uint32_t, uint32_t, const void*, const rt3_display_sequence_params*, const void*, void*, void*, void*) { return RT3_E_DEVICE; }
int rt3_debug_display_bloom(rt3_ctx*, float*, float*, uint64_t, uint32_t*, uint32_t*) { return RT3_E_DEVICE; }
int rt3_set_texture(rt3_ctx*, uint32_t, const float*, uint32_t, uint32_t, uint32_t) { return RT3_E_DEVICE; }     // (rt3_debug_texture_lookup / _sphere_uv / _face_uv are host code)
int rt3_set_texture_device(rt3_ctx*, uint32_t, const void*, uint32_t, uint32_t, uint32_t, void*) { return RT3_E_DEVICE; }
int rt3_clear_textures(rt3_ctx*) { return RT3_E_DEVICE; }
int rt3_texture_size(rt3_ctx*, uint32_t, uint32_t*, uint32_t*, uint32_t*) { return RT3_E_DEVICE; }
int rt3_bind_sphere_textures(rt3_ctx*, const uint32_t*, uint32_t) { return RT3_E_DEVICE; }
int rt3_bind_sphere_textures_device(rt3_ctx*, const void*, uint32_t, void*) { return RT3_E_DEVICE; }
int rt3_bind_mesh_textures(rt3_ctx*, const uint32_t*, const float*, uint32_t) { return RT3_E_DEVICE; }
int rt3_bind_mesh_textures_device(rt3_ctx*, const void*, const void*, uint32_t, void*) { return RT3_E_DEVICE; }
// (rt3_rows_owned / rt3_row_of_local are pure host arithmetic that happens to live in rt3_device.hip)
uint32_t rt3_rows_owned(const rt3_params* p) {
    uint32_t n = 0;
    for (uint32_t y = 0; y < p->height; y++) n += (p->tile_count <= 1 || ((y / p->tile_rows) % p->tile_count) == p->tile_index) ? 1u : 0u;
    return n;
}
uint32_t rt3_row_of_local(const rt3_params* p, uint32_t local_row) {
    if (p->tile_count <= 1) return local_row;
    return ((local_row / p->tile_rows) * p->tile_count + p->tile_index) * p->tile_rows + local_row % p->tile_rows;
}
}
