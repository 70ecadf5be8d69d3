// rt3_denoise.hpp — what rt3_device.hip needs of the denoiser (rt3_denoise.hip): its launchers.
#pragma once
#include "rt3.h"

// One rt3_denoise_device call once its arguments have been checked: k_denoise_prepare, k_denoise_moments and `iterations` a-trous passes on
// `stream`.  scratch: 3 * width * height float4 plus width * height floats (the two (I, v) planes, the guide plane, the depth slopes).
struct DenoiseLaunch {
    uint32_t width, height, iterations, normal_power;
    float sigma_l, sigma_z;
    const void* colour;                     // width * height float4
    const void* aov;                        // width * height rt3_aov (3 float4 each)
    void* out;                              // width * height float4
    float4* scratch;
};
hipError_t denoise_launch(const DenoiseLaunch& L, hipStream_t stream);

// One rt3_denoise_temporal_device call once its arguments have been checked: k_temporal_reproject, k_denoise_moments<true> and the passes,
// pass 0 also writing the history colour.  The same scratch as denoise_launch.  The per-call constants of the projection into the previous
// camera are computed by the caller in f32 in the order given there.
struct TemporalLaunch {
    DenoiseLaunch base;
    float cam[12];                          // this frame's rt3_camera: origin, horizontal, vertical, lower_left_corner
    float prev_o[3], prev_l[3];             // o' and L = llc' - o'
    float prev_n[3], a_u[3], a_v[3];        // n = h x v, a_u, a_v
    float ln;                               // L . n
    uint32_t has_prev, same_cam;            // a previous frame; *prev_cam == *cam byte for byte
    float alpha, moments_alpha, depth_tolerance, normal_tolerance;
    const void* prev_history;               // width * height rt3_history (3 float4 each), or nullptr without has_prev
    void* out_history;                      // width * height rt3_history
    const void* motion;                     // width * height float4 (m, moved) as motion_launch writes them, or nullptr
    const rt3_lens* lens;                   // nullptr: the camera above.  Else a lens frame: this frame's lens and, with has_prev,
    const rt3_lens* prev_lens;              // the previous one, of the same model; the camera fields above are not read
};
hipError_t temporal_launch(const TemporalLaunch& L, hipStream_t stream);

// One rt3_motion_device call once its arguments have been checked: k_motion on `stream`.  A class whose prev_* pointer is
// nullptr did not move; the counts bound every gather (a face index >= n_faces, a sphere index >= n_sph and a vertex index >= n_verts are
// never followed).
struct MotionLaunch {
    uint32_t width, height;
    float cam[12];                          // this frame's rt3_camera
    const rt3_lens* lens;                   // nullptr: the camera.  Else this frame's lens, and cam is not read
    const void* aov;                        // width * height rt3_aov
    const void* sph;                        // n_sph float4 (C, r): the records rt3_set_spheres took
    const float* sph_invr;                  // n_sph reciprocal radii
    const void* prev_sph;                   // n_sph float4 (C', r'), or nullptr
    const void* gfaces;                     // n_faces rt3_gface: the merged faces
    const void* verts;                      // n_verts float4: the merged vertices
    const void* prev_verts;                 // n_verts float4, or nullptr
    uint32_t n_sph, n_faces, n_verts;
    void* out;                              // width * height float4
};
hipError_t motion_launch(const MotionLaunch& L, hipStream_t stream);
