// rt3_display_sequence.hpp — what rt3_device.hip needs of display sequences (rt3_display_sequence.hip): its launchers.
#pragma once
#include "rt3_display.hpp"

// One rt3_display_sequence_device call once its arguments have been checked, queued on `stream` with no host wait.
//   the exposure: with display.auto_exposure the state zeroed, k_display_histogram and k_display_gain_step (prev -> out_exposure, the gain left in
//   the state); without it k_exposure_given if there is an out_exposure;
//   bloom_levels == 0: k_display_map, one launch;
//   bloom_levels == L: k_bloom_down_first, L - 1 x k_bloom_down, L - 1 x k_bloom_up, k_display_map_bloom: 2 L launches.
// pyramid: rt3dseq::pyramid_texels(width, height, L) float4 texels, D_1 .. D_L one behind the other; after the call plane 1 holds U_1.
struct DisplaySequenceLaunch {
    DisplayLaunch display;                  // npix = width * height; state as for display_launch
    uint32_t width, height;
    uint32_t adapt_brighter, adapt_darker, bloom_levels;
    float bloom_threshold, bloom_intensity;
    const rt3_exposure* prev;               // device, or nullptr
    rt3_exposure* out_exposure;             // device, or nullptr; may be prev
    void* pyramid;                          // nullptr without bloom
};
hipError_t display_sequence_launch(const DisplaySequenceLaunch& S, hipStream_t stream);
// Tests only: B = up(U_1) / levels at w0 x h0 into `out` (w0 * h0 float4), from U_1 (w1 x h1 float4).
hipError_t bloom_plane_launch(const void* u1, uint32_t w1, uint32_t h1, void* out, uint32_t w0, uint32_t h0, uint32_t levels, hipStream_t stream);
