// rt3_denoise.hpp — what rt3_device.hip needs of the denoiser (rt3_denoise.hip): its launcher.
#pragma once

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
