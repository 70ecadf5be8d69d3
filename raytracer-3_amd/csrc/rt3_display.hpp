// rt3_display.hpp — what rt3_display_sequence.hip needs of the display transform (rt3_display.hip): its first and its
// last step, between which a sequence call puts a gain kernel of its own.
#pragma once

// What the two steps read.  state: rt3disp::kStateWords words of the context (hist[512], dark, n, the gain's bits, a pad), or nullptr without
// auto-exposure.
struct DisplayLaunch {
    uint32_t npix;                          // width * height, 1 .. 2^26
    uint32_t curve, transfer;
    bool auto_exposure;
    float exposure, white;
    const void* rgba;                       // npix float4
    void* out;                              // npix uint32
    uint32_t* state;
};
// The state zeroed on `stream` and k_display_histogram (auto_exposure only).
hipError_t display_histogram_launch(const DisplayLaunch& L, hipStream_t stream);
// k_display_map, which with auto_exposure reads the gain from word kBins + 2 of the state and without it takes the uniform gain `exposure`.
hipError_t display_map_launch(const DisplayLaunch& L, hipStream_t stream);
