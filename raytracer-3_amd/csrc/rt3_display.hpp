// rt3_display.hpp — what rt3_device.hip needs of the display transform (rt3_display.hip): its launcher.
#pragma once

// One rt3_display_device call once its arguments have been checked.  Without auto-exposure: k_display_map on `stream` with the uniform gain
// `exposure`.  With it: the state zeroed on the stream, k_display_histogram, k_display_gain, then k_display_map reading the gain from the state —
// no host wait in between.  state: rt3disp::kStateWords words of the context (hist[512], dark, n, the gain's bits, a pad), or nullptr without the flag.
struct DisplayLaunch {
    uint32_t npix;                          // width * height, 1 .. 2^26
    uint32_t curve, transfer;
    bool auto_exposure;
    uint32_t trim_low, trim_high;
    float exposure, key, white;
    const void* rgba;                       // npix float4
    void* out;                              // npix uint32
    uint32_t* state;
};
hipError_t display_launch(const DisplayLaunch& L, hipStream_t stream);
// Its first and last steps on their own, for rt3_display_sequence.hip, which puts a gain kernel of its own between them: the state zeroed and
// k_display_histogram (auto_exposure only); k_display_map, which with auto_exposure reads the gain from word kBins + 2 of the state.
hipError_t display_histogram_launch(const DisplayLaunch& L, hipStream_t stream);
hipError_t display_map_launch(const DisplayLaunch& L, hipStream_t stream);
