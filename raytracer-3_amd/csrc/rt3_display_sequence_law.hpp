// rt3_display_sequence_law.hpp — the law of display sequences (rt3.h "Display sequences"), one statement for the device and the host:
// the exposure that follows a sequence (integers only) and the bloom pyramid (f32 operations rounded one by one; every file is compiled with
// -ffp-contract=off).  Included by rt3_display_sequence.hip (the kernels; the entry points' parameter check and the pyramid's size) and by
// rt3_host.cpp (rt3_debug_exposure_step / rt3_debug_bloom, the serial restatement the tests compare with tests/display_sequence_ref.py).
// The histogram, the trim, the curve and the transfer are rt3_display_law.hpp's.
#pragma once
#include <cstddef>
#include <cstdint>

#include "rt3_display_law.hpp"

namespace rt3dseq {

using namespace rt3disp;

constexpr uint32_t kMaxLevel = 511u << 19;                          // the last bin, in 2^-19 of a bin
constexpr uint32_t kMaxBloomLevels = 8;
constexpr uint32_t kMaxRate = 1024;

// ---- the exposure
// P_t of a histogram's trimmed sum: the quantity gain_from_sum forms.  t.n != 0.
RT3_HD uint32_t level_from_sum(const Trim& t, uint64_t s) { return (uint32_t)((s << 19) / t.m); }
// gain_from_sum's float expression of a level.
RT3_HD float gain_of_level(uint32_t level, float exposure, float key) {
    return exposure * (key / float_of((111u << 23) + level + (1u << 18)));
}
// One frame's move from `level` towards `target`: a share of the way, at least 1, never past the target.
RT3_HD uint32_t step_level(uint32_t level, uint32_t target, uint32_t brighter, uint32_t darker) {
    if (target == level) return level;
    const bool up = target > level;
    const uint64_t d = up ? target - level : level - target;
    const uint64_t share = (d * (up ? brighter : darker)) >> 10;    // rate <= 1024: share <= d
    const uint32_t step = (uint32_t)(share > 1u ? share : 1u);
    return up ? level + step : level - step;
}
// The state after a frame with n counted pixels and the target P_t (anything when n == 0).  prev_level, frames: the state before, frames == 0 where
// there is none; the level is read as at most kMaxLevel (the host form refuses a larger one before it gets here).
RT3_HD rt3_exposure exposure_next(uint32_t prev_level, uint32_t frames, uint64_t n, uint32_t target, uint32_t brighter, uint32_t darker, float exposure,
                                  float key) {
    if (frames == 0u) {
        if (n == 0) return rt3_exposure{ 0u, 0u, exposure, 0u };
        return rt3_exposure{ target, 1u, gain_of_level(target, exposure, key), 0u };
    }
    const uint32_t before = prev_level < kMaxLevel ? prev_level : kMaxLevel;
    const uint32_t level = n == 0 ? before : step_level(before, target, brighter, darker);
    return rt3_exposure{ level, frames == 0xFFFFFFFFu ? frames : frames + 1u, gain_of_level(level, exposure, key), 0u };
}
// The target of a histogram, serially: *n = the counted pixels; 0 when there are none.
RT3_HD uint32_t target_of(const uint32_t* hist, uint32_t trim_low, uint32_t trim_high, uint64_t* n_out) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < kBins; k++) n += hist[k];
    *n_out = n;
    if (n == 0) return 0u;
    const Trim t = trim_of(n, trim_low, trim_high);
    uint64_t s = 0, begin = 0;
    for (uint32_t k = 0; k < kBins; k++) {
        const uint64_t end = begin + hist[k];
        s += kept(t, begin, end) * k;
        begin = end;
    }
    return level_from_sum(t, s);
}

// ---- the bloom: planes of (r, g, b)
struct Rgb { float r, g, b; };
RT3_HD uint32_t half_of(uint32_t n) { return (n + 1u) >> 1; }       // W_l of W_{l-1}; 1 stays 1

// b0 of one input pixel under the gain: x = positive(gain * c, 65504), the part of it above the threshold.
RT3_HD Rgb exposed(float r, float g, float b, float gain) { return Rgb{ positive(gain * r, kHalfMax), positive(gain * g, kHalfMax), positive(gain * b, kHalfMax) }; }
RT3_HD Rgb bright(const Rgb& x, float threshold) {
    const float y = luminance(x.r, x.g, x.b);
    const float k = y > threshold ? (y - threshold) / y : 0.0f;
    return Rgb{ x.r * k, x.g * k, x.b * k };
}
// D_l(i, j) of its four sources s(2i, 2j), s(2i+1, 2j), s(2i, 2j+1), s(2i+1, 2j+1).
RT3_HD float down1(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }
RT3_HD Rgb down4(const Rgb& a, const Rgb& b, const Rgb& c, const Rgb& d) {
    return Rgb{ down1(a.r, b.r, c.r, d.r), down1(a.g, b.g, c.g, d.g), down1(a.b, b.b, c.b, d.b) };
}
// The source columns (or rows) of D_l's column i in a plane of ws columns: 2i and 2i + 1, clamped to the last.
RT3_HD uint32_t down_a(uint32_t i, uint32_t ws) { return 2u * i < ws - 1u ? 2u * i : ws - 1u; }
RT3_HD uint32_t down_b(uint32_t i, uint32_t ws) { return 2u * i + 1u < ws - 1u ? 2u * i + 1u : ws - 1u; }
// The two source columns (or rows) of up()'s column i in a coarse plane of wc columns: the near one (weight 0.75f) and the far one (0.25f).
RT3_HD uint32_t up_a(uint32_t i) { return i >> 1; }
RT3_HD uint32_t up_b(uint32_t i, uint32_t wc) {
    const uint32_t a = i >> 1;
    return (i & 1u) ? (a + 1u < wc - 1u ? a + 1u : wc - 1u) : (a > 0u ? a - 1u : 0u);
}
RT3_HD float up1(float aa, float ba, float ab, float bb) {
    const float ra = 0.75f * aa + 0.25f * ba, rb = 0.75f * ab + 0.25f * bb;
    return 0.75f * ra + 0.25f * rb;
}
// up(U)(i, j) of U(ia, ja), U(ib, ja), U(ia, jb), U(ib, jb).
RT3_HD Rgb up4(const Rgb& aa, const Rgb& ba, const Rgb& ab, const Rgb& bb) {
    return Rgb{ up1(aa.r, ba.r, ab.r, bb.r), up1(aa.g, ba.g, ab.g, bb.g), up1(aa.b, ba.b, ab.b, bb.b) };
}
RT3_HD Rgb sum(const Rgb& a, const Rgb& b) { return Rgb{ a.r + b.r, a.g + b.g, a.b + b.b }; }
RT3_HD float level_weight(uint32_t levels) { return 1.0f / (float)levels; }
RT3_HD Rgb scaled(const Rgb& a, float s) { return Rgb{ a.r * s, a.g * s, a.b * s }; }
// x' of x and B.
RT3_HD Rgb composite(const Rgb& x, const Rgb& bloom, float intensity) {
    return Rgb{ __builtin_fminf(x.r + intensity * bloom.r, kHalfMax), __builtin_fminf(x.g + intensity * bloom.g, kHalfMax),
                __builtin_fminf(x.b + intensity * bloom.b, kHalfMax) };
}

// A plane of float4 texels (the fourth float unused) wherever the caller keeps it, and the law's steps on whole texels of it.
struct Plane { const float* p; uint32_t w, h; };
RT3_HD Rgb texel(const Plane& s, uint32_t i, uint32_t j) {
    const float* t = s.p + 4u * ((size_t)j * s.w + i);
    return Rgb{ t[0], t[1], t[2] };
}
RT3_HD Rgb down_texel(const Plane& s, uint32_t i, uint32_t j) {
    const uint32_t ia = down_a(i, s.w), ib = down_b(i, s.w), ja = down_a(j, s.h), jb = down_b(j, s.h);
    return down4(texel(s, ia, ja), texel(s, ib, ja), texel(s, ia, jb), texel(s, ib, jb));
}
RT3_HD Rgb up_texel(const Plane& u, uint32_t i, uint32_t j) {
    const uint32_t ia = up_a(i), ib = up_b(i, u.w), ja = up_a(j), jb = up_b(j, u.h);
    return up4(texel(u, ia, ja), texel(u, ib, ja), texel(u, ia, jb), texel(u, ib, jb));
}
// B(i, j) of U_1.
RT3_HD Rgb bloom_texel(const Plane& u1, uint32_t i, uint32_t j, float weight) { return scaled(up_texel(u1, i, j), weight); }

// The pyramid's planes D_1 .. D_L, one behind the other: the texels before plane l (1-based) and in all of them.
inline size_t pyramid_texels(uint32_t w, uint32_t h, uint32_t levels) {
    size_t total = 0;
    for (uint32_t l = 0; l < levels; l++) { w = half_of(w); h = half_of(h); total += (size_t)w * h; }
    return total;
}

// The parameter check of every entry point: nullptr, or what is wrong.  The bloom's knobs are checked whether or not they are used.
inline const char* refusal(const rt3_display_sequence_params& p) {
    if (const char* why = rt3disp::refusal(p.display)) return why;
    if (p.adapt_brighter < 1u || p.adapt_brighter > kMaxRate || p.adapt_darker < 1u || p.adapt_darker > kMaxRate)
        return "adapt_brighter and adapt_darker must be 1 .. 1024";
    if (p.bloom_levels > kMaxBloomLevels) return "bloom_levels must be at most 8";
    if (!(p.bloom_threshold >= 0.0f) || !(p.bloom_threshold <= kFltMax)) return "bloom_threshold must be finite and >= 0";
    if (!(p.bloom_intensity >= 0.0f) || !(p.bloom_intensity <= kFltMax)) return "bloom_intensity must be finite and >= 0";
    if (p._pad[0] != 0u || p._pad[1] != 0u || p._pad[2] != 0u) return "rt3_display_sequence_params._pad must be 0";
    return nullptr;
}

}  // namespace rt3dseq
