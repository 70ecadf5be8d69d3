// rt3_sphere_plan.hpp — what a full sphere upload decides before it builds anything: the centre the filter's coordinates are taken about and the
// spheres that are tested directly.  Plain host C++ (no HIP): rt3_scene.hip includes it for rt3_set_spheres, rt3_host.cpp for
// rt3_debug_sphere_plan, which is what the device form of the upload (rt3_set_spheres_device, rt3_scene_build.hpp) is compared with.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// The centre of the spheres' filter coordinates: the component-wise median of the centres — the middle of where the spheres are,
// whatever a few far or huge ones do (the book scene's ground sphere, centre y = -1000, moves the mean by two units and the median not at
// all; weights of 1 / r^2, the minimiser of the sum of margin / r^2, follow the few smallest spheres instead: 9 % more exact tests on the
// 100 000-sphere scene).  Non-finite coordinates are skipped; (0, 0, 0) without any.
inline void sphere_filter_centre(const float* center_radius, uint32_t n, float out[3]) {
    std::vector<float> v;
    v.reserve(n);
    for (int a = 0; a < 3; a++) {
        v.clear();
        for (uint32_t i = 0; i < n; i++) { const float c = center_radius[4 * (size_t)i + a]; if (std::isfinite(c)) v.push_back(c); }
        out[a] = 0.0f;
        if (v.empty()) continue;
        std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
        out[a] = v[v.size() / 2];
    }
}

// Spheres that (nearly) every ray is a candidate for: the line of a ray that starts somewhere in the scene meets a sphere whose radius is
// comparable to its distance from there — the book scene's ground (r = 1000, its centre 1000 away).  The filter cannot reject such a sphere
// and it costs the pair list one entry per ray, so the matrix-filter kernels test it directly instead (TraceArgs::direct).  Any choice is
// correct; this one takes the (at most four) spheres with the largest r / max(|centre - c0|, R) above 1/2, R = the median distance of the
// centres from c0, i.e. the scene's own size: a unit sphere in the middle of the book scene (candidate for a few per cent of the rays) stays
// in the filter — a direct test costs every ray ~30 instructions.
inline uint32_t sphere_direct_list(const float* center_radius, uint32_t n, const float c0[3], uint32_t out[4]) {
    std::vector<double> dist(n);
    for (uint32_t i = 0; i < n; i++) {
        const float* s = center_radius + 4 * (size_t)i;
        const double dx = (double)s[0] - c0[0], dy = (double)s[1] - c0[1], dz = (double)s[2] - c0[2];
        dist[i] = std::sqrt(dx * dx + dy * dy + dz * dz);
    }
    double scene = 0.0;
    if (n) {
        std::vector<double> d(dist);
        for (double& v : d) if (!std::isfinite(v)) v = 0.0;
        std::nth_element(d.begin(), d.begin() + d.size() / 2, d.end());
        scene = d[d.size() / 2];
    }
    float best[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    uint32_t count = 0;
    for (uint32_t i = 0; i < n; i++) {
        const float ratio = (float)((double)center_radius[4 * (size_t)i + 3] / std::max(std::max(dist[i], scene), 1e-30));
        if (!(ratio >= 0.5f)) continue;                             // (NaN: not chosen)
        uint32_t k = count < 4 ? count++ : 4;
        if (k == 4) {                                               // replace the weakest if this one is stronger
            uint32_t w = 0;
            for (uint32_t q = 1; q < 4; q++) if (best[q] < best[w]) w = q;
            if (!(ratio > best[w])) continue;
            k = w;
        }
        best[k] = ratio; out[k] = i;
    }
    return count;
}
