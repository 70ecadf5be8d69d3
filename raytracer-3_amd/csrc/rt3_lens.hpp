// rt3_lens.hpp — the lens models' ray generator (rt3_lens_rays*, rt3_render_lens*, rt3_render_lens_aov*).  The kernel does not
// trace: a render runs k_lens_rays, then the rays form of the scene's trace kernel once per sample on that buffer, then k_accumulate; the AOV pass runs
// the query form and k_aov_accumulate as the camera's does.  The law itself is rt3_lens_law.hpp's, shared with the host.
// Part of rt3_device.hip (one translation unit, gfx950 only); included from there, in this order.
#pragma once

namespace {

// What k_lens_rays reads: the lens, the frame, the shard and the batch.  A struct of its own: no trace kernel ever sees it.
struct LensArgs {
    rt3_lens lens;
    rt3lens::Frame frame;
    uint32_t tile_rows, tile_index, tile_count;
    uint32_t npix;           // pixels owned by this shard
    uint32_t s0;             // first sample of this batch
    uint32_t total;          // npix * samples in this batch
};

// Item k of the batch (sample s0 + k / npix, owned pixel k % npix) -> rays[2 k] = (origin, +inf), rays[2 k + 1] = (unit direction, 0): two 16-byte stores
// per ray, rt3_camera_rays' item order.  keys (a shard's; null for a whole frame, whose ray index IS the frame pixel index): the batch's first sample
// also writes keys[pix] = y * W + x, the key rt3_radiance's law wants for that ray.  rays holds 2 * total float4, keys npix words.
template <uint32_t MODEL>
__global__ __launch_bounds__(kBlock) void k_lens_rays(const LensArgs A, float4* __restrict__ rays, uint32_t* __restrict__ keys) {
    const uint32_t item = blockIdx.x * kBlock + threadIdx.x;
    if (item >= A.total) return;
    const uint32_t sb = item / A.npix, pix = item - sb * A.npix;
    const uint32_t lrow = pix / A.frame.width, x = pix - lrow * A.frame.width;
    uint32_t y = lrow;
    if (A.tile_count > 1) {
        const uint32_t lb = lrow / A.tile_rows, in = lrow - lb * A.tile_rows;
        y = (lb * A.tile_count + A.tile_index) * A.tile_rows + in;
    }
    float o[3], d[3];
    rt3lens::ray<MODEL>(A.lens, A.frame, x, y, A.s0 + sb, o, d);
    float4* r = rays + 2 * (size_t)item;
    r[0] = make_float4(o[0], o[1], o[2], __builtin_inff());
    r[1] = make_float4(d[0], d[1], d[2], 0.0f);
    if (keys != nullptr && sb == 0) keys[pix] = y * A.frame.width + x;
}

}  // namespace
