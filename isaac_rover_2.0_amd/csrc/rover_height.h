// rover_height.h — the heightfield lookup of get_pos_height (rover.py:588-608) as one device function, shared by the kernels that read
// terrain heights: goals and sample_height (rover_reset.hip), the ray preparation (rover_rays.hip), the motion model (rover_motion.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"

namespace rover {

// camera.py:241-253: clamp bound is the dim-0 size for both axes; torch.round is half-to-even.
// `/ horizontal_scale` (a Python float): ATen's CPU kernel divides (rcp = 0, what the golden vectors pin); ATen's CUDA
// kernel multiplies by 1 / scale rounded to f32 (rcp = 1, option cell_index_mode) — they differ next to .5 ties only.
__device__ __forceinline__ uint32_t cell_coord(float v, float shift, float cell, float inv_cell, int32_t rcp, int32_t dim0) {
    float s = rcp ? (v - shift) * inv_cell : (v - shift) / cell;
    float hi = (float)(dim0 - 1);
    s = (s < 0.0f) ? 0.0f : s;
    s = (s > hi) ? hi : s;
    s = rintf(s);
    if (!(s == s)) return 0u;          // NaN pose: the reference raises; map to cell 0 (all tests then miss)
    return (uint32_t)s;
}

__device__ __forceinline__ float height_at(const HeightDev& h, float x, float y) {
    uint32_t ix = cell_coord(x, h.shift_x, h.hscale, h.inv_hscale, h.rcp, h.N0);
    uint32_t iy = cell_coord(y, h.shift_y, h.hscale, h.inv_hscale, h.rcp, h.N0);
    if (iy > (uint32_t)(h.N1 - 1)) iy = (uint32_t)(h.N1 - 1);
    return h.hm[(uint64_t)ix * h.N1 + iy] * h.vscale;
}

}  // namespace rover
