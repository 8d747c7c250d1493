// rover_stones.h — the stone clearance test of rover.py:536-539 / :655-656 in its two forms: the minimum over all stones in LDS tiles
// (clearance_tiles) and the decision through the stone-occupancy grid of rover_set_stones (collides_grid).
// Users: metrics_done_env (rover_obs.hip) and clearance / shift_spawns / goals (rover_reset.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"

namespace rover {

// ---------------------------------------------------------------------------------------------------
// reset path.  Stones are staged through LDS in tiles of STONE_TILE (x, y, r) triples.
// ---------------------------------------------------------------------------------------------------
#define STONE_TILE 1024

__device__ __forceinline__ float clearance_tiles(const float* __restrict__ info7, uint32_t S, float x, float y, bool live,
                                                 float* sx, float* sy, float* sr) {
    float best = __builtin_inff();
    for (uint32_t s0 = 0; s0 < S; s0 += STONE_TILE) {
        uint32_t cnt = min((uint32_t)STONE_TILE, S - s0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
            const float* r = info7 + 7ull * (s0 + i);
            sx[i] = r[0]; sy[i] = r[1]; sr[i] = r[6];
        }
        __syncthreads();
        if (live) {
            for (uint32_t i = 0; i < cnt; ++i) {
                float dx = x - sx[i], dy = y - sy[i];
                float d = sqrtf(dx * dx + dy * dy) - sr[i];                 // rover.py:536-537 / :655-656
                best = (d < best || d != d) ? d : best;                    // torch.min (:538): a NaN stone makes the minimum NaN
            }
        }
    }
    return best;
}

// Decision form of the same test, min_s(|p - stone_s| - r_s) <= thr, through the stone-occupancy grid built at
// rover_set_stones: a grid cell lists every stone whose disc inflated by the largest threshold used (1.4 m, plus a
// margin far above f32 rounding) touches the cell, so stones outside the list cannot satisfy the inequality and the
// per-stone arithmetic on the listed ones is the reference's own (sqrt of the f32 sum of squares, minus r).
__device__ __forceinline__ bool collides_grid(const StoneGridDev& g, const float* __restrict__ info7, float x, float y, float thr) {
    float fx = (x - g.x0) * g.inv_cell, fy = (y - g.y0) * g.inv_cell;
    if (!(fx >= 0.0f) || !(fy >= 0.0f) || !(fx < (float)g.nx) || !(fy < (float)g.ny)) return false;   // also NaN
    uint32_t c = (uint32_t)fx * (uint32_t)g.ny + (uint32_t)fy;
    uint32_t k0 = g.cell_start[c], k1 = g.cell_start[c + 1];
    (void)info7;
    for (uint32_t k = k0; k < k1; k += 4u) {                                // 4 independent 16-B loads in flight per trip
        bool hit = false;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const float4 r = g.stone_xyr[min(k + j, k1 - 1u)];                 // past the end: the last entry again
            float dx = x - r.x, dy = y - r.y;
            float d = sqrtf(dx * dx + dy * dy) - r.z;                       // rover.py:536-537 / :655-656
            hit |= d <= thr;
        }
        if (hit) return true;
    }
    return false;
}

}  // namespace rover
