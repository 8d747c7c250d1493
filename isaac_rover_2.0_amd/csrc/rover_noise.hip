// rover_noise.hip — the sensor model of the student's perception: noise on the heightmap columns of an observation matrix.
//
// The reference's authors tried Gaussian noise, dropout, a constant offset and zeroed columns on the observation (tasks/rover.py:326-329,
// commented out) and carry is_evaluation_with_noise / max_noise_dev; the definition this file implements is the project's own and is
// written out in include/rover_step.h (rover_obs_noise).  It is counter-based like the head's action noise: a value depends on (seed,
// call counter, global row, column) and the row's episode count, never on the batch shape, a stride or the launch.
//
// One launch, elementwise.  A workgroup of 256 threads owns OBS_NOISE_ROWS rows x 256 column pairs.  One thread owns one column pair of
// each of those rows: ONE Philox call gives the pair's two normals (words 0, 1 through the head's Box-Muller, rover_gauss.h) and its two
// dropout words (2, 3), and the pair moves as one 8-byte load and one 8-byte store where the addresses allow (VEC), as two scalars with
// the same arithmetic otherwise.  The offset draw (a second Philox call and a second logarithm, the same for every column of a row)
// is hoisted: the first OBS_NOISE_ROWS threads of the workgroup draw it once per row and leave (sigma_offset s) eo and sigma_point s
// in LDS — 1 draw per 256 pair draws.  A term whose sigma is 0 is not drawn at all (POINT, and the offset's test), dropout with thr = 0
// is not tested (DROP); with neither POINT nor DROP no Philox call is made.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"
#include "rover_philox.h"
#include "rover_gauss.h"

namespace rover {

#define OBS_NOISE_ROWS 8u           // rows per workgroup: the offset draw costs 1 / (8 x 256 / 64) = 1 / 32 of the pair draws' instructions
#define OBS_NOISE_MAX_GROUPS 32768u // most workgroups along the rows; more row groups than that are walked with a grid stride

// v of one element: one rounding per written operation (the library is built with -ffp-contract=off)
__device__ __forceinline__ float obs_noise_value(float x, float off, float a_point, float eps) { return (x + off) + a_point * eps; }

template <bool POINT, bool DROP, bool VEC>
__global__ void __launch_bounds__(256) obs_noise_kernel(ObsNoiseArgs a, uint32_t n_groups) {
    __shared__ float s_off[OBS_NOISE_ROWS], s_point[OBS_NOISE_ROWS];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = a.step + (a.step_dev ? *a.step_dev : 0ull);
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const uint32_t M = (uint32_t)a.M, first = (uint32_t)a.first, C = (uint32_t)(a.F - a.first);
    const uint32_t p = blockIdx.y * 256u + tid, c0 = 2u * p;         // this thread's column pair: heightmap columns c0, c0 + 1
    const bool in_place = a.in == a.out;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint32_t row0 = grp * OBS_NOISE_ROWS;
        if (tid < OBS_NOISE_ROWS && row0 + tid < M) {
            const uint32_t r = row0 + tid;
            const float s = a.row_scale ? a.row_scale[r] : 1.0f;
            float off = 0.0f;                                          // sigma_offset == 0: the term is +0.0f, no draw
            if (a.sigma_offset != 0.0f) {
                const uint64_t e = a.episode ? (uint64_t)a.episode[r] : 0ull;
                uint32_t w[4] = {(uint32_t)((uint64_t)a.row_offset + r), (uint32_t)e, (uint32_t)(e >> 32), 0x70000000u};
                philox4x32_10(w, k0, k1);
                float eo, unused;
                gauss_pair_of_words(w[0], w[1], eo, unused);
                off = (a.sigma_offset * s) * eo;
            }
            s_off[tid] = off;
            s_point[tid] = a.sigma_point * s;
        }
        __syncthreads();
        if (c0 < C) {
            const bool both = c0 + 1u < C;                             // false for the last pair of an odd C: its second element does not exist
#pragma unroll 4
            for (uint32_t q = 0; q < OBS_NOISE_ROWS; ++q) {
                const uint32_t r = row0 + q;
                if (r >= M) break;
                const float* src = a.in + (uint64_t)r * (uint64_t)a.in_stride + first + c0;
                float* dst = a.out + (uint64_t)r * (uint64_t)a.out_stride + first + c0;
                float x0, x1 = 0.0f;
                if (VEC && both) { const float2 x = *reinterpret_cast<const float2*>(src); x0 = x.x; x1 = x.y; }
                else { x0 = src[0]; if (both) x1 = src[1]; }
                uint32_t w[4] = {(uint32_t)((uint64_t)a.row_offset + r), (uint32_t)t, (uint32_t)(t >> 32), 0x60000000u | p};
                if (POINT || DROP) philox4x32_10(w, k0, k1);
                float e0 = 0.0f, e1 = 0.0f;
                if (POINT) gauss_pair_of_words(w[0], w[1], e0, e1);
                const float off = s_off[q], ap = s_point[q];
                float v0 = POINT ? obs_noise_value(x0, off, ap, e0) : (x0 + off) + 0.0f;      // sigma_point == 0: the term is +0.0f
                float v1 = POINT ? obs_noise_value(x1, off, ap, e1) : (x1 + off) + 0.0f;
                if (DROP) {
                    if ((w[2] >> 8) < a.thr) v0 = a.drop_value;
                    if ((w[3] >> 8) < a.thr) v1 = a.drop_value;
                }
                if (VEC && both) *reinterpret_cast<float2*>(dst) = make_float2(v0, v1);
                else { dst[0] = v0; if (both) dst[1] = v1; }
            }
        }
        if (!in_place)                                                 // the proprioceptive columns, shared among the workgroups of the row group
            for (uint32_t col = p; col < first; col += gridDim.y * 256u)
                for (uint32_t q = 0; q < OBS_NOISE_ROWS && row0 + q < M; ++q)
                    a.out[(uint64_t)(row0 + q) * (uint64_t)a.out_stride + col] = a.in[(uint64_t)(row0 + q) * (uint64_t)a.in_stride + col];
        __syncthreads();                                               // s_off / s_point are rewritten for the next row group
    }
}

template <bool POINT, bool DROP>
static void obs_noise_launch(const ObsNoiseArgs& a, bool vec, dim3 grid, uint32_t n_groups, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((obs_noise_kernel<POINT, DROP, true>), grid, dim3(256), 0, s, a, n_groups);
    else hipLaunchKernelGGL((obs_noise_kernel<POINT, DROP, false>), grid, dim3(256), 0, s, a, n_groups);
}

hipError_t launch_obs_noise(const ObsNoiseArgs& a, hipStream_t s) {
    const uint32_t n_groups = blocks_for((uint64_t)a.M, OBS_NOISE_ROWS);
    const uint32_t pairs = (uint32_t)(a.F - a.first + 1) / 2u;
    // columns without a pair still need workgroups for the copy of [0, first): one per 256 columns, as many as the pairs would take at most
    const uint32_t gy = pairs ? blocks_for(pairs, 256u) : 1u;
    const dim3 grid(n_groups < OBS_NOISE_MAX_GROUPS ? n_groups : OBS_NOISE_MAX_GROUPS, gy);
    // 8-byte moves: every pair of every row starts on an 8-byte boundary
    const bool vec = a.first % 2 == 0 && a.in_stride % 2 == 0 && a.out_stride % 2 == 0 && (uintptr_t)a.in % 8 == 0 && (uintptr_t)a.out % 8 == 0;
    const bool point = a.sigma_point != 0.0f, drop = a.thr != 0u;
    if (point && drop) obs_noise_launch<true, true>(a, vec, grid, n_groups, s);
    else if (point) obs_noise_launch<true, false>(a, vec, grid, n_groups, s);
    else if (drop) obs_noise_launch<false, true>(a, vec, grid, n_groups, s);
    else obs_noise_launch<false, false>(a, vec, grid, n_groups, s);
    return hipGetLastError();
}

}  // namespace rover
