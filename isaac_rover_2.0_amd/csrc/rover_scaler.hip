// rover_scaler.hip — skrl's RunningStandardScaler on the device: the column moments of a batch folded into caller-owned float64
// statistics (two launches), and the normalisation / its inverse (one launch).  The definition is written out in include/rover_step.h
// (rover_scaler_update, rover_scaler_apply); the plan (route, rows per chunk, chunk count, scratch) is rover_scaler_plan's, a pure
// function of (M, N).
//
// Moments.  Every chunk of rows leaves, per column, (count, mean, M2) in f64 from PLAIN SUMS: S1 = sum x and S2 = sum x*x, every x widened
// to f64 first (the product of two f32 values is exact in f64), mean = S1 / n, M2 = max(S2 - (S1 * S1) / n, 0).
//   wide:   a thread owns two neighbouring columns (one 8-byte load per row where base and stride allow, two scalar loads otherwise: the
//           same additions in the same order) and walks the chunk's rows in order — at most 128 additions per sum, no merge.
//   narrow: the 256 threads of a workgroup split the chunk's rows (thread t takes rows t, t + 256, ...: at most 64 per sum), column by
//           column, and add their sums in a fixed binary tree in LDS (8 levels).
// The finishing launch merges the chunks IN CHUNK ORDER by Chan's update, in two levels — 8 runs of consecutive chunks per column, one
// thread each, then the 8 runs in order —, and folds the batch into the state.  (One thread per column over all chunks was 19 us at 128
// chunks and 70 us at 512: a chain of dependent f64 divisions.)
// No atomics anywhere: the same inputs give the same bits whatever the launch, the alignment or the row stride.
//
// Apply.  Bandwidth bound: wide, a thread owns a column pair for SCALER_APPLY_ROWS rows (its four statistics are read and rounded to f32
// once); narrow, the matrix is walked as a flat list of elements and the (at most 8) columns' statistics sit in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"

namespace rover {

#define SCALER_BLOCK 256u
#define SCALER_FOLD_COLS 32u         // the finishing kernel: columns per workgroup ...
#define SCALER_FOLD_RUNS 8u          // ... times runs of consecutive chunks = SCALER_BLOCK threads
#define SCALER_APPLY_ROWS 16u        // rows per workgroup of the wide apply kernel
#define SCALER_APPLY_ITEMS 4u        // elements per thread of the narrow apply kernel

__device__ __forceinline__ void scaler_store_partial(const ScalerUpdateArgs& a, uint32_t chunk, uint32_t col, double n, double s1, double s2) {
    const uint64_t plane = (uint64_t)a.n_chunks * a.N, at = (uint64_t)chunk * a.N + col;
    const double m2 = s2 - (s1 * s1) / n;
    a.partials[at] = n;
    a.partials[plane + at] = s1 / n;
    a.partials[2u * plane + at] = m2 < 0.0 ? 0.0 : m2;               // a NaN stays a NaN
}

// The finishing launch reads the count the call started from out of the scratch header: it writes *count itself.
__device__ __forceinline__ void scaler_keep_count(const ScalerUpdateArgs& a) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.partials[-1] = *a.count;
}

template <bool VEC>
__global__ void __launch_bounds__(SCALER_BLOCK) scaler_moments_wide_kernel(ScalerUpdateArgs a) {
    scaler_keep_count(a);
    const uint32_t c0 = 2u * (blockIdx.y * SCALER_BLOCK + threadIdx.x);
    if (c0 >= a.N) return;
    const bool both = c0 + 1u < a.N;                                  // false for the last pair of an odd N
    const uint32_t row0 = blockIdx.x * a.rows_per_chunk, row1 = min(row0 + a.rows_per_chunk, a.M);
    const float* p = a.x + (uint64_t)row0 * (uint64_t)a.x_stride + c0;
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0;
#pragma unroll 4
    for (uint32_t r = row0; r < row1; ++r, p += a.x_stride) {
        float x0, x1 = 0.0f;
        if (VEC && both) { const float2 v = *reinterpret_cast<const float2*>(p); x0 = v.x; x1 = v.y; }
        else { x0 = p[0]; if (both) x1 = p[1]; }
        const double d0 = (double)x0, d1 = (double)x1;
        s1a += d0; s2a += d0 * d0;
        s1b += d1; s2b += d1 * d1;
    }
    const double n = (double)(row1 - row0);
    scaler_store_partial(a, blockIdx.x, c0, n, s1a, s2a);
    if (both) scaler_store_partial(a, blockIdx.x, c0 + 1u, n, s1b, s2b);
}

__global__ void __launch_bounds__(SCALER_BLOCK) scaler_moments_narrow_kernel(ScalerUpdateArgs a) {
    __shared__ double s_1[SCALER_BLOCK], s_2[SCALER_BLOCK];
    scaler_keep_count(a);
    const uint32_t tid = threadIdx.x;
    const uint32_t row0 = blockIdx.x * a.rows_per_chunk, row1 = min(row0 + a.rows_per_chunk, a.M);
    for (uint32_t c = 0; c < a.N; ++c) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
        for (uint32_t r = row0 + tid; r < row1; r += SCALER_BLOCK) {
            const double d = (double)a.x[(uint64_t)r * (uint64_t)a.x_stride + c];
            s1 += d; s2 += d * d;
        }
        s_1[tid] = s1; s_2[tid] = s2;
        __syncthreads();
        for (uint32_t w = SCALER_BLOCK / 2u; w > 0u; w >>= 1) {
            if (tid < w) { s_1[tid] += s_1[tid + w]; s_2[tid] += s_2[tid + w]; }
            __syncthreads();
        }
        if (tid == 0) scaler_store_partial(a, blockIdx.x, c, (double)(row1 - row0), s_1[0], s_2[0]);
        __syncthreads();                                              // s_1 / s_2 are rewritten for the next column
    }
}

// One Chan update: (n, mean, M2) absorbs a chunk (or a run of chunks) that follows it in row order
__device__ __forceinline__ void scaler_merge(double& n, double& mean, double& M2, double nk, double mean_k, double m2_k) {
    const double d = mean_k - mean, tot = n + nk, f = nk / tot;
    mean = mean + d * f;
    M2 = (M2 + m2_k) + (d * d) * (n * f);
    n = tot;
}

// A workgroup owns SCALER_FOLD_COLS columns; thread (run, column) merges the chunks of run `run` — ceil(n_chunks / SCALER_FOLD_RUNS)
// consecutive chunks — in chunk order, then the run-0 thread of each column merges the runs in order and folds the batch into the state.
__global__ void __launch_bounds__(SCALER_BLOCK) scaler_fold_kernel(ScalerUpdateArgs a) {
    __shared__ double s_n[SCALER_FOLD_RUNS][SCALER_FOLD_COLS], s_mu[SCALER_FOLD_RUNS][SCALER_FOLD_COLS], s_m2[SCALER_FOLD_RUNS][SCALER_FOLD_COLS];
    if (a.skip_if && *a.skip_if != 0) return;                         // the same for every thread; the state stays bit-unchanged
    const uint32_t lane = threadIdx.x % SCALER_FOLD_COLS, run = threadIdx.x / SCALER_FOLD_COLS;
    const uint32_t c = blockIdx.x * SCALER_FOLD_COLS + lane;
    const uint32_t per = (a.n_chunks + SCALER_FOLD_RUNS - 1u) / SCALER_FOLD_RUNS;
    const uint32_t k0 = run * per, k1 = min(k0 + per, a.n_chunks);
    const uint64_t plane = (uint64_t)a.n_chunks * a.N;
    const double *cnt = a.partials, *mu = a.partials + plane, *m2 = a.partials + 2u * plane;
    double n = 0.0, mb = 0.0, M2 = 0.0;                                // an empty run (k0 >= k1) keeps n = 0 and is passed over below
    if (c < a.N && k0 < k1) {
        const uint64_t first = (uint64_t)k0 * a.N + c;
        n = cnt[first]; mb = mu[first]; M2 = m2[first];
#pragma unroll 4
        for (uint32_t k = k0 + 1u; k < k1; ++k) {
            const uint64_t at = (uint64_t)k * a.N + c;
            scaler_merge(n, mb, M2, cnt[at], mu[at], m2[at]);
        }
    }
    s_n[run][lane] = n; s_mu[run][lane] = mb; s_m2[run][lane] = M2;
    __syncthreads();
    if (run != 0u || c >= a.N) return;                                // run 0 holds chunk 0: never empty
    for (uint32_t r = 1; r < SCALER_FOLD_RUNS; ++r)
        if (s_n[r][lane] != 0.0) scaler_merge(n, mb, M2, s_n[r][lane], s_mu[r][lane], s_m2[r][lane]);
    const double Md = (double)a.M, count = a.partials[-1], mean = a.mean[c], var = a.var[c];
    const double vb = M2 / (Md - 1.0);
    const double delta = mb - mean, total = count + Md;
    const double m2s = (var * count + vb * Md) + (((delta * delta) * count) * Md) / total;
    a.mean[c] = mean + (delta * Md) / total;
    a.var[c] = m2s / total;
    if (c == 0) *a.count = total;
}

hipError_t launch_scaler_update(const ScalerUpdateArgs& a, int route, hipStream_t s) {
    if (route == SCALER_ROUTE_NARROW) {
        hipLaunchKernelGGL(scaler_moments_narrow_kernel, dim3(a.n_chunks), dim3(SCALER_BLOCK), 0, s, a);
    } else {
        const dim3 grid(a.n_chunks, blocks_for((a.N + 1u) / 2u, SCALER_BLOCK));
        const bool vec = a.x_stride % 2 == 0 && (uintptr_t)a.x % 8 == 0;      // every column pair of every row starts on an 8-byte boundary
        if (vec) hipLaunchKernelGGL(scaler_moments_wide_kernel<true>, grid, dim3(SCALER_BLOCK), 0, s, a);
        else hipLaunchKernelGGL(scaler_moments_wide_kernel<false>, grid, dim3(SCALER_BLOCK), 0, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scaler_fold_kernel, dim3(blocks_for(a.N, SCALER_FOLD_COLS)), dim3(SCALER_BLOCK), 0, s, a);
    return hipGetLastError();
}

// torch.clamp: a NaN stays a NaN (fminf / fmaxf alone would return the bound)
__device__ __forceinline__ float scaler_clamp(float v, float clip) { return v != v ? v : fminf(fmaxf(v, -clip), clip); }

// one rounding per written operation (the library is built with -ffp-contract=off); `scale` is sqrt(f32(var)) + f32(eps) forward,
// sqrt(f32(var)) inverse
template <bool INVERSE>
__device__ __forceinline__ float scaler_value(float x, float mean, float scale, float clip) {
    if (INVERSE) return scale * scaler_clamp(x, clip) + mean;
    return scaler_clamp((x - mean) / scale, clip);
}

template <bool INVERSE>
__device__ __forceinline__ void scaler_stats(const ScalerApplyArgs& a, uint32_t c, float& mean, float& scale) {
    mean = (float)a.mean[c];
    const float sd = sqrtf((float)a.var[c]);
    scale = INVERSE ? sd : sd + a.epsilon;
}

template <bool INVERSE, bool VEC>
__global__ void __launch_bounds__(SCALER_BLOCK) scaler_apply_wide_kernel(ScalerApplyArgs a) {
    const uint32_t c0 = 2u * (blockIdx.y * SCALER_BLOCK + threadIdx.x);
    if (c0 >= a.N) return;
    const bool both = c0 + 1u < a.N;
    float m0, k0, m1 = 0.0f, k1 = 1.0f;
    scaler_stats<INVERSE>(a, c0, m0, k0);
    if (both) scaler_stats<INVERSE>(a, c0 + 1u, m1, k1);
    const uint32_t row0 = blockIdx.x * SCALER_APPLY_ROWS, row1 = min(row0 + SCALER_APPLY_ROWS, a.M);
#pragma unroll 4
    for (uint32_t r = row0; r < row1; ++r) {
        const float* src = a.x + (uint64_t)r * (uint64_t)a.x_stride + c0;
        float* dst = a.y + (uint64_t)r * (uint64_t)a.y_stride + c0;
        float x0, x1 = 0.0f;
        if (VEC && both) { const float2 v = *reinterpret_cast<const float2*>(src); x0 = v.x; x1 = v.y; }
        else { x0 = src[0]; if (both) x1 = src[1]; }
        const float y0 = scaler_value<INVERSE>(x0, m0, k0, a.clip), y1 = scaler_value<INVERSE>(x1, m1, k1, a.clip);
        if (VEC && both) *reinterpret_cast<float2*>(dst) = make_float2(y0, y1);
        else { dst[0] = y0; if (both) dst[1] = y1; }
    }
}

template <bool INVERSE>
__global__ void __launch_bounds__(SCALER_BLOCK) scaler_apply_narrow_kernel(ScalerApplyArgs a) {
    __shared__ float s_mean[SCALER_NARROW_MAX_N], s_scale[SCALER_NARROW_MAX_N];
    if (threadIdx.x < a.N) scaler_stats<INVERSE>(a, threadIdx.x, s_mean[threadIdx.x], s_scale[threadIdx.x]);
    __syncthreads();
    const uint32_t total = a.M * a.N, base = blockIdx.x * (SCALER_BLOCK * SCALER_APPLY_ITEMS) + threadIdx.x;      // M N < 2^31
#pragma unroll
    for (uint32_t i = 0; i < SCALER_APPLY_ITEMS; ++i) {
        const uint32_t e = base + i * SCALER_BLOCK;
        if (e >= total) break;
        const uint32_t r = e / a.N, c = e - r * a.N;
        const float x = a.x[(uint64_t)r * (uint64_t)a.x_stride + c];
        a.y[(uint64_t)r * (uint64_t)a.y_stride + c] = scaler_value<INVERSE>(x, s_mean[c], s_scale[c], a.clip);
    }
}

template <bool INVERSE>
static void scaler_apply_launch(const ScalerApplyArgs& a, hipStream_t s) {
    if (a.N <= SCALER_NARROW_MAX_N) {
        const uint32_t grid = blocks_for((uint64_t)a.M * a.N, SCALER_BLOCK * SCALER_APPLY_ITEMS);
        hipLaunchKernelGGL(scaler_apply_narrow_kernel<INVERSE>, dim3(grid), dim3(SCALER_BLOCK), 0, s, a);
        return;
    }
    const dim3 grid(blocks_for(a.M, SCALER_APPLY_ROWS), blocks_for((a.N + 1u) / 2u, SCALER_BLOCK));
    const bool vec = a.x_stride % 2 == 0 && a.y_stride % 2 == 0 && (uintptr_t)a.x % 8 == 0 && (uintptr_t)a.y % 8 == 0;
    if (vec) hipLaunchKernelGGL((scaler_apply_wide_kernel<INVERSE, true>), grid, dim3(SCALER_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((scaler_apply_wide_kernel<INVERSE, false>), grid, dim3(SCALER_BLOCK), 0, s, a);
}

hipError_t launch_scaler_apply(const ScalerApplyArgs& a, bool inverse, hipStream_t s) {
    if (inverse) scaler_apply_launch<true>(a, s);
    else scaler_apply_launch<false>(a, s);
    return hipGetLastError();
}

}  // namespace rover
