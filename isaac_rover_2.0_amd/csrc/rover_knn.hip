// rover_knn.hip — the KNN map builder (rover_build_knn_map): centroids, bucketing, ring search (gfx950, wave64).
//
// Reference (pure PyTorch; paths relative to omniisaacgymenvs/):
//   tasks/utils/rover_utils.py:52-118
// Built with -ffp-contract=off: see rover_rays.hip.
// Kernels; the scan between the two bucket passes is rover_sort.hip's launch_scan_exclusive:
//   knn_centroid / knn_bucket / knn_select kernels                                                                   (f-3)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"

namespace rover {

// ---------------------------------------------------------------------------------------------------
// KNN map builder ("next" row f-3): for every map cell the K triangles whose centroid is nearest in xy
// (tasks/utils/rover_utils.py:52-118, which ranks ALL centroids per cell with a python double loop of topk).
// Here: centroids are bucketed on a uniform grid; one workgroup per map cell gathers buckets ring by ring into
// LDS as 64-bit keys (f32 squared distance bits << 32 | triangle id), bitonic-sorts them and stops as soon as the
// K-th distance is inside the searched radius.  Ranking: exact f32 squared distance, ties by triangle id (the
// reference ranks fp16-rounded distances with an unspecified tie order, so it cannot be matched bit for bit).
// ---------------------------------------------------------------------------------------------------
#define KNN_CAP 8192
#define KNN_STOP_SLACK 0x1p-20f          // knn_select_kernel's stop test; tests/knn_ref.py (STOP_SLACK) restates the value

// ref = 1: the reference's own arithmetic — numpy float64 centroid of the (float64) open3d vertices (rover_utils.py:68-70),
// then torch.tensor(..., dtype=float16) (:72), which converts double -> float -> half; kept here as the half's float value.
__global__ void __launch_bounds__(256) knn_centroid_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           uint32_t T, uint32_t V, int ref, float* __restrict__ cx, float* __restrict__ cy) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    uint32_t a = (uint32_t)tris[3ull * t], b = (uint32_t)tris[3ull * t + 1], c = (uint32_t)tris[3ull * t + 2];
    a = a < V ? a : 0u; b = b < V ? b : 0u; c = c < V ? c : 0u;
    if (ref) {
        double x = (((double)verts[3ull * a] + (double)verts[3ull * b]) + (double)verts[3ull * c]) / 3.0;
        double y = (((double)verts[3ull * a + 1] + (double)verts[3ull * b + 1]) + (double)verts[3ull * c + 1]) / 3.0;
        cx[t] = (float)(_Float16)(float)x;
        cy[t] = (float)(_Float16)(float)y;
        return;
    }
    cx[t] = (verts[3ull * a] + verts[3ull * b] + verts[3ull * c]) / 3.0f;             // rover_utils.py:68-70
    cy[t] = (verts[3ull * a + 1] + verts[3ull * b + 1] + verts[3ull * c + 1]) / 3.0f;
}

__device__ __forceinline__ uint32_t knn_bucket(float v, float origin, float inv_g, uint32_t n) {
    float f = (v - origin) * inv_g;
    if (!(f > 0.0f)) return 0u;
    uint32_t b = (uint32_t)f;
    return b < n ? b : n - 1u;
}

// pass 1 (count = 1): histogram of bucket ids; pass 2 (count = 0): fill ids at cursor positions
__global__ void __launch_bounds__(256) knn_bucket_kernel(const float* __restrict__ cx, const float* __restrict__ cy, uint32_t T,
                                                         float ox, float oy, float inv_g, uint32_t nbx, uint32_t nby,
                                                         uint32_t* __restrict__ cursor, uint32_t* __restrict__ items, int count) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    uint32_t b = knn_bucket(cx[t], ox, inv_g, nbx) * nby + knn_bucket(cy[t], oy, inv_g, nby);
    uint32_t pos = atomicAdd(cursor + b, 1u);
    if (!count) items[pos] = t;
}

__global__ void __launch_bounds__(256) knn_select_kernel(const float* __restrict__ cx, const float* __restrict__ cy,
                                                         const uint32_t* __restrict__ bucket_start, const uint32_t* __restrict__ items,
                                                         float ox, float oy, float g, float span, uint32_t nbx, uint32_t nby, uint32_t X,
                                                         uint32_t Y, float res, uint32_t K, const float* __restrict__ cell_x,
                                                         const float* __restrict__ cell_y, int32_t* __restrict__ out,
                                                         int32_t* __restrict__ overflow) {
    __shared__ unsigned long long keys[KNN_CAP];
    __shared__ uint32_t count;
    const uint32_t cell = blockIdx.x, x = cell / Y, y = cell % Y, tid = threadIdx.x;
    // rover_utils.py:75-81: cell (x, y) sits at (x res, y res).  Reference ranking (cell_x != NULL): the fp16 coordinate tables
    // of its torch.arange(..., dtype=float16), and distances as its fp16 tensors give them (:99-102): fp16(c - p) per axis,
    // norm = sqrt of the f32 sum of squares, rounded to fp16; the key is that fp16 value, ties by triangle id.
    const bool ref = cell_x != nullptr;
    const float px = ref ? cell_x[x] : (float)x * res, py = ref ? cell_y[y] : (float)y * res;
    const float inv_g = 1.0f / g;
    const int bx = (int)knn_bucket(px, ox, inv_g, nbx), by = (int)knn_bucket(py, oy, inv_g, nby);
    const int rmax = (int)max(nbx, nby);
    if (tid == 0) count = 0;
    __syncthreads();
    for (int r = 0; r <= rmax; ++r) {
        // append the buckets at Chebyshev distance r (the square ring), one bucket per thread at a time
        const int side = 2 * r + 1, nring = r == 0 ? 1 : 8 * r;
        for (int q = (int)tid; q < nring; q += 256) {
            int i, j;
            if (r == 0) { i = bx; j = by; }
            else if (q < side) { i = bx - r; j = by - r + q; }                         // left column
            else if (q < 2 * side) { i = bx + r; j = by - r + (q - side); }            // right column
            else if (q < 2 * side + (side - 2)) { i = bx - r + 1 + (q - 2 * side); j = by - r; }     // bottom row
            else { i = bx - r + 1 + (q - 2 * side - (side - 2)); j = by + r; }                     // top row
            if (i < 0 || j < 0 || i >= (int)nbx || j >= (int)nby) continue;
            const uint32_t b = (uint32_t)i * nby + (uint32_t)j, s0 = bucket_start[b], s1 = bucket_start[b + 1];
            if (s1 == s0) continue;
            uint32_t base = atomicAdd(&count, s1 - s0);
            for (uint32_t k = s0; k < s1; ++k, ++base) {
                if (base >= KNN_CAP) break;
                const uint32_t t = items[k];
                float dx = cx[t] - px, dy = cy[t] - py;
                if (ref) { dx = (float)(_Float16)dx; dy = (float)(_Float16)dy; }
                const float d2 = dx * dx + dy * dy;
                const float key = ref ? (float)(_Float16)sqrtf(d2) : d2;        // non-negative floats order like their bits
                keys[base] = ((unsigned long long)__float_as_uint(key) << 32) | t;
            }
        }
        __syncthreads();
        const uint32_t n = count;
        __syncthreads();                 // every wave has read n before any wave appends the next ring to `count`
        if (n > KNN_CAP) { if (tid == 0) *overflow = 1; return; }
        const bool covers_all = (bx - r <= 0) && (by - r <= 0) && (bx + r >= (int)nbx - 1) && (by + r >= (int)nby - 1);
        if (n >= K || covers_all) {
            uint32_t m = 1; while (m < n) m <<= 1;                       // bitonic sort of keys[0..m), padded with +inf keys
            for (uint32_t k = n + tid; k < m; k += 256) keys[k] = ~0ull;
            __syncthreads();
            for (uint32_t len = 2; len <= m; len <<= 1) {
                for (uint32_t stride = len >> 1; stride > 0; stride >>= 1) {
                    for (uint32_t k = tid; k < (m >> 1); k += 256) {
                        const uint32_t lo = ((k / stride) * stride << 1) + (k % stride), hi = lo + stride;
                        const bool up = ((lo & len) == 0);
                        const unsigned long long a = keys[lo], b = keys[hi];
                        if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
                    }
                    __syncthreads();
                }
            }
            // Every triangle not gathered yet lies more than r buckets out along one axis.  In real numbers that puts it more than r*g
            // away; in knn_bucket's float32 it does not quite ("KNN stop test").  With u = 2^-24, c the centroid's and p
            // the cell's coordinate on that axis, o the origin and F(v) = fl(fl(v - o) * inv_g), which is monotone in v:
            //   floor(F(c)) >= floor(F(p)) + r + 1 (the clamps of knn_bucket keep that)   =>   F(c) - F(p) > r
            //   F(v) = (v - o) / g * (1 + e), |e| <= 3u + 3u^2: the subtraction, the product, and inv_g = fl(1 / g) (the same for both)
            //   =>  c - p > r g (1 - u) - 4 (1 + u) u span,      span >= |c - o|, |p - o|  (the host passes it: the largest one there is)
            //   d2 = fl(fl(dx dx) + fl(dy dy)) >= fl(dx dx) with dx = fl(c - p)   =>   d2 >= (c - p)^2 (1 - u)^3
            // so d2 > (r g (1 - 2.5 u) - 4.1 u span)^2, while lim below is at most r g (1 - 13 u) - 15.9 u span and fl(lim lim) <=
            // lim^2 (1 + u): a K-th key <= lim^2 is strictly below every ungathered key, ties included.  The slack has a part relative
            // to the reach and a part absolute in span: a relative factor alone does not cover a mesh far from its cells.
            // (reference ranking: an ungathered triangle is >= reach away in the fp16-rounded coordinates, up to the same few u span, and
            //  its fp16 distance is at most a factor 1 - 2^-9.9 below that, so a K-th key strictly below reach (1 - 2^-9) cannot be
            //  undercut or tied: tests/test_knn_ring_property.py holds both claims against the arithmetic)
            const float reach = (float)r * g;
            const float lim = reach - (reach + span) * KNN_STOP_SLACK;
            const float kth = n >= K ? __uint_as_float((uint32_t)(keys[K - 1] >> 32)) : __builtin_inff();
            if (covers_all || (ref ? kth < reach * (1.0f - 1.0f / 512.0f) : (lim > 0.0f && kth <= lim * lim))) {
                for (uint32_t k = tid; k < K; k += 256) out[(uint64_t)cell * K + k] = k < n ? (int32_t)(uint32_t)keys[k] : 0;
                return;
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t launch_knn_centroids(const float* verts, const int32_t* tris, uint32_t T, uint32_t V, int ref, float* cx, float* cy,
                                hipStream_t s) {
    hipLaunchKernelGGL(knn_centroid_kernel, dim3(blocks_for(T, 256)), dim3(256), 0, s, verts, tris, T, V, ref, cx, cy);
    return hipGetLastError();
}

hipError_t launch_knn_bucket(const float* cx, const float* cy, uint32_t T, float ox, float oy, float inv_g, uint32_t nbx, uint32_t nby,
                             uint32_t* cursor, uint32_t* items, int count, hipStream_t s) {
    hipLaunchKernelGGL(knn_bucket_kernel, dim3(blocks_for(T, 256)), dim3(256), 0, s, cx, cy, T, ox, oy, inv_g, nbx, nby, cursor, items,
                       count);
    return hipGetLastError();
}

hipError_t launch_knn_select(const float* cx, const float* cy, const uint32_t* bucket_start, const uint32_t* items, float ox, float oy,
                             float g, float span, uint32_t nbx, uint32_t nby, uint32_t X, uint32_t Y, float res, uint32_t K,
                             const float* cell_x, const float* cell_y, int32_t* out, int32_t* overflow, hipStream_t s) {
    hipLaunchKernelGGL(knn_select_kernel, dim3(X * Y), dim3(256), 0, s, cx, cy, bucket_start, items, ox, oy, g, span, nbx, nby, X, Y, res, K,
                       cell_x, cell_y, out, overflow);
    return hipGetLastError();
}

}  // namespace rover
