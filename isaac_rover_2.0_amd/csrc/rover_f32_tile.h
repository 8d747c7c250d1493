// rover_f32_tile.h — THE 32 x 32 x 2 f32 tile core (v_mfma_f32_32x32x2_f32: exact f32 products, one rounding per accumulate) under the
// five per-layer kernels: linear_act (rover_mlp.hip), linear_wgrad / linear_dgrad (rover_train.hip), gru_cell / gru_cell_backward
// (rover_gru.hip).  A kernel is its operand functors, one f32_slabs() loop and its epilogue; a change of the tile design
// (more column tiles, a second LDS buffer) is made here.  NW = waves per workgroup throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rover {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// One LDS slab, R rows x C columns at a row pitch, and the staging map that fills it: thread tid holds the elements (row sr + 2 NW j,
// column 32 t + sc), sc = tid & 31, sr = tid >> 5, as register t (R / 2 NW) + j — 128-byte coalesced rows of whatever `at` reads.
template <int NW, int R, int C, int PITCH>
struct F32Slab {
    static constexpr uint32_t RSTEP = 2u * NW, NJ = R / RSTEP, NP = (C / 32) * NJ, WORDS = R * PITCH;
    float* s;
    // f(i, slab_row, slab_col) for each of the NP elements this thread stages, i its register
    template <class F>
    static __device__ __forceinline__ void each(F&& f) {
        const uint32_t sc = threadIdx.x & 31u, sr = threadIdx.x >> 5;
#pragma unroll
        for (int t = 0; t < C / 32; ++t)
#pragma unroll
            for (int j = 0; j < (int)NJ; ++j) f(t * (int)NJ + j, sr + RSTEP * j, 32u * t + sc);
    }
    // at(slab_row, slab_col) -> float forms the element: the bounds checks (zeros past the matrix) and the operand's arithmetic are its.
    // Name the global indices before checking them (const uint32_t gr = row0 + r, gk = k0 + c; ...): with the sums written inside the
    // short-circuit conditions hipcc doubled the SGPR spills of the GRU kernels (EXPERIMENTS.md §25).
    template <class At>
    static __device__ __forceinline__ void stage(float (&p)[NP], At&& at) {
        each([&](int i, uint32_t r, uint32_t c) { p[i] = at(r, c); });
    }
    __device__ __forceinline__ void stash(const float (&p)[NP]) const {
        each([&](int i, uint32_t r, uint32_t c) { s[r * PITCH + c] = p[i]; });
    }
};
// The MFMA operand of a lane is element (i = lane & 31, k = kk + (lane >> 5)) of a 32-wide tile t, for A[i][k] and B[k][j] alike.
// k-minor: [ROWS][32 k] at a pitch of 33 words (the column read of a 32-lane half falls on 32 banks)
template <int NW, int ROWS>
struct F32KMinor : F32Slab<NW, ROWS, 32, 33> {
    __device__ __forceinline__ float operand(uint32_t t, uint32_t kk) const {
        return this->s[(t * 32u + (threadIdx.x & 31u)) * 33u + kk + ((threadIdx.x & 63u) >> 5)];
    }
};
// k-major: [32 k][COLS] as the tensor lies, no padding (a row read of 32 consecutive words never conflicts)
template <int NW, int COLS>
struct F32KMajor : F32Slab<NW, 32, COLS, COLS> {
    __device__ __forceinline__ float operand(uint32_t t, uint32_t kk) const {
        return this->s[(kk + ((threadIdx.x & 63u) >> 5)) * COLS + t * 32u + (threadIdx.x & 31u)];
    }
};

template <int N>
__device__ __forceinline__ void f32_zero(f32x16 (&acc)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}

// The slab loop over reduction offsets lo, lo + 32, .. < end: fetch(o) fills the staged registers of the slab at o, stash(o) stores them
// to LDS, mid() runs on the staged slab before its k-steps, and a k-step (kk = 0, 2, .. 30) is step(kk) on the slabs before `split`,
// step_hi(kk) from there on: which accumulators a k-step feeds is chosen once per slab, uniformly, never inside the k-steps.  One LDS
// buffer, two barriers per slab; the slab after the current one is in flight during its MFMAs.
template <class Fetch, class Stash, class Mid, class Step, class StepHi>
__device__ __forceinline__ void f32_slabs(uint32_t lo, uint32_t end, Fetch&& fetch, Stash&& stash, Mid&& mid, Step&& step, uint32_t split,
                                          StepHi&& step_hi) {
    fetch(lo);
    for (uint32_t o = lo; o < end; o += 32u) {
        stash(o);
        __syncthreads();
        if (o + 32u < end) fetch(o + 32u);
        mid();
        if (o < split) {
#pragma unroll 4
            for (uint32_t kk = 0; kk < 32u; kk += 2) step(kk);
        } else {
#pragma unroll 4
            for (uint32_t kk = 0; kk < 32u; kk += 2) step_hi(kk);
        }
        __syncthreads();
    }
}
// one kind of k-step for the whole reduction
template <class Fetch, class Stash, class Mid, class Step>
__device__ __forceinline__ void f32_slabs(uint32_t lo, uint32_t end, Fetch&& fetch, Stash&& stash, Mid&& mid, Step&& step) {
    f32_slabs(lo, end, fetch, stash, mid, step, end, step);
}

// C/D layout of the 32 x 32 MFMA: accumulator register r of a lane is element (row, col) of the tile
struct F32Coord { uint32_t row, col; };
__device__ __forceinline__ F32Coord f32_cd(uint32_t lane, int r) {
    return F32Coord{(uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5), lane & 31u};
}

}  // namespace rover
