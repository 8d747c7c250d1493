// rover_mars.hip — the heightfield of the reference's Mars terrain generator from a plan of hills and rock stamps (rover_mars_heightfield;
// the definition is written out in include/rover_step.h and DESIGN.md §4.21).
//
// A gather: one workgroup per MARS_TILE x MARS_TILE nodes (256 threads, one node each; neighbouring lanes on neighbouring columns).
// A node starts at 0.0, adds every hill that covers it in index order — a loop over ALL hills with wave-uniform bounds, a hill whose
// window misses the tile is skipped by the whole workgroup, g comes through L2 — and then every kept stamp that covers it in ascending
// stamp order: the host lists the tile's stamps (mars_fill_lists in rover_capi_scene.cpp, the code rover_mars_tiles runs), the workgroup stages
// MARS_CHUNK records at a time in LDS and every thread walks them in order (all lanes read the same record: an LDS broadcast).  Nothing
// is scattered, so there are no atomics and the bits do not depend on the launch order.
//
// Every product and sum is written with __dmul_rn / __dadd_rn (and the library is built with -ffp-contract=off): one IEEE float64
// rounding each, as numpy's `field[slice] += table * factor` does them.  The kernel is gather- and latency-bound; its FP64 work is two
// operations per (node, covering item).
//
// Bounds: rover_mars_heightfield validates the descriptor before anything is uploaded — every window lies inside the field and inside
// g, every kept stamp's square inside the field, every class inside its table — so the indices below stay inside their buffers; a
// thread outside the field (a ragged last tile) takes part in the barriers and touches no memory.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"

namespace rover {

static_assert(MARS_TILE * MARS_TILE == 256, "one thread per node of a tile");

__global__ void __launch_bounds__(256) mars_heightfield_kernel(MarsArgs a) {
    __shared__ MarsStamp s_stamp[MARS_CHUNK];
    const uint32_t tile = blockIdx.x;
    const int32_t ti = (int32_t)(tile / a.tiles_c), tj = (int32_t)(tile % a.tiles_c);
    const int32_t tr0 = ti * MARS_TILE, tc0 = tj * MARS_TILE;
    const int32_t r = tr0 + (int32_t)(threadIdx.x >> 4), c = tc0 + (int32_t)(threadIdx.x & 15u);
    const bool inside = r < a.rows && c < a.cols;
    double h = 0.0;
    for (int32_t i = 0; i < a.n_hills; ++i) {
        const MarsHill w = a.hills[i];
        if (w.r1 <= tr0 || w.r0 >= tr0 + MARS_TILE || w.c1 <= tc0 || w.c0 >= tc0 + MARS_TILE) continue;      // (workgroup-uniform)
        if (inside && r >= w.r0 && r < w.r1 && c >= w.c0 && c < w.c1)
            h = __dadd_rn(h, __dmul_rn(__dmul_rn(a.g[w.a0 + (r - w.r0)], a.g[w.b0 + (c - w.c0)]), w.amp));
    }
    const int32_t begin = a.tile_start[tile], end = a.tile_start[tile + 1];
    bool rock = false;
    for (int32_t base = begin; base < end; base += MARS_CHUNK) {
        const int32_t n = min(end - base, (int32_t)MARS_CHUNK);
        if (base != begin) __syncthreads();              // the previous chunk has been walked by every thread
        for (int32_t i = (int32_t)threadIdx.x; i < n; i += 256) s_stamp[i] = a.stamps[a.tile_items[base + i]];
        __syncthreads();
        if (inside) {
            for (int32_t i = 0; i < n; ++i) {
                const MarsStamp s = s_stamp[i];
                const uint32_t dr = (uint32_t)(r - s.row), dc = (uint32_t)(c - s.col);      // (negative wraps to a huge value)
                if (dr < s.side && dc < s.side) {
                    h = __dadd_rn(h, __dmul_rn(a.tables[s.table + dr * s.side + dc], s.factor));
                    rock = true;
                }
            }
        }
    }
    if (inside) {
        const uint64_t at = (uint64_t)r * (uint32_t)a.cols + (uint32_t)c;
        a.hf[at] = h;
        if (a.mask) a.mask[at] = rock ? 1 : 0;
    }
}

hipError_t launch_mars_heightfield(const MarsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mars_heightfield_kernel, dim3(a.tiles_r * a.tiles_c), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rover
