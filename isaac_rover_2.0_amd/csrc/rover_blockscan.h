// rover_blockscan.h — two workgroup-wide primitives on wave64: the exclusive scan of one value per thread and the count of a flag
// per 256-thread block.  Users: the scans and the bucket sort (rover_sort.hip), the done count and the compaction (rover_obs.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rover {

// exclusive scan of one value per thread across a workgroup of NW waves; returns the exclusive prefix, total via ref
template <int NW>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds /*[NW]*/, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= (uint32_t)off) inc += o;
    }
    if (lane == 63u) lds[w] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { uint32_t c = lds[i]; wbase += ((uint32_t)i < w) ? c : 0u; tot += c; }
    __syncthreads();
    total = tot;
    return wbase + inc - v;
}

__device__ __forceinline__ void block_count_flags(bool flag, uint32_t* __restrict__ block_cnt, uint32_t bid) {
    __shared__ uint32_t wcnt[4];
    unsigned long long ballot = __ballot(flag);
    if ((threadIdx.x & 63u) == 0u) wcnt[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[bid] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

}  // namespace rover
