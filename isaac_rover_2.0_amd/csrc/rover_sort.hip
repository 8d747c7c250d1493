// rover_sort.hip — the bucket sort of the step's ray slots by (map, cell) and the generic three-level exclusive scan (gfx950, wave64).
// No reference counterpart: the reference casts every ray against its own cell's triangles in env order.
// Built with -ffp-contract=off: see rover_rays.hip.
// Kernels:
// * bucket_hist / rowscan / scatter / sort   bucket sort of the ray slots by (map, cell), LDS atomics only (3 - 4 launches)
//   scan_block_sums / scan_top / scan_apply kernels   launch_scan_exclusive, the KNN map builder's scan (f-3)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"
#include "rover_blockscan.h"

namespace rover {

// ---------------------------------------------------------------------------------------------------
// ray binning: sort of the step's rays by (map, cell).  At 65 536 envs a bin holds ~4-5 rays per step; sorted, the
// 3.6 KB cell block is fetched from HBM once per bin and served from registers to its rays.
// Results do not depend on the order inside a bin, so the LDS atomics do not make the step non-deterministic.
// The generic 3-level scan below now only serves the KNN map builder; the binning has its own row scan.
// ---------------------------------------------------------------------------------------------------
#define SCAN_ITEMS 8
#define SCAN_BLOCK 256
#define SCAN_TILE (SCAN_ITEMS * SCAN_BLOCK)

__global__ void __launch_bounds__(SCAN_BLOCK) scan_block_sums_kernel(const uint32_t* __restrict__ cnt, uint32_t n,
                                                                     uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t lds[SCAN_BLOCK / 64];
    uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS, sum = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) sum += (base + i < n) ? cnt[base + i] : 0u;
    uint32_t total;
    (void)block_exclusive_scan<SCAN_BLOCK / 64>(sum, lds, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: exclusive scan in place of up to 1024*SCAN_ITEMS block sums
__global__ void __launch_bounds__(1024) scan_top_kernel(uint32_t* __restrict__ block_sums, uint32_t nb) {
    __shared__ uint32_t lds[16];
    uint32_t base = threadIdx.x * SCAN_ITEMS, v[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { v[i] = (base + i < nb) ? block_sums[base + i] : 0u; sum += v[i]; }
    uint32_t total, run = block_exclusive_scan<16>(sum, lds, total);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { if (base + i < nb) block_sums[base + i] = run; run += v[i]; }
}

__global__ void __launch_bounds__(SCAN_BLOCK) scan_apply_kernel(uint32_t* __restrict__ cnt, uint32_t n,
                                                                const uint32_t* __restrict__ block_offsets) {
    __shared__ uint32_t lds[SCAN_BLOCK / 64];
    uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS, v[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { v[i] = (base + i < n) ? cnt[base + i] : 0u; sum += v[i]; }
    uint32_t total, run = block_exclusive_scan<SCAN_BLOCK / 64>(sum, lds, total) + block_offsets[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { if (base + i < n) cnt[base + i] = run; run += v[i]; }
}

// ---- bucket sort of the ray slots by bin = (map, cell), without returning global atomics ---------------------------
// (the only global atomics are the few per (tile, bucket) of the histogram pass fused into prep_rays_kernel: bin_hist_fused)
//   bucket_hist_kernel     per 4096-slot block: LDS histogram over the coarse buckets (bin >> low_bits) -> counts[block][bucket]
//                          (or prep_rays_kernel itself: bin_hist_fused)
//   bucket_rowscan_kernel  one workgroup per bucket: exclusive prefix along its row of block counts + the bucket total
//                          (the scan over the bucket totals is redone by every scatter block in LDS: <= 4096 values)
//   bucket_scatter_kernel  same blocks: (bin, slot) pairs to their bucket range, position from an LDS cursor per bucket
//   bucket_sort_kernel     one workgroup per bucket: LDS counting sort on the low bits -> sorted slot ids
// The order of equal bins is whatever the LDS atomics produce; the ray cast does not depend on it.
#define BKT_ITEMS 16
#define BKT_TILE (256 * BKT_ITEMS)
#define BKT_MAX 4096            // max coarse buckets, and max 2^low_bits
#define BKT_STAGE 8192u         // entries of a bucket that bucket_sort_kernel orders in LDS before writing them out

// NT threads take a tile of NT x 16 slots: 256 (4 096 slots), or 1 024 for big ray sets (launch_bin_rays)
template <int NT>
__global__ void __launch_bounds__(NT) bucket_hist_kernel(const uint32_t* __restrict__ bins, uint32_t n_slots, uint32_t low_bits,
                                                          uint32_t n_buckets, uint32_t n_blocks, uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[BKT_MAX];
    for (uint32_t i = threadIdx.x; i < n_buckets; i += NT) h[i] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (NT * BKT_ITEMS);
    uint32_t bv[BKT_ITEMS];                                   // all 16 loads in flight before the first atomic (the kernel is latency-bound)
#pragma unroll
    for (uint32_t it = 0; it < BKT_ITEMS; ++it) {
        const uint32_t i = base + it * NT + threadIdx.x;
        bv[it] = i < n_slots ? bins[i] : 0xffffffffu;
    }
#pragma unroll
    for (uint32_t it = 0; it < BKT_ITEMS; ++it)
        if (bv[it] != 0xffffffffu) atomicAdd(&h[bv[it] >> low_bits], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_buckets; i += NT) counts[(size_t)blockIdx.x * n_buckets + i] = h[i];   // [block][bucket]: coalesced
}

// counts[bucket][block] -> exclusive prefix inside every bucket row (one workgroup per bucket) + the row total
// counts [block][bucket] -> exclusive prefix over the BLOCKS, in place, and the bucket totals.  One workgroup per 16 buckets, 16 waves;
// a wave takes 64 consecutive blocks of a 1 024-block tile: lane (kb = lane & 15, ph = lane >> 4) holds bucket kb of blocks b0 + 4 j + ph,
// j < 16, in registers — one round of loads (four 64-byte rows per instruction), a register / cross-lane scan, one round of stores.
// (The table was [bucket][block] with one workgroup scanning a row: the histogram's 720 k stores and the scatter's 720 k loads were
// 4 bytes at a 4 KB stride; as [block][bucket] with one lane per bucket and 64 buckets per workgroup only 11 CUs worked: 10.6 us.)
#define RSCAN_WAVES 16
__global__ void __launch_bounds__(64 * RSCAN_WAVES) bucket_rowscan_kernel(uint32_t* __restrict__ counts, uint32_t n_blocks, uint32_t n_buckets,
                                                                          uint32_t* __restrict__ bucket_tot) {
    __shared__ uint32_t part[RSCAN_WAVES][16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, kb = lane & 15u, ph = lane >> 4;
    const uint32_t k = blockIdx.x * 16u + kb;
    const bool kin = k < n_buckets;
    uint32_t carry = 0;                                              // rays of this bucket in the tiles before
    for (uint32_t tile0 = 0; tile0 < n_blocks; tile0 += 64u * RSCAN_WAVES) {
        const uint32_t b0 = tile0 + w * 64u + ph;                    // this lane's blocks: b0 + 4 j
        uint32_t* __restrict__ p = counts + (size_t)b0 * n_buckets + (kin ? k : 0u);
        uint32_t v[16], ex[16], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) v[j] = (kin && b0 + 4u * j < n_blocks) ? p[(size_t)(4u * j) * n_buckets] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            // blocks 4 j .. 4 j + 3 sit in the four lane groups: inclusive scan over ph, then this lane's exclusive share
            uint32_t inc = v[j];
            uint32_t o = (uint32_t)__shfl_up((int)inc, 16, 64); if (ph >= 1u) inc += o;
            o = (uint32_t)__shfl_up((int)inc, 32, 64);          if (ph >= 2u) inc += o;
            const uint32_t four = (uint32_t)__shfl((int)inc, 48 + (int)kb, 64);       // all four blocks of this j
            ex[j] = sum + inc - v[j];
            sum += four;
        }
        if (ph == 0u) part[w][kb] = sum;
        __syncthreads();
        uint32_t run = carry, total = 0;
#pragma unroll
        for (uint32_t i = 0; i < RSCAN_WAVES; ++i) { const uint32_t c = part[i][kb]; run += i < w ? c : 0u; total += c; }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j)
            if (kin && b0 + 4u * j < n_blocks) p[(size_t)(4u * j) * n_buckets] = run + ex[j];
        carry += total;
    }
    if (w == 0 && ph == 0u && kin) bucket_tot[k] = carry;
}

// PACKED: an entry is one dword, low bin bits << (32 - low_bits) | slot — all bucket_sort_kernel reads of a pair — when the slot
// ids leave room for them (n_slots <= 2^(32 - low_bits): 65 536 envs x 64 slots with 1 024 bins per bucket just fit); half the
// scatter's writes and half the sort's reads.  Otherwise (bin, slot) as two dwords.
template <bool PACKED> struct BktEntry;
template <> struct BktEntry<false> {
    typedef uint2 T;
    static __device__ __forceinline__ T make(uint32_t bin, uint32_t slot, uint32_t) { return make_uint2(bin, slot); }
    static __device__ __forceinline__ T none() { return make_uint2(0u, 0xffffffffu); }
    static __device__ __forceinline__ uint32_t lo(T v, uint32_t low_bits) { return v.x & ((1u << low_bits) - 1u); }
    static __device__ __forceinline__ uint32_t slot(T v, uint32_t) { return v.y; }
};
template <> struct BktEntry<true> {
    typedef uint32_t T;
    static __device__ __forceinline__ T make(uint32_t bin, uint32_t slot, uint32_t low_bits) { return (bin << (32u - low_bits)) | slot; }
    static __device__ __forceinline__ T none() { return 0xffffffffu; }
    static __device__ __forceinline__ uint32_t lo(T v, uint32_t low_bits) { return v >> (32u - low_bits); }
    static __device__ __forceinline__ uint32_t slot(T v, uint32_t low_bits) { return v & (0xffffffffu >> low_bits); }
};

// Every block turns the bucket totals into bucket start offsets in LDS (n_buckets <= 4096: 16 values per thread); block 0 also
// publishes them (plus the grand total) for bucket_sort_kernel.  The block's 4 096 entries are first ordered by bucket in LDS
// (rank from one LDS atomic per entry, local start from a scan of the block's bucket counts) next to their global positions, then
// written out in that order: neighbouring lanes then write neighbouring entries of a bucket's run (~6 per bucket and block) and the
// run leaves as one or two write transactions instead of one per entry.
template <bool PACKED, int NT>
__global__ void __launch_bounds__(NT) bucket_scatter_kernel(const uint32_t* __restrict__ bins, uint32_t n_slots, uint32_t low_bits,
                                                             uint32_t n_buckets, uint32_t n_blocks, const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ bucket_tot, uint32_t* __restrict__ bucket_base,
                                                             uint2* __restrict__ pairs2) {
    typedef BktEntry<PACKED> En;
    typename En::T* __restrict__ pairs = reinterpret_cast<typename En::T*>(pairs2);
    extern __shared__ __attribute__((aligned(8))) uint32_t bkt_lds[];        // sized by the launch: 2 n_buckets + (NT * BKT_ITEMS) (1 + dwords per entry) dwords
    uint32_t* const cur = bkt_lds;               // global position of this block's first entry in each bucket
    uint32_t* const cnt = cur + n_buckets;       // this block's entries per bucket -> their local start
    uint32_t* const s_dst = cnt + n_buckets;
    typename En::T* const s_val = reinterpret_cast<typename En::T*>(s_dst + (NT * BKT_ITEMS));      // (an even dword offset from an 8-byte aligned base: two-dword entries stay 8-byte aligned)
    __shared__ uint32_t wl[NT / 64];
    const uint32_t per = (n_buckets + NT - 1u) / NT, first = threadIdx.x * per;
    const uint32_t base = blockIdx.x * (NT * BKT_ITEMS);
    uint32_t bv[BKT_ITEMS], rk[BKT_ITEMS];                    // the block's 16 loads per thread go out first: their latency passes
#pragma unroll                                               // under the bucket-offset scan below
    for (uint32_t it = 0; it < BKT_ITEMS; ++it) {
        const uint32_t i = base + it * NT + threadIdx.x;
        bv[it] = i < n_slots ? bins[i] : 0xffffffffu;
    }
    {
        uint32_t sum = 0;
        for (uint32_t j = 0; j < per; ++j) sum += (first + j < n_buckets) ? bucket_tot[first + j] : 0u;
        uint32_t total, run = block_exclusive_scan<NT / 64>(sum, wl, total);
        for (uint32_t j = 0; j < per; ++j) {
            const uint32_t i = first + j;
            if (i < n_buckets) {
                cur[i] = run + offsets[(size_t)blockIdx.x * n_buckets + i];
                cnt[i] = 0u;
                if (blockIdx.x == 0) bucket_base[i] = run;
                run += bucket_tot[i];
            }
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) bucket_base[n_buckets] = total;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t it = 0; it < BKT_ITEMS; ++it) rk[it] = bv[it] != 0xffffffffu ? atomicAdd(&cnt[bv[it] >> low_bits], 1u) : 0u;
    __syncthreads();
    uint32_t n_here;
    {
        uint32_t sum = 0;
        for (uint32_t j = 0; j < per; ++j) sum += (first + j < n_buckets) ? cnt[first + j] : 0u;
        uint32_t run = block_exclusive_scan<NT / 64>(sum, wl, n_here);
        for (uint32_t j = 0; j < per; ++j) {
            const uint32_t i = first + j;
            if (i < n_buckets) { const uint32_t c = cnt[i]; cnt[i] = run; run += c; }
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t it = 0; it < BKT_ITEMS; ++it) {
        if (bv[it] != 0xffffffffu) {
            const uint32_t b = bv[it] >> low_bits, l = cnt[b] + rk[it];
            s_dst[l] = cur[b] + rk[it];
            s_val[l] = En::make(bv[it], base + it * NT + threadIdx.x, low_bits);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n_here; k += NT) pairs[s_dst[k]] = s_val[k];
}

template <bool PACKED, int NT, int IPT>      // IPT: items a thread may hold (buckets of up to NT x IPT entries take the one-pass path)
__global__ void __launch_bounds__(NT) bucket_sort_kernel(const uint2* __restrict__ pairs2, const uint32_t* __restrict__ bucket_base,
                                                          uint32_t low_bits, uint32_t* __restrict__ sorted, uint32_t* __restrict__ zero,
                                                          uint32_t n_zero) {
    typedef BktEntry<PACKED> En;
    const typename En::T* __restrict__ pairs = reinterpret_cast<const typename En::T*>(pairs2);
    extern __shared__ uint32_t bkt_lds[];        // sized by the launch: 2^low_bits + BKT_STAGE dwords
    __shared__ uint32_t wl[NT / 64];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, nl = 1u << low_bits;
    if (zero) {      // the count table is spent (the scatter has run): cleared for the next step's prep_rays_kernel, a share per block
        const uint32_t per = (n_zero + gridDim.x - 1u) / gridDim.x, z1 = min(n_zero, (b + 1u) * per);
        for (uint32_t i = b * per + tid; i < z1; i += NT) zero[i] = 0u;
    }
    uint32_t* const h = bkt_lds;
    uint32_t* const stage = bkt_lds + nl;
    const uint32_t s0 = bucket_base[b], s1 = bucket_base[b + 1u];
    if (s1 <= s0) return;
    for (uint32_t i = tid; i < nl; i += NT) h[i] = 0;
    __syncthreads();
    if (s1 - s0 <= (uint32_t)(NT * IPT)) {
        // The usual bucket (6-12 k rays): ONE pass of LDS atomics.  A thread keeps its <= 64 items in registers with the rank the
        // histogram atomic returned (rank inside the bin), so after the scan the position is start[bin] + rank — no second read of
        // the pairs and no second round of atomics.
        uint32_t slot[IPT], br[IPT];                                 // br = low bin bits | rank << 12
#pragma unroll
        for (int g = 0; g < IPT / 8; ++g) {
            typename En::T pv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { const uint32_t k = s0 + tid + (uint32_t)(8 * g + j) * NT; pv[j] = k < s1 ? pairs[k] : En::none(); }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t k = s0 + tid + (uint32_t)(8 * g + j) * NT, lo = En::lo(pv[j], low_bits);
                slot[8 * g + j] = En::slot(pv[j], low_bits);
                br[8 * g + j] = k < s1 ? (lo | (atomicAdd(&h[lo], 1u) << 12)) : 0u;
            }
        }
        __syncthreads();
        const uint32_t per = (nl + NT - 1u) / NT, first = tid * per;
        uint32_t sum = 0;
        for (uint32_t j = 0; j < per; ++j) sum += first + j < nl ? h[first + j] : 0u;
        uint32_t total, run = block_exclusive_scan<NT / 64>(sum, wl, total);
        for (uint32_t j = 0; j < per; ++j) if (first + j < nl) { const uint32_t c = h[first + j]; h[first + j] = run; run += c; }
        __syncthreads();
        // through LDS: a wave's 64 positions are anywhere in the bucket's 24-48 KB of output, 64 partial-line writes per store
        // instruction (4.1 M L2 write transactions a launch); staged, the bucket leaves in whole lines
        if (s1 - s0 <= BKT_STAGE) {
#pragma unroll
            for (int i = 0; i < IPT; ++i) {
                const uint32_t k = s0 + tid + (uint32_t)i * NT;
                if (k < s1) stage[h[br[i] & 0xfffu] + (br[i] >> 12)] = slot[i];
            }
            __syncthreads();
            for (uint32_t k = tid; k < s1 - s0; k += NT) sorted[s0 + k] = stage[k];
            return;
        }
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const uint32_t k = s0 + tid + (uint32_t)i * NT;
            if (k < s1) sorted[s0 + h[br[i] & 0xfffu] + (br[i] >> 12)] = slot[i];
        }
        return;
    }
    // eight loads in flight per thread before their atomics: the kernel waits on memory 93 % of the time otherwise
    for (uint32_t k0 = s0 + tid; k0 < s1; k0 += 8u * NT) {
        typename En::T bx[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const uint32_t k = k0 + (uint32_t)j * NT; bx[j] = k < s1 ? pairs[k] : En::none(); }
#pragma unroll
        for (int j = 0; j < 8; ++j) if (k0 + (uint32_t)j * NT < s1) atomicAdd(&h[En::lo(bx[j], low_bits)], 1u);
    }
    __syncthreads();
    // exclusive scan of h[0..nl): each thread owns ceil(nl / NT) consecutive entries
    const uint32_t per = (nl + NT - 1u) / NT, first = tid * per;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < per; ++j) sum += first + j < nl ? h[first + j] : 0u;
    uint32_t total, run = block_exclusive_scan<NT / 64>(sum, wl, total);
    for (uint32_t j = 0; j < per; ++j) if (first + j < nl) { const uint32_t c = h[first + j]; h[first + j] = run; run += c; }
    __syncthreads();
    for (uint32_t k0 = s0 + tid; k0 < s1; k0 += 8u * NT) {
        typename En::T pv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const uint32_t k = k0 + (uint32_t)j * NT; pv[j] = k < s1 ? pairs[k] : En::none(); }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k0 + (uint32_t)j * NT < s1) sorted[s0 + atomicAdd(&h[En::lo(pv[j], low_bits)], 1u)] = En::slot(pv[j], low_bits);
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
// tile of the sort's first two passes: 4 096 slots per 256-thread block; from 2 M slots 16 384 per 1 024-thread block — a (block, bucket)
// run of the scatter is then ~23 entries instead of ~6 (its partial-line writes were 9 of its 21 us at 65 536 envs) and the count
// table a quarter of the rows; small batches keep the small tile (more blocks than CUs matter more there)
// a sort entry is one dword — slot ids leave room for the low bin bits — (else (bin, slot) as two): the one place that decides it
bool bin_entries_packed(uint32_t n_slots, uint32_t low_bits) { return (uint64_t)n_slots <= (1ull << (32u - low_bits)); }
static inline uint32_t bin_tile_threads(uint32_t n_slots, bool packed) {
    const bool big = n_slots >= (2u << 20);
    return big ? (packed ? 1024u : 512u) : 256u;                                  // (two-dword entries: 12 bytes of LDS per slot, 8 192 slots)
}

// The sort's first pass — keys per (tile, coarse bucket) — can run inside prep_rays_kernel when the keys of one of its 64-env blocks lie
// in ONE tile (the tile is a multiple of 64 x R8 slots: R8 = 64 with the default 37 + 26 rays); the blocks of a tile add their LDS
// histograms to the tile's row, which therefore has to be zero when the step starts: bucket_sort_kernel, the sort's last pass, clears
// the table again.  One launch less per step (6.1 us at 65 536 envs, 4.7 at 4 096); other ray counts keep bucket_hist_kernel.
bool bin_hist_fused(uint32_t n_slots, uint32_t R8, uint32_t n_bins, uint32_t low_bits, uint32_t* blocks_per_tile) {
    const uint32_t n_buckets = (n_bins + (1u << low_bits) - 1u) >> low_bits;
    const uint32_t tile = bin_tile_threads(n_slots, bin_entries_packed(n_slots, low_bits)) * BKT_ITEMS, keys = 64u * R8;      // keys of a prep_rays block's 64 envs
    if (low_bits < 8u || low_bits > 12u || n_buckets > 1024u || keys > tile || tile % keys != 0u) return false;
    *blocks_per_tile = tile / keys;
    return true;
}

// sort the valid ray slots by bin; work = [counts/offsets table | pairs]; returns hipErrorInvalidValue when the bin space is too large
hipError_t launch_bin_rays(const uint32_t* bins, uint32_t n_slots, uint32_t n_valid, uint32_t n_bins, uint32_t low_bits, bool packed,
                           uint32_t* table, uint2* pairs, uint32_t* block_sums, uint32_t* sorted, bool hist_done, hipStream_t s) {
    const uint32_t n_buckets = (n_bins + (1u << low_bits) - 1u) >> low_bits;
    if (low_bits < 8u || low_bits > 12u || n_buckets > BKT_MAX) return hipErrorInvalidValue;
    const bool big = n_slots >= (2u << 20);
    if (packed != bin_entries_packed(n_slots, low_bits)) return hipErrorInvalidValue;
    const uint32_t nt = bin_tile_threads(n_slots, packed), tile = nt * BKT_ITEMS;
    const uint32_t n_blocks = blocks_for(n_slots, tile);
    uint32_t* bucket_tot = block_sums;                 // [BKT_MAX]
    uint32_t* const zero = hist_done ? table : nullptr;         // counted by prep_rays_kernel: the table has to be zero again after this sort
    const uint32_t n_zero = n_blocks * n_buckets;
    uint32_t* bucket_base = block_sums + BKT_MAX;      // [BKT_MAX + 1]
    const uint32_t scatter_lds = (2u * n_buckets + (packed ? 2u : 3u) * tile + 2u) * 4u, sort_lds = ((1u << low_bits) + BKT_STAGE) * 4u;
#define BKT_LAUNCH(PK, NT)                                                                                                            \
    do {                                                                                                                              \
        if (!hist_done) hipLaunchKernelGGL(bucket_hist_kernel<NT>, dim3(n_blocks), dim3(NT), 0, s, bins, n_slots, low_bits, n_buckets, n_blocks, table); \
        hipLaunchKernelGGL(bucket_rowscan_kernel, dim3(blocks_for(n_buckets, 16)), dim3(64 * RSCAN_WAVES), 0, s, table, n_blocks, n_buckets, bucket_tot); \
        hipLaunchKernelGGL((bucket_scatter_kernel<PK, NT>), dim3(n_blocks), dim3(NT), scatter_lds, s, bins, n_slots, low_bits, n_buckets, n_blocks, \
                           table, bucket_tot, bucket_base, pairs);                                                                   \
        /* buckets of <= 16 384 entries: 512 threads x 32; mean bucket above 8 192 (dense ray sets: the terrain buckets of 65 536 envs x 120 rays hold 22 k): 1 024 x 32 */ \
        if ((uint64_t)n_valid > 8192ull * n_buckets)                                                                                  \
            hipLaunchKernelGGL((bucket_sort_kernel<PK, 1024, 32>), dim3(n_buckets), dim3(1024), sort_lds, s, pairs, bucket_base, low_bits, sorted, zero, n_zero); \
        else                                                                                                                          \
            hipLaunchKernelGGL((bucket_sort_kernel<PK, 512, 32>), dim3(n_buckets), dim3(512), sort_lds, s, pairs, bucket_base, low_bits, sorted, zero, n_zero);     \
    } while (0)
    if (big) {      // more than 64 KB of dynamic LDS: the kernel has to be told (once per size)
        static uint32_t raised_of[64][2] = {};       // per device: the attribute belongs to the function on the current device
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        uint32_t* raised = raised_of[dev];
        if (scatter_lds > raised[packed]) {
            const void* f = packed ? reinterpret_cast<const void*>(&bucket_scatter_kernel<true, 1024>) : reinterpret_cast<const void*>(&bucket_scatter_kernel<false, 512>);
            const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)scatter_lds);
            if (e != hipSuccess) return e;
            raised[packed] = scatter_lds;
        }
    }
    if (packed) { if (big) BKT_LAUNCH(true, 1024); else BKT_LAUNCH(true, 256); }
    else { if (big) BKT_LAUNCH(false, 512); else BKT_LAUNCH(false, 256); }
#undef BKT_LAUNCH
    return hipGetLastError();
}

hipError_t launch_scan_exclusive(uint32_t* data, uint32_t n, uint32_t* block_sums, hipStream_t s) {
    const uint32_t nb = blocks_for(n, SCAN_TILE);
    if (nb > 1024u * SCAN_ITEMS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, s, data, n, block_sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(1024), 0, s, block_sums, nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, s, data, n, block_sums);
    return hipGetLastError();
}

}  // namespace rover
