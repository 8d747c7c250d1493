// rover_track.hip — episode statistics on the device (rover_episode_track; the definition is written out in include/rover_step.h and
// DESIGN.md §4.17): per-env cumulative reward and step count, the ring of the last W finished episodes, the interval record.
//
// Two launches per env step, no atomics, no host read:
//   track_update_kernel   ceil(E / 256) workgroups, one thread per env: step 1 of the definition; the workgroup's finished (return,
//                         length) pairs are compacted in env order into its own 256 scratch slots (ballot + popcount, as the done
//                         compaction in rover_obs.hip), and its minima, maxima and sums go into one TrackPartial — xor butterflies
//                         inside a wave, then the four waves in wave order: a fixed tree
//   track_merge_kernel    one workgroup: folds the partials (the f64 columns by 8 slices of workgroups in workgroup order, then the 8
//                         slices in a fixed tree), scans the per-workgroup counts in chunks of 256 workgroups, copies the last
//                         min(n_finished, W) pairs into the ring, reduces the ring's valid slots and updates the record
// Both loop where there is more than one item per thread; the order of every f64 addition depends on E, W and K alone.
//
// Built with -ffp-contract=off: c = cum_reward + reward is one f32 add (tests/track_ref.py restates it in numpy float32).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rover_step.h"
#include "rover_internal.h"

namespace rover {

static_assert(TRACK_MAX_COMP == ROVER_TRACK_MAX_COMPONENTS, "the internal and the public component limits are one number");
static_assert(sizeof(rover_track_record) == 240, "rover_track_record has a fixed layout");

#define TRACK_NSUM (3 + TRACK_MAX_COMP)        // the f64 columns: inst_sum, ep_ret_sum, ep_ret_sumsq, comp_sum[16]
#define TRACK_SLICES 8                         // the merge kernel folds the f64 columns as 8 slices x 32 columns

struct TrackPartial {                          // what one update workgroup hands to the merge kernel
    double sum[TRACK_NSUM];
    int64_t ep_len_sum;
    float inst_min, inst_max, ep_ret_min, ep_ret_max;
    int32_t ep_len_min, ep_len_max;
    uint32_t ep_count, pad;
};
static_assert(sizeof(TrackPartial) == 192, "the partial record is 192 bytes");

uint32_t track_partial_bytes() { return (uint32_t)sizeof(TrackPartial); }

// The caller's scratch for `nparts` update workgroups: the partial records, then 256 finished returns per workgroup, then the lengths
struct TrackScratch {
    TrackPartial* parts;
    float* fin_ret;
    int32_t* fin_len;
    __device__ TrackScratch(void* base, uint32_t nparts)
        : parts(reinterpret_cast<TrackPartial*>(base)), fin_ret(reinterpret_cast<float*>(parts + nparts)),
          fin_len(reinterpret_cast<int32_t*>(fin_ret + (uint64_t)nparts * TRACK_BLOCK)) {}
};

// minimum / maximum with -0 below +0, so that the result does not depend on the order of the operands
__device__ __forceinline__ float omin(float a, float b) { return (b < a || (b == a && __builtin_signbitf(b))) ? b : a; }
__device__ __forceinline__ float omax(float a, float b) { return (b > a || (b == a && !__builtin_signbitf(b))) ? b : a; }

// the scalars a workgroup reduces together: one pass of butterflies, one exchange through LDS
struct TrackScal {
    double dsum;
    int64_t lsum;
    float fmin[2], fmax[2];
    int32_t imin, imax;
    uint32_t cnt;
};

__device__ __forceinline__ TrackScal scal_identity() {
    TrackScal v;
    v.dsum = 0.0; v.lsum = 0; v.cnt = 0u;
    v.fmin[0] = v.fmin[1] = __builtin_inff(); v.fmax[0] = v.fmax[1] = -__builtin_inff();
    v.imin = INT32_MAX; v.imax = INT32_MIN;
    return v;
}

__device__ __forceinline__ TrackScal scal_combine(const TrackScal& a, const TrackScal& b) {
    TrackScal v;
    v.dsum = a.dsum + b.dsum; v.lsum = a.lsum + b.lsum; v.cnt = a.cnt + b.cnt;
#pragma unroll
    for (int i = 0; i < 2; ++i) { v.fmin[i] = omin(a.fmin[i], b.fmin[i]); v.fmax[i] = omax(a.fmax[i], b.fmax[i]); }
    v.imin = min(a.imin, b.imin); v.imax = max(a.imax, b.imax);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// every thread of the 256 ends with the combination of all 256 values: butterflies in the wave, then waves 0..3 in order
__device__ __forceinline__ TrackScal block_combine(TrackScal v, TrackScal* __restrict__ lds4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        TrackScal o;
        o.dsum = __shfl_xor(v.dsum, off, 64); o.lsum = __shfl_xor(v.lsum, off, 64); o.cnt = __shfl_xor(v.cnt, off, 64);
        o.fmin[0] = __shfl_xor(v.fmin[0], off, 64); o.fmin[1] = __shfl_xor(v.fmin[1], off, 64);
        o.fmax[0] = __shfl_xor(v.fmax[0], off, 64); o.fmax[1] = __shfl_xor(v.fmax[1], off, 64);
        o.imin = __shfl_xor(v.imin, off, 64); o.imax = __shfl_xor(v.imax, off, 64);
        v = scal_combine(v, o);
    }
    if ((threadIdx.x & 63u) == 0u) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    TrackScal r = scal_combine(scal_combine(lds4[0], lds4[1]), scal_combine(lds4[2], lds4[3]));
    __syncthreads();                           // lds4 may be written again
    return r;
}

__global__ void __launch_bounds__(TRACK_BLOCK) track_update_kernel(TrackArgs a) {
    __shared__ double s_sum[4][TRACK_NSUM];
    __shared__ TrackScal s_scal[4];
    __shared__ uint32_t s_cnt[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t e = blockIdx.x * (uint32_t)TRACK_BLOCK + tid;
    const bool live = e < a.E;
    const uint32_t nsum = 3u + a.K;
    const TrackScratch sc(a.scratch, gridDim.x);
    TrackPartial* __restrict__ part = sc.parts + blockIdx.x;
    float* __restrict__ fin_ret = sc.fin_ret + (uint64_t)blockIdx.x * TRACK_BLOCK;           // this workgroup's 256 slots
    int32_t* __restrict__ fin_len = sc.fin_len + (uint64_t)blockIdx.x * TRACK_BLOCK;

    // 1. per env
    float r = 0.0f, c = 0.0f;
    int32_t n = 0;
    bool fin = false;
    if (live) {
        r = a.rewards[e];
        fin = a.done8 ? (reinterpret_cast<const int64_t*>(a.done)[e] != 0) : (reinterpret_cast<const uint8_t*>(a.done)[e] != 0);
        c = a.cum_reward[e] + r;
        n = a.cum_steps[e] + 1;
        a.cum_reward[e] = fin ? 0.0f : c;
        a.cum_steps[e] = fin ? 0 : n;
    }

    // the workgroup's finished pairs, in env order
    const unsigned long long ballot = __ballot(fin);
    if (lane == 0u) s_cnt[w] = (uint32_t)__popcll(ballot);

    // the f64 columns: one butterfly each, lane 0 of every wave keeps the wave's sum
    {
        const double s0 = wave_sum(live ? (double)r : 0.0);
        const double s1 = wave_sum(fin ? (double)c : 0.0);
        const double s2 = wave_sum(fin ? (double)c * (double)c : 0.0);          // exact: 48 significant bits
        if (lane == 0u) { s_sum[w][0] = s0; s_sum[w][1] = s1; s_sum[w][2] = s2; }
    }
    for (uint32_t k = 0; k < a.K; ++k) {
        double x = 0.0;
        if (live) x = ((a.comp_i64 >> k) & 1u) ? (double)reinterpret_cast<const int64_t*>(a.comp[k])[e] : (double)reinterpret_cast<const float*>(a.comp[k])[e];
        x = wave_sum(x);
        if (lane == 0u) s_sum[w][3u + k] = x;
    }

    TrackScal v = scal_identity();
    if (live) { v.fmin[0] = r; v.fmax[0] = r; }
    if (fin) { v.fmin[1] = c; v.fmax[1] = c; v.imin = n; v.imax = n; v.lsum = n; v.cnt = 1u; }
    v = block_combine(v, s_scal);              // its barriers also publish s_cnt and s_sum

    if (fin) {
        uint32_t woff = 0;
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) woff += (u < w) ? s_cnt[u] : 0u;
        const uint32_t pos = woff + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));      // < 256: inside this workgroup's slots
        fin_ret[pos] = c;
        fin_len[pos] = n;
    }
    if (tid < (uint32_t)TRACK_NSUM)
        part->sum[tid] = (tid < nsum) ? (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]) : 0.0;
    if (tid == 0u) {
        part->ep_len_sum = v.lsum;
        part->inst_min = v.fmin[0]; part->inst_max = v.fmax[0];
        part->ep_ret_min = v.fmin[1]; part->ep_ret_max = v.fmax[1];
        part->ep_len_min = v.imin; part->ep_len_max = v.imax;
        part->ep_count = v.cnt; part->pad = 0u;
    }
}

__global__ void __launch_bounds__(TRACK_BLOCK) track_merge_kernel(TrackArgs a, uint32_t nparts) {
    __shared__ double s_slice[TRACK_SLICES][32];
    __shared__ TrackScal s_scal[4];
    __shared__ uint32_t s_wtot[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t nsum = 3u + a.K;
    const TrackScratch sc(a.scratch, nparts);
    const TrackPartial* __restrict__ parts = sc.parts;
    const float* __restrict__ fin_ret = sc.fin_ret;
    const int32_t* __restrict__ fin_len = sc.fin_len;
    rover_track_record* __restrict__ rec = reinterpret_cast<rover_track_record*>(a.record);

    // the f64 columns: thread (slice, column) adds the workgroups slice, slice + 8, ... in that order
    {
        const uint32_t col = tid & 31u, slice = tid >> 5;
        double acc = 0.0;
        if (col < nsum)
            for (uint32_t p = slice; p < nparts; p += (uint32_t)TRACK_SLICES) acc = acc + parts[p].sum[col];
        s_slice[slice][col] = acc;
    }
    // the scalars: thread t takes the workgroups t, t + 256, ...
    TrackScal v = scal_identity();
    for (uint32_t p = tid; p < nparts; p += (uint32_t)TRACK_BLOCK) {
        const TrackPartial& q = parts[p];
        v.lsum += q.ep_len_sum; v.cnt += q.ep_count;
        v.fmin[0] = omin(v.fmin[0], q.inst_min); v.fmax[0] = omax(v.fmax[0], q.inst_max);
        v.fmin[1] = omin(v.fmin[1], q.ep_ret_min); v.fmax[1] = omax(v.fmax[1], q.ep_ret_max);
        v.imin = min(v.imin, q.ep_len_min); v.imax = max(v.imax, q.ep_len_max);
    }
    v = block_combine(v, s_scal);              // its barriers also publish s_slice
    const uint32_t n_fin = v.cnt;

    // 2. the ring: the last min(n_fin, W) finished pairs, entry j of this call at slot (ring_count + j) mod W
    const int64_t rc = *a.ring_count;          // read by every thread; thread 0 stores the new count after the last barrier
    if (n_fin > 0u) {
        const uint32_t start = (n_fin > a.W) ? n_fin - a.W : 0u;
        const uint32_t rc_mod = (uint32_t)(rc % (int64_t)a.W);
        uint32_t running = 0;
        for (uint32_t base = 0; base < nparts; base += (uint32_t)TRACK_BLOCK) {
            const uint32_t p = base + tid;
            const uint32_t cnt = (p < nparts) ? parts[p].ep_count : 0u;
            uint32_t x = cnt;                  // inclusive scan of the chunk's counts
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d, 64);
                if (lane >= (uint32_t)d) x += y;
            }
            if (lane == 63u) s_wtot[w] = x;
            __syncthreads();
            uint32_t woff = 0, chunk = 0;
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) { woff += (u < w) ? s_wtot[u] : 0u; chunk += s_wtot[u]; }
            const uint32_t off = running + woff + (x - cnt);                   // this call's finished episodes before workgroup p
            if (cnt > 0u && off + cnt > start) {
                const uint32_t first = (off < start) ? start - off : 0u;
                for (uint32_t i = first; i < cnt; ++i) {                        // cnt <= 256: inside workgroup p's slots
                    const uint32_t slot = (rc_mod + (off + i)) % a.W;          // distinct for the <= W entries written
                    a.ring_ret[slot] = fin_ret[(uint64_t)p * TRACK_BLOCK + i];
                    a.ring_len[slot] = fin_len[(uint64_t)p * TRACK_BLOCK + i];
                }
            }
            running += chunk;
            __syncthreads();                   // s_wtot is written again; after the last chunk: the ring is complete
        }
    }

    // 3. the ring's valid slots
    const int64_t rc_new = rc + (int64_t)n_fin;
    const uint32_t valid = (rc_new < (int64_t)a.W) ? (uint32_t)rc_new : a.W;
    TrackScal g = scal_identity();
    for (uint32_t s = tid; s < valid; s += (uint32_t)TRACK_BLOCK) {
        const float x = a.ring_ret[s];
        const int32_t l = a.ring_len[s];
        g.dsum = g.dsum + (double)x; g.lsum += l;
        g.fmin[0] = omin(g.fmin[0], x); g.fmax[0] = omax(g.fmax[0], x);
        g.imin = min(g.imin, l); g.imax = max(g.imax, l);
    }
    g = block_combine(g, s_scal);

    // the record: thread j < 3 + K owns f64 column j, thread 0 everything else
    if (tid < nsum) {
        const double t = ((s_slice[0][tid] + s_slice[1][tid]) + (s_slice[2][tid] + s_slice[3][tid])) +
                         ((s_slice[4][tid] + s_slice[5][tid]) + (s_slice[6][tid] + s_slice[7][tid]));
        double* dst = (tid == 0u) ? &rec->inst_sum : (tid == 1u) ? &rec->ep_ret_sum : (tid == 2u) ? &rec->ep_ret_sumsq : &rec->comp_sum[tid - 3u];
        if (nparts > 0u) *dst = *dst + t;
    }
    if (tid == 0u) {
        rec->calls += 1;
        rec->inst_min = omin(rec->inst_min, v.fmin[0]); rec->inst_max = omax(rec->inst_max, v.fmax[0]);
        rec->ep_count += (int64_t)n_fin;
        rec->ep_len_sum += v.lsum;
        rec->ep_ret_min = omin(rec->ep_ret_min, v.fmin[1]); rec->ep_ret_max = omax(rec->ep_ret_max, v.fmax[1]);
        rec->ep_len_min = min(rec->ep_len_min, v.imin); rec->ep_len_max = max(rec->ep_len_max, v.imax);
        if (valid > 0u) {
            rec->win_calls += 1;
            rec->win_ret_mean_sum = rec->win_ret_mean_sum + g.dsum / (double)valid;
            rec->win_len_mean_sum = rec->win_len_mean_sum + (double)g.lsum / (double)valid;
            rec->win_ret_min = omin(rec->win_ret_min, g.fmin[0]); rec->win_ret_max = omax(rec->win_ret_max, g.fmax[0]);
            rec->win_len_min = min(rec->win_len_min, g.imin); rec->win_len_max = max(rec->win_len_max, g.imax);
        }
        *a.ring_count = rc_new;
    }
}

hipError_t launch_track(const TrackArgs& a, hipStream_t s) {
    const uint32_t nparts = track_partials(a.E);
    if (nparts) hipLaunchKernelGGL(track_update_kernel, dim3(nparts), dim3(TRACK_BLOCK), 0, s, a);
    hipLaunchKernelGGL(track_merge_kernel, dim3(1), dim3(TRACK_BLOCK), 0, s, a, nparts);
    return hipGetLastError();
}

}  // namespace rover
