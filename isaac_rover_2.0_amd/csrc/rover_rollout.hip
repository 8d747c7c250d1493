// rover_rollout.hip — the rollout side of PPO on the device: generalised advantage estimation over a stored rollout in one pass,
// its moments, and the normalisation (rover_gae of the C ABI).
//
// The reference does this through skrl (train.py:82 RandomMemory(memory_size=60), cfg/trainSKRL/RoverPPOSKRL.yaml:12-16 rollouts 60,
// discount_factor 0.99, lambda 0.95; skrl's PPO._update calls compute_gae).  skrl is not part of this repository: the semantics below
// are restated from a reading of skrl 0.10 / 1.x, not verified against an installed copy, and are THIS project's definition
// (tests/gae_ref.py restates them independently in float64):
//
//     adv = 0                                                    per env
//     for t = T-1 .. 0:
//         nv   = values[t+1] if t < T-1 else last_values
//         adv  = rewards[t] - values[t] + gamma (dones[t] ? 0 : 1) (nv + lam adv)
//         A[t] = adv
//     returns    = A + values
//     advantages = (A - mean(A)) / (std(A) + 1e-8)               mean and UNBIASED std over all T E elements
//
// NaN and Inf get no special handling (a done flag multiplies by 0, it does not select: 0 * Inf is NaN, as in torch).
//
// Arithmetic (normative; the library is built with -ffp-contract=off, one IEEE rounding per operation), all f32:
//     g = gamma * (done ? 0 : 1)      exact
//     x = lam * adv;  y = nv + x;  z = g * y;  w = rewards[t] - values[t];  adv = w + z;  returns[t] = adv + values[t]
// A column (one env) is evaluated by one thread in this order whatever E, the block shape or the grid: returns[:, e] and the raw
// A[:, e] depend on env e's column alone, so two half-shards reproduce the whole bit for bit.
//
// Layout.  One thread per env, lanes on consecutive envs: every load and store of a wave is one coalesced 256-byte row (64 B for the
// done bytes).  The recurrence is sequential in t, the addresses are not: the kernel loads GAE_U time steps of (reward, value, done)
// per lane at once and keeps the NEXT chunk's loads in flight while it runs the dependent chain of the current one (two register
// chunks, ping-pong; the newest T mod GAE_U steps are a partial chunk whose loads go out together with the first whole chunk's),
// because at 65 536 envs there is about one wave per SIMD and nothing else hides the HBM latency.  values[t+1] is
// the value register of the step before: each input element is read once, and returns may alias values (a thread reads element
// (t, e) before it — and only it — writes it).
//
// Moments, deterministic, no floating-point atomics.  Each thread sums its column in f64 shifted by the column's first A (s1 = sum d,
// s2 = sum d^2 with d = A - A[T-1]: no cancellation against a large common mean), turns that into (count, mean, M2) and merges
// columns, lanes (a fixed shuffle tree) and, in the finishing kernel, the per-block partials (thread i takes partials i, i + 256, ...
// in order, then a fixed tree) with Chan's pairwise formula, whose M2 update adds non-negative terms only.  Every block of the
// finishing kernel repeats that same reduction, so all of them normalise with the same bits.  The partials live in a buffer of
// GAE_MAX_BLOCKS entries that the ctx allocates at rover_create: the call allocates nothing and is capturable; like the chain entry
// points, rover_gae calls of one ctx run on one stream at a time.
//
// Launches: the scan (ROVER_GAE_RAW and ROVER_GAE_NORMALIZE_GIVEN normalise nothing afterwards: one launch); plus the finishing kernel
// when the call's own moments are needed (ROVER_GAE_NORMALIZE, or stats_out given): two launches.
//
// A composition scan over t across lanes for small E (A_t = a_t + c_t A_{t+1} composed pairwise) rounds (a1 + c1 a2) and (c1 c2)
// where the recurrence rounds a2 + c2 A first: it cannot give the recurrence's bits, so by the sharding identity it is not built.
#include "rover_internal.h"

#include <algorithm>

namespace rover {

constexpr int GAE_U = 4;                   // time steps per register chunk (two chunks in flight per lane); measured against 2, 6, 8,
                                           // 16 and 32 at T = 60 (EXPERIMENTS.md section 12): 4 is the fastest, larger chunks cost registers
constexpr int GAE_BLOCK = 64;              // one wave per block: small batches spread over as many CUs as they have waves
constexpr int GAE_FIN_BLOCK = 256;

struct Mom { double n, mean, m2; };        // count, mean, sum of squared deviations

// Chan, Golub & LeVeque's pairwise update; an empty side leaves the other unchanged
__host__ __device__ static inline Mom mom_merge(const Mom& a, const Mom& b) {
    if (a.n == 0.0) return b;
    if (b.n == 0.0) return a;
    const double n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
    return Mom{n, a.mean + d * f, a.m2 + b.m2 + d * d * (a.n * f)};
}

void gae_combine_moments(const double* a, const double* b, double* out) {
    const Mom m = mom_merge(Mom{a[0], a[1], a[2]}, Mom{b[0], b[1], b[2]});
    out[0] = m.n; out[1] = m.mean; out[2] = m.m2;
}

// what the normalisation subtracts and divides by, from (count, mean, M2)
__device__ static inline void gae_norm_of(const Mom& m, float* mean, float* den) {
    *mean = (float)m.mean;
    *den = (float)(sqrt(m.m2 / (m.n - 1.0)) + 1e-8);
}

struct GaeChunk { float r[GAE_U], v[GAE_U]; uint32_t d[GAE_U]; };

// time steps t_hi, t_hi - 1, ... of env e: all GAE_U of them (branch-free, so that the compiler can count the loads still in flight), or
// with HEAD only the first `n` (the same in every lane)
template <bool HEAD>
__device__ __forceinline__ void gae_load(GaeChunk& c, const GaeArgs& a, uint32_t e, int t_hi, int n) {
#pragma unroll
    for (int i = 0; i < GAE_U; ++i) {
        const int t = t_hi - i;
        if (!HEAD || i < n) {
            c.r[i] = a.rewards[(int64_t)t * a.rewards_stride + e];
            c.v[i] = a.values[(int64_t)t * a.values_stride + e];
            c.d[i] = a.dones[(int64_t)t * a.dones_stride + e];
        }
    }
}

struct GaeCarry { float adv, nv, mean, den; double ref, s1, s2; };

template <bool STATS, bool GIVEN, bool HEAD>
__device__ __forceinline__ void gae_steps(const GaeChunk& c, const GaeArgs& a, uint32_t e, int t_hi, int n, GaeCarry& k) {
#pragma unroll
    for (int i = 0; i < GAE_U; ++i) {
        const int t = t_hi - i;
        if (!HEAD || i < n) {
            const float g = a.gamma * (c.d[i] ? 0.0f : 1.0f);
            const float x = a.lam * k.adv;
            const float y = k.nv + x;
            const float z = g * y;
            const float w = c.r[i] - c.v[i];
            k.adv = w + z;
            k.nv = c.v[i];
            a.returns[(int64_t)t * a.returns_stride + e] = k.adv + c.v[i];
            a.advantages[(int64_t)t * a.advantages_stride + e] = GIVEN ? (k.adv - k.mean) / k.den : k.adv;
            if (STATS) {
                if (t == a.T - 1) k.ref = (double)k.adv;
                const double d = (double)k.adv - k.ref;
                k.s1 += d;
                k.s2 += d * d;
            }
        }
    }
}

// STATS: leave this block's (count, mean, M2) of the raw A in partials[blockIdx.x]; GIVEN: write (A - mean) / den of stats_in
template <bool STATS, bool GIVEN>
__global__ __launch_bounds__(GAE_BLOCK) void gae_scan_kernel(GaeArgs a) {
    GaeCarry k{};
    if (GIVEN) gae_norm_of(Mom{a.stats_in[0], a.stats_in[1], a.stats_in[2]}, &k.mean, &k.den);
    Mom acc{0.0, 0.0, 0.0};
    const uint32_t tiles = (a.E + GAE_BLOCK - 1) / GAE_BLOCK;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t e = tile * GAE_BLOCK + threadIdx.x;
        if (e >= a.E) continue;
        k.adv = 0.0f;
        k.nv = a.last_values[e];
        k.ref = k.s1 = k.s2 = 0.0;
        GaeChunk c0, c1;
        int t_hi = a.T - 1;
        const int head = a.T % GAE_U;                          // the newest T mod GAE_U steps first: whole chunks remain
        if (head) {                                            // their loads and the first whole chunk's go out together
            gae_load<true>(c1, a, e, t_hi, head);
            if (t_hi - head >= 0) gae_load<false>(c0, a, e, t_hi - head, 0);
            gae_steps<STATS, GIVEN, true>(c1, a, e, t_hi, head, k);
            t_hi -= head;
        } else {
            gae_load<false>(c0, a, e, t_hi, 0);
        }
        while (t_hi >= 0) {                                    // the tests are the same in every lane
            if (t_hi - GAE_U >= 0) gae_load<false>(c1, a, e, t_hi - GAE_U, 0);
            gae_steps<STATS, GIVEN, false>(c0, a, e, t_hi, 0, k);
            if ((t_hi -= GAE_U) < 0) break;
            if (t_hi - GAE_U >= 0) gae_load<false>(c0, a, e, t_hi - GAE_U, 0);
            gae_steps<STATS, GIVEN, false>(c1, a, e, t_hi, 0, k);
            t_hi -= GAE_U;
        }
        if (STATS) {
            const double n = (double)a.T, q = k.s1 / n;
            const double m2 = k.s2 - k.s1 * q;                 // >= 0 up to rounding; a NaN stays a NaN
            acc = mom_merge(acc, Mom{n, k.ref + q, m2 < 0.0 ? 0.0 : m2});
        }
    }
    if (STATS) {
#pragma unroll
        for (int off = GAE_BLOCK / 2; off > 0; off >>= 1) {
            const Mom o{__shfl_down(acc.n, off, GAE_BLOCK), __shfl_down(acc.mean, off, GAE_BLOCK), __shfl_down(acc.m2, off, GAE_BLOCK)};
            acc = mom_merge(acc, o);
        }
        if (threadIdx.x == 0) {
            double* p = a.partials + 3 * (size_t)blockIdx.x;
            p[0] = acc.n; p[1] = acc.mean; p[2] = acc.m2;
        }
    }
}

// Merges the n_parts partials in a fixed order (the same in every block), writes stats_out, and with NORM rewrites the raw A in
// `advantages` as (A - mean) / (std + 1e-8).
template <bool NORM>
__global__ __launch_bounds__(GAE_FIN_BLOCK) void gae_finish_kernel(GaeArgs a, uint32_t n_parts, FastDiv e_div) {
    __shared__ double sh[3][GAE_FIN_BLOCK];
    const uint32_t i = threadIdx.x;
    Mom acc{0.0, 0.0, 0.0};
    for (uint32_t p = i; p < n_parts; p += GAE_FIN_BLOCK)
        acc = mom_merge(acc, Mom{a.partials[3 * (size_t)p], a.partials[3 * (size_t)p + 1], a.partials[3 * (size_t)p + 2]});
    sh[0][i] = acc.n; sh[1][i] = acc.mean; sh[2][i] = acc.m2;
    __syncthreads();
    for (uint32_t s = GAE_FIN_BLOCK / 2; s > 0; s >>= 1) {
        if (i < s) {
            const Mom m = mom_merge(Mom{sh[0][i], sh[1][i], sh[2][i]}, Mom{sh[0][i + s], sh[1][i + s], sh[2][i + s]});
            sh[0][i] = m.n; sh[1][i] = m.mean; sh[2][i] = m.m2;
        }
        __syncthreads();
    }
    const Mom m{sh[0][0], sh[1][0], sh[2][0]};
    if (a.stats_out && blockIdx.x == 0 && i == 0) { a.stats_out[0] = m.n; a.stats_out[1] = m.mean; a.stats_out[2] = m.m2; }
    if (NORM) {
        float mean, den;
        gae_norm_of(m, &mean, &den);
        const uint32_t total = (uint32_t)a.T * a.E;                        // < 2^31
        for (uint32_t idx = blockIdx.x * GAE_FIN_BLOCK + i; idx < total; idx += gridDim.x * GAE_FIN_BLOCK) {
            const uint32_t t = e_div.div(idx), e = idx - t * a.E;
            float* p = a.advantages + (int64_t)t * a.advantages_stride + e;
            *p = (*p - mean) / den;
        }
    }
}

int gae_launches(const GaeArgs& a) { return a.E == 0 ? 0 : (a.normalize == GAE_NORMALIZE || a.stats_out) ? 2 : 1; }

hipError_t launch_gae(const GaeArgs& a, hipStream_t s) {
    if (a.E == 0) return hipSuccess;
    const bool finish = gae_launches(a) == 2, given = a.normalize == GAE_NORMALIZE_GIVEN;
    const uint32_t grid = std::min<uint32_t>(blocks_for(a.E, GAE_BLOCK), GAE_MAX_BLOCKS);
    if (finish && given) gae_scan_kernel<true, true><<<grid, GAE_BLOCK, 0, s>>>(a);
    else if (finish) gae_scan_kernel<true, false><<<grid, GAE_BLOCK, 0, s>>>(a);
    else if (given) gae_scan_kernel<false, true><<<grid, GAE_BLOCK, 0, s>>>(a);
    else gae_scan_kernel<false, false><<<grid, GAE_BLOCK, 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !finish) return e;
    if (a.normalize == GAE_NORMALIZE) {
        const uint32_t fin = std::min<uint32_t>(blocks_for((uint64_t)a.T * a.E, 4 * GAE_FIN_BLOCK), 1024);
        gae_finish_kernel<true><<<fin, GAE_FIN_BLOCK, 0, s>>>(a, grid, make_fastdiv(a.E));
    } else {
        gae_finish_kernel<false><<<1, GAE_FIN_BLOCK, 0, s>>>(a, grid, make_fastdiv(a.E));
    }
    return hipGetLastError();
}

}  // namespace rover
