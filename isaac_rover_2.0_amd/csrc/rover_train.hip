// rover_train.hip — the learner side of PPO on the device: the backward of one Layer (rover_linear_backward) and the PPO minibatch
// loss at the nets' outputs with its gradients (rover_ppo_loss).
//
// The reference trains through skrl's PPO._update on torch autograd (train.py:82-124, cfg/trainSKRL/RoverPPOSKRL.yaml); the nets here
// hold plain tensors and run on the kernels of rover_mlp.hip, so the backward is written out.  The semantics are restated from a
// reading of skrl 1.x (skrl is not installed) and of ATen's backward formulas, and are THIS project's definition (include/rover_step.h;
// tests/ppo_ref.py restates them independently in float64).
//
// ---- the backward of y = act(x W^T + b) ------------------------------------------------------------------------------------------
// dz = dy act'(y) with the derivative taken from the stored output y alone; dW = dz^T x, db = column sums of dz, dx = dz W.
//
// Weight gradient (the hot path: a reduction over M = 65 536 rows for 80 x 1 112 outputs), f32-input MFMA like the forward
// (v_mfma_f32_32x32x2_f32: exact f32 products, one rounding per accumulate).  The MFMA's reduction index is the batch row m:
//     A[i = n][kk = m] = dz[m][n]        B[kk = m][j = k] = x[m][k]        D[n][k] += A B
// and both operands have the LANE on the contiguous index of their tensor (lane & 31 = n resp. k, lane >> 5 = one of two rows): a
// slab of 32 rows is staged through LDS exactly as it lies in memory — no transpose, no padding (ds_read_b32 / ds_write_b32 bank on
// the address mod 32 per 32-lane half: 32 consecutive words never conflict).  dz is formed in registers while dy and y are fetched
// (dy act'(y), 0 past M / N); no dz tensor exists in HBM.  A workgroup = NW waves: they share the dz slab [32][NT x 32] and take one
// 32-column tile of x each, NT accumulator tiles per wave (<= 48 VGPRs), the next slab's loads in flight under the MFMAs (the
// slab loop of the f32 tile core, rover_f32_tile.h, with both slabs k-major).  grid = (K tiles / NW, N tiles / NT, S): M is cut into
// S splits of whole slabs.
//   * M >= 8 192: NW = 4, NT <= 3 (N = 80: all of dz in one workgroup, x read once), S = M / 1 024 rounded down to a power of two,
//     at most 64 — 80 x 1 112 at 65 536 rows: 9 x 1 x 64 = 576 workgroups of 4 waves on 256 CUs;
//   * below: NW = NT = 1 (one wave per 32 x 32 tile) and S = 1 / 2 / 4 / 8 from 0 / 128 / 256 / 512 rows: at 512 rows the same layer is
//     35 x 3 x 8 = 840 waves — the card is filled by tiling over (N, K), not over M.
// Determinism: split s writes its f32 partial tile to scratch[s][N][K] (and its db partial to [s][N]) with plain stores; a merge
// kernel adds the S partials of an element in the order s = 0 .. S - 1.  No floating-point atomics anywhere: the same inputs give
// the same bits on every run.  S = 1 writes dW and db directly (no merge).  db rides along: the workgroups of K tile 0 sum the
// columns of each staged dz slab (row order) — K = 0 still has that one K tile, so db is written and dW is empty.
// The scratch is the ctx's, grown on demand outside a stream capture (the chain kernels' rule).
//
// dx = dz W is a GEMM of the forward's shape with dz as the left operand, on the same core: the left slab is k-minor like the
// forward's (32 rows x 32 k at the 33-word pitch) with dz formed by its staging functor, and W is a k-major slab, read as it lies
// ([n][k], lane on k: B[kk = n][j = k]) instead of transposed.  Its route is the forward's own for an M x K output
// (linear_route(M, K)).
//
// ---- the PPO loss ----------------------------------------------------------------------------------------------------------------
// One thread per row evaluates the row's terms in f32 in the order written above ppo_loss_kernel; the sums over M (policy, value, kl and the A
// log-std sums) are f64: a fixed shuffle tree per wave, the waves of a block in order, per-block partials in a ctx buffer, and a
// one-block finishing kernel that adds them as rover_gae's does (thread i takes partials i, i + 256, ... then a fixed tree).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include "rover_internal.h"
#include "rover_f32_tile.h"

namespace rover {

// act'(v) from the stored output y = act(v)
__device__ __forceinline__ float act_grad_from_y(float y, int act) {
    switch (act) {
        case 1: return y > 0.0f ? 1.0f : 0.01f;
        case 2: return 1.0f - y * y;
        case 3: return y > 0.0f ? 1.0f : 0.0f;
        case 4: return y > 0.0f ? 1.0f : y + 1.0f;
        default: return 1.0f;
    }
}
__device__ __forceinline__ float dz_at(const LinearBwdArgs& a, uint32_t row, uint32_t col) {
    const float dy = a.dy[(size_t)row * a.dy_stride + col];
    return a.act == 0 ? dy : dy * act_grad_from_y(a.y[(size_t)row * a.y_stride + col], a.act);
}

// ---- dW / db: on the f32 tile core (rover_f32_tile.h), both operands k-major (the reduction index is the batch row) ----------------
template <int NT, int NW>
__global__ void __launch_bounds__(64 * NW) linear_wgrad_kernel(LinearBwdArgs a, int K, int rows_per_split, float* __restrict__ wpart,
                                                                float* __restrict__ bpart) {
    static_assert(NT * 32 <= 64 * NW, "one thread per dz column sums db");
    using DSlab = F32KMajor<NW, 32 * NT>;
    using XSlab = F32KMajor<NW, 32 * NW>;
    constexpr uint32_t DP = NT * 32u, XP = NW * 32u;
    __shared__ float Dz[DSlab::WORDS];
    __shared__ float Xs[XSlab::WORDS];
    const DSlab ds{Dz};
    const XSlab xs{Xs};
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k0 = blockIdx.x * XP, n0 = blockIdx.y * DP, split = blockIdx.z;
    const uint32_t m_lo = split * (uint32_t)rows_per_split, m_hi = min((uint32_t)a.M, m_lo + (uint32_t)rows_per_split);
    f32x16 acc[NT];
    f32_zero(acc);
    float pd[DSlab::NP], px[XSlab::NP];
    auto fetch = [&](uint32_t m0) {
        DSlab::stage(pd, [&](uint32_t r, uint32_t c) {
            const uint32_t row = m0 + r, col = n0 + c;
            return (row < m_hi && col < (uint32_t)a.N) ? dz_at(a, row, col) : 0.0f;
        });
        XSlab::stage(px, [&](uint32_t r, uint32_t c) {
            const uint32_t row = m0 + r, col = k0 + c;
            return (row < m_hi && col < (uint32_t)K) ? a.x[(size_t)row * a.x_stride + col] : 0.0f;
        });
    };
    const bool sum_db = bpart != nullptr && blockIdx.x == 0 && tid < DP;
    float dbs = 0.0f;
    f32_slabs(m_lo, m_hi, fetch, [&](uint32_t) { ds.stash(pd); xs.stash(px); },
              [&] {
                  if (sum_db)
                      for (uint32_t r = 0; r < 32u; ++r) dbs += Dz[r * DP + tid];      // rows past the split are zeros
              },
              [&](uint32_t kk) {
                  const float bv = xs.operand(wave, kk);
#pragma unroll
                  for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds.operand(t, kk), bv, acc[t], 0, 0, 0);
              });
    if (sum_db && n0 + tid < (uint32_t)a.N) bpart[(size_t)split * a.N + n0 + tid] = dbs;
    const uint32_t col = k0 + wave * 32u + f32_cd(lane, 0).col;      // the tile's column is k, its row n
    if (col >= (uint32_t)K) return;
    float* __restrict__ o = wpart + (size_t)split * a.N * K;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t n = n0 + 32u * t + f32_cd(lane, r).row;
            if (n < (uint32_t)a.N) o[(size_t)n * K + col] = acc[t][r];
        }
}

// element i of dW (i < N K) or of db (i - N K): its S partials added in the order s = 0 .. S - 1
__global__ void __launch_bounds__(256) wgrad_merge_kernel(const float* __restrict__ wpart, const float* __restrict__ bpart, int S, uint32_t nk,
                                                          uint32_t n, float* __restrict__ dw, float* __restrict__ db) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nk) {
        float v = 0.0f;
        for (int s = 0; s < S; ++s) v += wpart[(size_t)s * nk + i];
        dw[i] = v;
    } else if (i - nk < n && db) {
        float v = 0.0f;
        for (int s = 0; s < S; ++s) v += bpart[(size_t)s * n + (i - nk)];
        db[i - nk] = v;
    }
}

// ---- dx: on the f32 tile core, dz formed while staged as the k-minor left operand and W read as it lies (k-major) ---------------------
template <int NT, int NW>
__global__ void __launch_bounds__(64 * NW) linear_dgrad_kernel(LinearBwdArgs a) {
    using ASlab = F32KMinor<NW, 32 * NW>;
    using WSlab = F32KMajor<NW, 32 * NT>;
    __shared__ float As[ASlab::WORDS];                                // dz[m][n slab]
    __shared__ float Ws[WSlab::WORDS];                                // W[n slab][k tile columns]
    const ASlab as{As};
    const WSlab ws{Ws};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t row0 = blockIdx.x * (32u * NW), c0 = blockIdx.y * (NT * 32u);
    f32x16 acc[NT];
    f32_zero(acc);
    float pa[ASlab::NP], pw[WSlab::NP];
    auto fetch = [&](uint32_t n0) {
        ASlab::stage(pa, [&](uint32_t r, uint32_t c) {
            const uint32_t gr = row0 + r, gn = n0 + c;
            return (gn < (uint32_t)a.N && gr < (uint32_t)a.M) ? dz_at(a, gr, gn) : 0.0f;
        });
        WSlab::stage(pw, [&](uint32_t r, uint32_t c) {
            const uint32_t n = n0 + r, col = c0 + c;
            return (n < (uint32_t)a.N && col < (uint32_t)a.K) ? a.w[(size_t)n * a.K + col] : 0.0f;
        });
    };
    f32_slabs(0u, (uint32_t)a.N, fetch, [&](uint32_t) { as.stash(pa); ws.stash(pw); }, [] {}, [&](uint32_t kk) {
        const float av = as.operand(wave, kk);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ws.operand(t, kk), acc[t], 0, 0, 0);
    });
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const uint32_t col = c0 + 32u * t + f32_cd(lane, 0).col;
        if (col >= (uint32_t)a.K) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row = row0 + wave * 32u + f32_cd(lane, r).row;
            if (row < (uint32_t)a.M) a.dx[(size_t)row * a.dx_stride + col] = acc[t][r];
        }
    }
}

// ---- the one place that decides what a backward launches ---------------------------------------------------------------------------
LinearBwdRoute linear_backward_route(int M, int K, int N, bool want_dx) {
    LinearBwdRoute r{};
    if (M < 0 || K < 0 || N <= 0 || N > 256 || (want_dx && K > 256)) return r;
    const int nt_all = (N + 31) / 32;
    int S;
    if (M >= 8192) {
        const int groups = (nt_all + 2) / 3;
        r.nw = 4; r.nt = (nt_all + groups - 1) / groups;
        S = 8;
        while (S < 64 && 2 * S * 1024 <= M) S *= 2;
    } else {
        r.nw = 1; r.nt = 1;
        S = M >= 512 ? 8 : M >= 256 ? 4 : M >= 128 ? 2 : 1;
    }
    r.splits = S;
    r.rows_per_split = (int)((((int64_t)M + S - 1) / S + 31) / 32 * 32);      // whole slabs; trailing splits may be empty (they write zeros)
    if (want_dx && K > 0) r.dx = linear_route(M, K);
    r.ok = true;
    return r;
}
size_t linear_backward_scratch_floats(const LinearBwdRoute& r, int K, int N) {
    return r.splits > 1 ? (size_t)r.splits * ((size_t)N * K + (size_t)N) : 0;
}
const char* linear_backward_route_name(const LinearBwdRoute& r) {
    if (!r.ok) return nullptr;
    static thread_local char buf[64];
    if (r.dx.nw) snprintf(buf, sizeof buf, "wgrad<%d,%d>/%d;dgrad<%d,%d>%s", r.nt, r.nw, r.splits, r.dx.nt, r.dx.nw, r.dx.ny == 2 && r.dx.nw == 4 ? "x2" : "");
    else snprintf(buf, sizeof buf, "wgrad<%d,%d>/%d", r.nt, r.nw, r.splits);
    return buf;
}

template <int NT, int NW>
static void launch_wgrad(const LinearBwdArgs& a, int K, const LinearBwdRoute& r, float* wpart, float* bpart, hipStream_t s) {
    const dim3 grid((uint32_t)std::max(1, (K + 32 * NW - 1) / (32 * NW)), (uint32_t)((a.N + 32 * NT - 1) / (32 * NT)), (uint32_t)r.splits);
    hipLaunchKernelGGL((linear_wgrad_kernel<NT, NW>), grid, dim3(64 * NW), 0, s, a, K, r.rows_per_split, wpart, bpart);
}
// scratch: linear_backward_scratch_floats() floats (unused with one split)
hipError_t launch_linear_backward(const LinearBwdArgs& a, const LinearBwdRoute& r, float* scratch, hipStream_t s) {
    if (!r.ok) return hipErrorInvalidValue;
    const size_t nk = (size_t)a.N * a.K;
    if (a.M == 0) {                                                   // no rows: the sums are zero, dx is empty
        hipError_t e = hipSuccess;
        if (a.dw && nk) e = hipMemsetAsync(a.dw, 0, nk * sizeof(float), s);
        if (e == hipSuccess && a.db) e = hipMemsetAsync(a.db, 0, (size_t)a.N * sizeof(float), s);
        return e;
    }
    if (a.dw || a.db) {
        const int K = a.dw ? a.K : 0;                                 // db alone: the one K tile that carries it
        const bool merge = r.splits > 1;
        float* wpart = merge ? scratch : a.dw;
        float* bpart = a.db ? (merge ? scratch + (size_t)r.splits * a.N * K : a.db) : nullptr;
        if (r.nw == 4) {
            switch (r.nt) {
                case 1: launch_wgrad<1, 4>(a, K, r, wpart, bpart, s); break;
                case 2: launch_wgrad<2, 4>(a, K, r, wpart, bpart, s); break;
                case 3: launch_wgrad<3, 4>(a, K, r, wpart, bpart, s); break;
                default: return hipErrorInvalidValue;
            }
        } else if (r.nw == 1 && r.nt == 1) {
            launch_wgrad<1, 1>(a, K, r, wpart, bpart, s);
        } else {
            return hipErrorInvalidValue;
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (merge) {
            const uint32_t wk = (uint32_t)((size_t)a.N * K);
            hipLaunchKernelGGL(wgrad_merge_kernel, dim3(blocks_for((uint64_t)wk + a.N, 256u)), dim3(256), 0, s, wpart, bpart, r.splits, wk, (uint32_t)a.N,
                               a.dw, a.db);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    return a.dx && a.K > 0 ? launch_linear_dgrad(a, r.dx, s) : hipSuccess;
}

// ---- dx alone, any width (rover_linear_dgrad) ----------------------------------------------------------------------------------------
// The same kernel on a route of its own: linear_dgrad_kernel already tiles K over blockIdx.y and walks N in slabs, so neither width has
// a limit but the grid's (65 535 column tiles).  One wave per 32 x 32 tile of dx below 65 536 rows (the forward's switch point); from
// there 128-row workgroups that hold two column tiles (one when K <= 32), which halves the re-reads of the dz slab.  Reasoned, not measured.
LinearRoute linear_dgrad_route(int M, int N, int K) {
    if (M < 0 || N < 1 || K < 1) return LinearRoute{0, 0, 0};
    const int64_t kt = ((int64_t)K + 31) / 32;
    LinearRoute r = M >= 128 * 512 ? LinearRoute{4, K > 32 ? 2 : 1, 0} : LinearRoute{1, 1, 0};
    const int64_t ny = (kt + r.nt - 1) / r.nt;
    if (ny > 65535) return LinearRoute{0, 0, 0};
    r.ny = (int)ny;
    return r;
}
const char* linear_dgrad_route_name(const LinearRoute& r) {
    if (!r.nw) return nullptr;
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "dgrad<%d,%d>x%d", r.nt, r.nw, r.ny);
    return buf;
}
hipError_t launch_linear_dgrad(const LinearBwdArgs& a, const LinearRoute& r, hipStream_t s) {
    if (a.M == 0) return hipSuccess;
    return launch_linear_route(a.M, r, [&](auto nt, auto nw, dim3 grid) {
        hipLaunchKernelGGL((linear_dgrad_kernel<decltype(nt)::value, decltype(nw)::value>), grid, dim3(64 * decltype(nw)::value), 0, s, a);
    });
}

// ---- the PPO loss ------------------------------------------------------------------------------------------------------------------
constexpr int PPO_BLOCK = 256;
constexpr int PPO_NSUM = 3 + GAUSS_MAX_A;                            // surrogate, squared value error, kl, then the A log-std sums

__device__ __forceinline__ float ppo_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }     // a NaN stays a NaN

// Arithmetic of one row (normative; -ffp-contract=off), all f32, j = 0 .. A - 1 in order:
//     ls' = clamp(ls_j) (if clip_log_std); sigma = expf(ls'); d = a_ij - mean_ij; z = d / sigma; lp_j = (-0.5 (z z) - ls') - 0.5 log 2pi
//     lp = lp_0 + lp_1 + ...;  q = lp - old_log_prob;  r = expf(q);  kl term (r - 1) - q
//     s = min(adv r, adv clamp(r, 1 - c, 1 + c));  g = -(adv / M) [1 - c <= r <= 1 + c or adv r < adv clamp(r)];  t = g r
//     d_mean_ij = (t z) / sigma;  log-std term t (z z - 1)
//     v' = old + clamp(value - old, -vc, vc) (if clip_predicted_values);  e = v' - returns;  value term e e
//     d_value = (vls (2 / M)) e [|value - old| <= vc, or no clipping]
__global__ void __launch_bounds__(PPO_BLOCK) ppo_loss_kernel(PpoArgs a) {
    double sums[PPO_NSUM];
#pragma unroll
    for (int c = 0; c < PPO_NSUM; ++c) sums[c] = 0.0;
    const float fm = (float)a.M;
    const float lo = 1.0f - a.ratio_clip, hi = 1.0f + a.ratio_clip;
    const float vscale = a.value_loss_scale * (2.0f / fm);
    for (uint32_t row = blockIdx.x * PPO_BLOCK + threadIdx.x; row < (uint32_t)a.M; row += gridDim.x * PPO_BLOCK) {
        float z[GAUSS_MAX_A], sg[GAUSS_MAX_A];
        float lp = 0.0f;
#pragma unroll
        for (int j = 0; j < GAUSS_MAX_A; ++j) {
            z[j] = 0.0f; sg[j] = 1.0f;
            if (j >= a.A) continue;
            float ls = a.log_std[j];
            if (a.clip_log_std) ls = ppo_clamp(ls, a.min_log_std, a.max_log_std);
            sg[j] = expf(ls);
            const float d = a.actions[(size_t)row * a.actions_stride + j] - a.mean[(size_t)row * a.mean_stride + j];
            z[j] = d / sg[j];
            const float l = (-0.5f * (z[j] * z[j]) - ls) - 0.91893853320467274f;
            lp = j == 0 ? l : lp + l;
        }
        const float q = lp - a.old_log_prob[row];
        const float r = expf(q);
        const float adv = a.advantages[row];
        const float rc = ppo_clamp(r, lo, hi);
        const float s1 = adv * r, s2 = adv * rc;
        const float surr = (s1 < s2 || s1 != s1) ? s1 : s2;          // torch.min: a NaN on either side comes out
        const bool pass = (lo <= r && r <= hi) || s1 < s2;
        const float g = -(adv / fm) * (pass ? 1.0f : 0.0f);
        const float t = g * r;
        sums[0] += (double)surr;
        sums[2] += (double)((r - 1.0f) - q);
#pragma unroll
        for (int j = 0; j < GAUSS_MAX_A; ++j) {
            if (j >= a.A) continue;
            a.d_mean[(size_t)row * a.d_mean_stride + j] = (t * z[j]) / sg[j];
            sums[3 + j] += (double)(t * (z[j] * z[j] - 1.0f));
        }
        const float val = a.value[row], old = a.old_values[row];
        const float dv = val - old;
        const float vp = a.clip_predicted_values ? old + ppo_clamp(dv, -a.value_clip, a.value_clip) : val;
        const float e = vp - a.returns[row];
        sums[1] += (double)(e * e);
        const bool vpass = !a.clip_predicted_values || (-a.value_clip <= dv && dv <= a.value_clip);
        a.d_value[row] = (vscale * e) * (vpass ? 1.0f : 0.0f);
    }
    __shared__ double sh[PPO_BLOCK / 64][PPO_NSUM];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < PPO_NSUM; ++c) {
        double v = sums[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) sh[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < PPO_NSUM) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < PPO_BLOCK / 64; ++w) v += sh[w][threadIdx.x];
        a.partials[(size_t)blockIdx.x * PPO_NSUM + threadIdx.x] = v;
    }
}

// one block: component c's n_parts partials (thread i takes i, i + 256, ... in order, then a fixed tree) -> stats and d_log_std
__global__ void __launch_bounds__(PPO_BLOCK) ppo_finish_kernel(PpoArgs a, uint32_t n_parts) {
    __shared__ double sh[PPO_BLOCK];
    __shared__ double tot[PPO_NSUM];
    const uint32_t i = threadIdx.x;
    for (int c = 0; c < 3 + a.A; ++c) {
        double v = 0.0;
        for (uint32_t p = i; p < n_parts; p += PPO_BLOCK) v += a.partials[(size_t)p * PPO_NSUM + c];
        sh[i] = v;
        __syncthreads();
        for (uint32_t s = PPO_BLOCK / 2; s > 0; s >>= 1) {
            if (i < s) sh[i] += sh[i + s];
            __syncthreads();
        }
        if (i == 0) tot[c] = sh[0];
        __syncthreads();
    }
    const double m = (double)a.M;
    if (i < (uint32_t)a.A) {
        const float ls = a.log_std[i];
        const bool pass = !a.clip_log_std || (a.min_log_std <= ls && ls <= a.max_log_std);
        a.d_log_std[i] = pass ? (float)(tot[3 + i] - (double)a.entropy_loss_scale / (double)a.A) : 0.0f;
    }
    if (i == 0) {
        double ent = 0.0;
        for (int j = 0; j < a.A; ++j) {
            float ls = a.log_std[j];
            if (a.clip_log_std) ls = ppo_clamp(ls, a.min_log_std, a.max_log_std);
            ent += (double)ls;
        }
        a.stats[0] = -tot[0] / m;
        a.stats[1] = (double)a.value_loss_scale * (tot[1] / m);
        a.stats[2] = -(double)a.entropy_loss_scale * (0.5 + 0.91893853320467274 + ent / (double)a.A);
        a.stats[3] = tot[2] / m;
    }
}

hipError_t launch_ppo_loss(const PpoArgs& a, hipStream_t s) {
    if (a.M == 0) return hipSuccess;
    const uint32_t grid = std::min<uint32_t>(blocks_for((uint64_t)a.M, PPO_BLOCK), PPO_MAX_BLOCKS);
    hipLaunchKernelGGL(ppo_loss_kernel, dim3(grid), dim3(PPO_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ppo_finish_kernel, dim3(1), dim3(PPO_BLOCK), 0, s, a, grid);
    return hipGetLastError();
}

}  // namespace rover
