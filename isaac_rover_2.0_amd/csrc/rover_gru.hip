// rover_gru.hip — the student policy's recurrent block: one GRU layer for one time step in ONE launch, and the sigmoid gate that
// follows it.
//
// Reference: omniisaacgymenvs/tasks/utils/learning_by_cheating/student_model.py — Belief_Encoder (:42-92): nn.GRU(124 -> 300, 2 layers)
// whose output feeds two Layer chains gb / ga, belief = gb(out) + l_e * sigmoid(ga(out)); Belief_Decoder (:94-131):
// estimated = decoded + e * sigmoid(gate).  student_loader.act (:21-24) runs one time step per env step with a carried hidden state.
//
// gru_cell_kernel stands on the f32 tile core (rover_f32_tile.h: staging map, slab loop, operand reads, C/D coordinates — shared with
// linear_act, linear_wgrad and linear_dgrad): a 32-row k-minor slab of the left operand per wave, the weights k-minor as they lie
// ([3H][K] and [3H][H], lane on k), exact f32 MFMA (v_mfma_f32_32x32x2_f32).  The left operand is x followed by h along the reduction.  A workgroup owns 32 NW rows and ONE 32-column
// tile j of the hidden state, for which it needs weight rows j (r), H + j (z) and 2H + j (n) of both matrices; it keeps FOUR accumulator
// tiles — r and z summed over K + H, gi_n over K, gh_n over H (64 accumulator registers) — and the gate arithmetic runs on them in
// the epilogue, so neither [M, 3H] pre-activation tensor exists in memory.
//
// The arithmetic of the epilogue is written out below operation by operation and compiled with -ffp-contract=off (build.sh): one
// IEEE rounding per operation, in this order, on every instantiation.  No atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"
#include "rover_act.h"
#include "rover_f32_tile.h"

namespace rover {

// (gru_sigmoid is rover_act.h's)

// bit j: the row of this thread's staged register j (F32KMinor's map) keeps its h_in: it is in range and reset_mask does not mark it
template <int NW>
__device__ __forceinline__ uint32_t gru_live_rows(uint32_t row0, uint32_t M, const uint8_t* __restrict__ reset_mask) {
    uint32_t live = 0u;
    F32KMinor<NW, 32 * NW>::each([&](int j, uint32_t r, uint32_t) {
        if (row0 + r < M && !(reset_mask && reset_mask[row0 + r])) live |= 1u << j;
    });
    return live;
}

// TRAIN: the epilogue also stores r | z | n | q (q = s_hn + b_hn) to a.gates for the backward; h' is computed by the same operations.
template <int NW, bool TRAIN = false>
__global__ void __launch_bounds__(64 * NW, NW == 1 ? 1 : 2) gru_cell_kernel(GruArgs a) {
    using XSlab = F32KMinor<NW, 32 * NW>;
    using WSlab = F32KMinor<NW, 3 * 32>;
    __shared__ float As[XSlab::WORDS];                               // the left operand's k-slab: x, then h
    __shared__ float Ws[WSlab::WORDS];                               // weight rows j, H + j, 2H + j of the same k-slab: tile g = gate g
    const XSlab xs{As};
    const WSlab ws{Ws};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t row0 = blockIdx.x * (32u * NW), n0 = blockIdx.y * 32u;    // blockIdx.y: the 32-column tile of the hidden state
    const uint32_t H = (uint32_t)a.H, M = (uint32_t)a.M;
    f32x16 acc[4];                                                   // r, z, i_n, h_n
    f32_zero(acc);
    float pa[XSlab::NP], pw[WSlab::NP];
    // rows of h_in that reset_mask marks are read as zeros (here, in the products, and in the epilogue's z * h)
    const uint32_t live = gru_live_rows<NW>(row0, M, a.reset_mask);
    // the reduction: the slabs of x (zero past K) at offsets 0 .. ox, then those of h (zero past H, and on reset rows) up to `end` — the
    // left operand's columns and the same columns of the three gates' weight rows
    const uint32_t ox = ((uint32_t)a.K + 31u) / 32u * 32u, end = ox + (H + 31u) / 32u * 32u;
    auto fetch = [&](uint32_t o) {
        const bool phase_h = o >= ox;
        const uint32_t Kp = phase_h ? H : (uint32_t)a.K, k0 = phase_h ? o - ox : o;
        const float* __restrict__ w = phase_h ? a.w_hh : a.w_ih;
        const float* __restrict__ src = phase_h ? a.h_in : a.x;
        const int64_t src_stride = phase_h ? a.h_in_stride : a.x_stride;
        XSlab::each([&](int j, uint32_t r, uint32_t c) {
            const uint32_t gr = row0 + r, gk = k0 + c;
            const bool ok = gk < Kp && gr < M && (!phase_h || ((live >> j) & 1u));
            pa[j] = ok ? src[(size_t)gr * src_stride + gk] : 0.0f;
        });
        WSlab::stage(pw, [&](uint32_t r, uint32_t c) {               // slab row r: column n0 + r % 32 of the hidden state, gate r / 32
            const uint32_t n = n0 + (r & 31u), gk = k0 + c;
            return (gk < Kp && n < H) ? w[((size_t)(r >> 5) * H + n) * Kp + gk] : 0.0f;
        });
    };
    auto stash = [&](uint32_t) { xs.stash(pa); ws.stash(pw); };
    auto step = [&](uint32_t kk, f32x16& acc_n) {
        const float av = xs.operand(wave, kk);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ws.operand(0, kk), acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ws.operand(1, kk), acc[1], 0, 0, 0);
        acc_n = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ws.operand(2, kk), acc_n, 0, 0, 0);
    };
    f32_slabs(0u, end, fetch, stash, [] {}, [&](uint32_t kk) { step(kk, acc[2]); }, ox, [&](uint32_t kk) { step(kk, acc[3]); });
    const uint32_t col = n0 + f32_cd(lane, 0).col;
    if (col >= H) return;
    const float b_ir = a.b_ih ? a.b_ih[col] : 0.0f, b_iz = a.b_ih ? a.b_ih[H + col] : 0.0f, b_in = a.b_ih ? a.b_ih[2u * H + col] : 0.0f;
    const float b_hr = a.b_hh ? a.b_hh[col] : 0.0f, b_hz = a.b_hh ? a.b_hh[H + col] : 0.0f, b_hn = a.b_hh ? a.b_hh[2u * H + col] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t row = row0 + wave * 32u + f32_cd(lane, r).row;
        if (row >= M) continue;
        const bool reset = a.reset_mask && a.reset_mask[row];
        const float h = reset ? 0.0f : a.h_in[(size_t)row * a.h_in_stride + col];
        // the cell (rover_step.h): every line one rounding
        const float gr = gru_sigmoid((acc[0][r] + b_ir) + b_hr);
        const float gz = gru_sigmoid((acc[1][r] + b_iz) + b_hz);
        const float hn = acc[3][r] + b_hn;
        const float gn = tanhf((acc[2][r] + b_in) + gr * hn);
        const float keep = gz * h;
        const float take = (1.0f - gz) * gn;
        a.h_out[(size_t)row * a.h_out_stride + col] = take + keep;
        if constexpr (TRAIN) {
            float* __restrict__ g = a.gates + (size_t)row * a.gates_stride + col;
            g[0] = gr; g[H] = gz; g[2u * H] = gn; g[3u * H] = hn;
        }
    }
}

// The one place that decides what a cell launches, forward and backward: both run on a grid of row slabs x 32-column tiles of the
// hidden state.  Four waves (128 rows) per workgroup once that still leaves two workgroups for each of the 256 CUs; below, one wave per
// workgroup, which puts four times as many workgroups on the chip.  H: the launch grid's y limit (65 535 tiles of 32 columns).  The
// switch point is reasoned from the workgroup count, NOT measured, and so is leaving gru_cell<1> at one wave per SIMD (320 registers):
// at 512 envs and H = 300 it is 160 single-wave workgroups with nothing but their own prefetch to hide the global loads
// (EXPERIMENTS.md §16 lists the timings that would settle both).
static GruRoute gru_route(int M, int H) {
    if (M < 0 || H < 1 || H > 32 * 65535) return GruRoute{0};
    const int64_t tiles = (H + 31) / 32;
    return GruRoute{(((int64_t)M + 127) / 128) * tiles >= 512 ? 4 : 1};
}
GruRoute gru_cell_route(int M, int K, int H) { return K < 0 ? GruRoute{0} : gru_route(M, H); }
GruRoute gru_cell_backward_route(int M, int H) { return gru_route(M, H); }
const char* gru_cell_route_name(const GruRoute& r) { return r.nw == 4 ? "gru_cell<4>" : (r.nw == 1 ? "gru_cell<1>" : nullptr); }

hipError_t launch_gru_cell(const GruArgs& a, hipStream_t s) {
    const GruRoute r = gru_cell_route(a.M, a.K, a.H);
    const uint32_t tiles = (uint32_t)((a.H + 31) / 32);
    const dim3 g4((uint32_t)(((int64_t)a.M + 127) / 128), tiles), g1((uint32_t)(((int64_t)a.M + 31) / 32), tiles);
    if (r.nw == 4 && a.gates) hipLaunchKernelGGL((gru_cell_kernel<4, true>), g4, dim3(256), 0, s, a);
    else if (r.nw == 4) hipLaunchKernelGGL((gru_cell_kernel<4>), g4, dim3(256), 0, s, a);
    else if (r.nw == 1 && a.gates) hipLaunchKernelGGL((gru_cell_kernel<1, true>), g1, dim3(64), 0, s, a);
    else if (r.nw == 1) hipLaunchKernelGGL((gru_cell_kernel<1>), g1, dim3(64), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- the backward of one cell ------------------------------------------------------------------------------------------------------
// dh_in = dgh W_hh + g z on the same core with linear_dgrad_kernel's operands (rover_train.hip: a k-minor left slab, W_hh k-major as it
// lies, reduction over 3H in 32-wide slabs, one 32-column tile of dh_in per blockIdx.y); the left operand dgh is formed from the stored
// gates by the staging functor: no pass over [M, 3H] precedes the product.  Every workgroup forms the slabs it multiplies; the
// workgroups of column tile 0 (blockIdx.y == 0, a condition uniform over the workgroup) also store them as dgi / dgh.
// Arithmetic of element (m, c), every line one rounding (rover_step.h); h = h_in[m][c], 0 on a reset row:
//     g = dh_above + dh_next (dh_above alone without dh_next)
//     d_n = g (1 - z);  a_n = d_n (1 - n n);  d_z = g (h - n);  a_z = d_z (z (1 - z));  d_r = a_n q;  a_r = d_r (r (1 - r))
//     dgi = [a_r | a_z | a_n]     dgh = [a_r | a_z | a_n r]
//     dh_in = (sum over j < 3H of dgh_j W_hh[j][c], exact f32 MFMA in the order of j) + g z;   0 on a reset row
template <int NW>
__global__ void __launch_bounds__(64 * NW) gru_cell_backward_kernel(GruBwdArgs a) {
    using ASlab = F32KMinor<NW, 32 * NW>;
    using WSlab = F32KMajor<NW, 32>;
    __shared__ float As[ASlab::WORDS];                               // dgh[m][j slab]
    __shared__ float Ws[WSlab::WORDS];                               // W_hh[j slab][column tile]
    const ASlab as{As};
    const WSlab ws{Ws};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t row0 = blockIdx.x * (32u * NW), c0 = blockIdx.y * 32u;
    const uint32_t H = (uint32_t)a.H, M = (uint32_t)a.M, G = 3u * H;
    const bool writer = blockIdx.y == 0;                             // uniform over the workgroup
    f32x16 acc[1];
    f32_zero(acc);
    float pa[ASlab::NP], pi[ASlab::NP], pw[WSlab::NP];
    const uint32_t live = gru_live_rows<NW>(row0, M, a.reset_mask);
    auto fetch = [&](uint32_t j0) {
        ASlab::each([&](int j, uint32_t sr, uint32_t sc) {           // dgh into pa, dgi of the same element into pi
            const uint32_t gr = row0 + sr, gj = j0 + sc;             // gj: index into [a_r | a_z | a_n r]
            const uint32_t blk = gj >= 2u * H ? 2u : (gj >= H ? 1u : 0u), c = gj - blk * H;
            float vh = 0.0f, vi = 0.0f;
            if (gj < G && gr < M) {
                const float* __restrict__ gt = a.gates + (size_t)gr * a.gates_stride + c;
                float g = a.dh_above[(size_t)gr * a.dh_above_stride + c];
                if (a.dh_next) g = g + a.dh_next[(size_t)gr * a.dh_next_stride + c];
                const float z = gt[H], n = gt[2u * H];
                if (blk == 1u) {
                    const float h = ((live >> j) & 1u) ? a.h_in[(size_t)gr * a.h_in_stride + c] : 0.0f;
                    const float d_z = g * (h - n);
                    vh = vi = d_z * (z * (1.0f - z));
                } else {
                    const float d_n = g * (1.0f - z);
                    const float a_n = d_n * (1.0f - n * n);
                    const float r = gt[0];
                    if (blk == 2u) {
                        vi = a_n;
                        vh = a_n * r;
                    } else {
                        const float d_r = a_n * gt[3u * H];
                        vh = vi = d_r * (r * (1.0f - r));
                    }
                }
            }
            pa[j] = vh; pi[j] = vi;
        });
        WSlab::stage(pw, [&](uint32_t r, uint32_t c) {
            const uint32_t n = j0 + r, col = c0 + c;
            return (n < G && col < H) ? a.w_hh[(size_t)n * H + col] : 0.0f;
        });
    };
    auto stash = [&](uint32_t j0) {
        as.stash(pa);
        ws.stash(pw);
        ASlab::each([&](int j, uint32_t sr, uint32_t sc) {           // the workgroups of column tile 0 also store what they staged
            const uint32_t gr = row0 + sr, gj = j0 + sc;
            if (writer && gj < G && gr < M) {
                a.dgh[(size_t)gr * a.dgh_stride + gj] = pa[j];
                a.dgi[(size_t)gr * a.dgi_stride + gj] = pi[j];
            }
        });
    };
    // G is the same for every thread of the grid
    f32_slabs(0u, G, fetch, stash, [] {}, [&](uint32_t kk) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(as.operand(wave, kk), ws.operand(0, kk), acc[0], 0, 0, 0);
    });
    const uint32_t col = c0 + f32_cd(lane, 0).col;
    if (col >= H) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t row = row0 + wave * 32u + f32_cd(lane, r).row;
        if (row >= M) continue;
        float out = 0.0f;
        if (!(a.reset_mask && a.reset_mask[row])) {                  // nothing flows across an episode boundary
            float g = a.dh_above[(size_t)row * a.dh_above_stride + col];
            if (a.dh_next) g = g + a.dh_next[(size_t)row * a.dh_next_stride + col];
            const float gz = g * a.gates[(size_t)row * a.gates_stride + H + col];
            out = acc[0][r] + gz;
        }
        a.dh_in[(size_t)row * a.dh_in_stride + col] = out;
    }
}

const char* gru_cell_backward_route_name(const GruRoute& r) { return r.nw == 4 ? "gru_bwd<4>" : (r.nw == 1 ? "gru_bwd<1>" : nullptr); }

hipError_t launch_gru_cell_backward(const GruBwdArgs& a, hipStream_t s) {
    const GruRoute r = gru_cell_backward_route(a.M, a.H);
    const uint32_t tiles = (uint32_t)((a.H + 31) / 32);
    if (r.nw == 4) hipLaunchKernelGGL((gru_cell_backward_kernel<4>), dim3((uint32_t)(((int64_t)a.M + 127) / 128), tiles), dim3(256), 0, s, a);
    else if (r.nw == 1) hipLaunchKernelGGL((gru_cell_backward_kernel<1>), dim3((uint32_t)(((int64_t)a.M + 31) / 32), tiles), dim3(64), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// out = add + mul * sigmoid(pre), one thread per element (a row stride of 0 repeats one row of an input for every output row)
__global__ void __launch_bounds__(256) gated_sum_kernel(GatedSumArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)a.M * (uint64_t)a.N) return;
    const uint64_t row = i / (uint32_t)a.N, col = i % (uint32_t)a.N;
    const float g = gru_sigmoid(a.pre[row * (uint64_t)a.pre_stride + col]);
    const float p = a.mul[row * (uint64_t)a.mul_stride + col] * g;
    a.out[row * (uint64_t)a.out_stride + col] = a.add[row * (uint64_t)a.add_stride + col] + p;
}

hipError_t launch_gated_sum(const GatedSumArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(gated_sum_kernel, dim3(blocks_for((uint64_t)a.M * (uint64_t)a.N, 256u)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the gate's backward, one thread per element: s = sigmoid(pre) as the forward evaluates it; d_mul = d_out s; d_pre = (d_out mul) (s (1 - s))
__global__ void __launch_bounds__(256) gated_sum_backward_kernel(GatedSumBwdArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)a.M * (uint64_t)a.N) return;
    const uint64_t row = i / (uint32_t)a.N, col = i % (uint32_t)a.N;
    const float g = gru_sigmoid(a.pre[row * (uint64_t)a.pre_stride + col]);
    const float d = a.d_out[row * (uint64_t)a.d_out_stride + col];
    if (a.d_mul) a.d_mul[row * (uint64_t)a.d_mul_stride + col] = d * g;
    if (a.d_pre) {
        const float dm = d * a.mul[row * (uint64_t)a.mul_stride + col];
        a.d_pre[row * (uint64_t)a.d_pre_stride + col] = dm * (g * (1.0f - g));
    }
}

hipError_t launch_gated_sum_backward(const GatedSumBwdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(gated_sum_backward_kernel, dim3(blocks_for((uint64_t)a.M * (uint64_t)a.N, 256u)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rover
