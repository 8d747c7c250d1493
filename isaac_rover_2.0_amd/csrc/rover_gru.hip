// rover_gru.hip — the student policy's recurrent block: one GRU layer for one time step in ONE launch, and the sigmoid gate that
// follows it.
//
// Reference: omniisaacgymenvs/tasks/utils/learning_by_cheating/student_model.py — Belief_Encoder (:42-92): nn.GRU(124 -> 300, 2 layers)
// whose output feeds two Layer chains gb / ga, belief = gb(out) + l_e * sigmoid(ga(out)); Belief_Decoder (:94-131):
// estimated = decoded + e * sigmoid(gate).  student_loader.act (:21-24) runs one time step per env step with a carried hidden state.
//
// gru_cell_kernel is linear_act_kernel's structure (rover_mlp.hip) specialised: a 32-row slab of the left operand per wave at the
// 33-word pitch (conflict-free column reads), the weights read as they lie ([3H][K] and [3H][H], lane on k), exact f32 MFMA
// (v_mfma_f32_32x32x2_f32).  The left operand is x followed by h along the reduction.  A workgroup owns 32 NW rows and ONE 32-column
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

namespace rover {

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define GRU_BK 32
#define GRU_PITCH 33

// (gru_sigmoid is rover_act.h's)

// TRAIN: the epilogue also stores r | z | n | q (q = s_hn + b_hn) to a.gates for the backward; h' is computed by the same operations.
template <int NW, bool TRAIN = false>
__global__ void __launch_bounds__(64 * NW, NW == 1 ? 1 : 2) gru_cell_kernel(GruArgs a) {
    constexpr uint32_t BM = 32u * NW, RSTEP = 2u * NW;               // rows per workgroup; rows staged per pass
    __shared__ float As[BM * GRU_PITCH];                             // the left operand's k-slab: x, then h
    __shared__ float Ws[3 * 32 * GRU_PITCH];                         // weight rows j, H + j, 2H + j of the same k-slab
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t row0 = blockIdx.x * BM, n0 = blockIdx.y * 32u;    // blockIdx.y: the 32-column tile of the hidden state
    const uint32_t H = (uint32_t)a.H, M = (uint32_t)a.M;
    f32x16 acc_r, acc_z, acc_in, acc_hn;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_r[r] = acc_z[r] = acc_in[r] = acc_hn[r] = 0.0f;
    const uint32_t ar = lane & 31u, ak = lane >> 5;                  // A[i = lane&31][k = lane>>5], B[k = lane>>5][j = lane&31]
    const uint32_t sc = tid & 31u, sr = tid >> 5;                    // staging: thread (row sr + RSTEP j, k column sc), 128-byte rows
    float pa[BM / RSTEP], pw[3 * 32 / RSTEP];
    // rows of h_in that reset_mask marks are read as zeros (here, in the products, and in the epilogue's z * h)
    uint32_t live = 0u;                                              // bit j: staged row j of this thread keeps its h_in
#pragma unroll
    for (int j = 0; j < (int)(BM / RSTEP); ++j) {
        const uint32_t gr = row0 + sr + RSTEP * j;
        if (gr < M && !(a.reset_mask && a.reset_mask[gr])) live |= 1u << j;
    }
    // slab s of the reduction: the slabs of x (zero past K), then those of h (zero past H, and on reset rows) — the left operand's
    // columns k0 .. k0 + 31 and the same columns of the three gates' weight rows
    const uint32_t sx = ((uint32_t)a.K + GRU_BK - 1u) / GRU_BK, sh = (H + GRU_BK - 1u) / GRU_BK, ns = sx + sh;
    auto fetch = [&](uint32_t s) {
        const bool phase_h = s >= sx;
        const uint32_t Kp = phase_h ? H : (uint32_t)a.K, gk = (phase_h ? s - sx : s) * GRU_BK + sc;
        const float* __restrict__ w = phase_h ? a.w_hh : a.w_ih;
        const float* __restrict__ src = phase_h ? a.h_in : a.x;
        const int64_t src_stride = phase_h ? a.h_in_stride : a.x_stride;
        const bool kin = gk < Kp;
#pragma unroll
        for (int j = 0; j < (int)(BM / RSTEP); ++j) {
            const uint32_t gr = row0 + sr + RSTEP * j;
            const bool ok = kin && gr < M && (!phase_h || ((live >> j) & 1u));
            pa[j] = ok ? src[(size_t)gr * src_stride + gk] : 0.0f;
        }
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int j = 0; j < (int)(32 / RSTEP); ++j) {
                const uint32_t n = n0 + sr + RSTEP * j;               // column of the hidden state; weight row g H + n
                pw[g * (32 / RSTEP) + j] = (kin && n < H) ? w[((size_t)g * H + n) * Kp + gk] : 0.0f;
            }
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < (int)(BM / RSTEP); ++j) As[(sr + RSTEP * j) * GRU_PITCH + sc] = pa[j];
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int j = 0; j < (int)(32 / RSTEP); ++j) Ws[(g * 32u + sr + RSTEP * j) * GRU_PITCH + sc] = pw[g * (32 / RSTEP) + j];
    };
    fetch(0);                                                        // the slab after the current one is in flight during its MFMAs
    for (uint32_t s = 0; s < ns; ++s) {
        stash();
        __syncthreads();
        if (s + 1 < ns) fetch(s + 1);
        if (s < sx) {
#pragma unroll 4
            for (uint32_t kk = 0; kk < GRU_BK; kk += 2) {
                const float av = As[(wave * 32u + ar) * GRU_PITCH + kk + ak];
                acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Ws[(0u * 32u + ar) * GRU_PITCH + kk + ak], acc_r, 0, 0, 0);
                acc_z = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Ws[(1u * 32u + ar) * GRU_PITCH + kk + ak], acc_z, 0, 0, 0);
                acc_in = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Ws[(2u * 32u + ar) * GRU_PITCH + kk + ak], acc_in, 0, 0, 0);
            }
        } else {
#pragma unroll 4
            for (uint32_t kk = 0; kk < GRU_BK; kk += 2) {
                const float av = As[(wave * 32u + ar) * GRU_PITCH + kk + ak];
                acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Ws[(0u * 32u + ar) * GRU_PITCH + kk + ak], acc_r, 0, 0, 0);
                acc_z = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Ws[(1u * 32u + ar) * GRU_PITCH + kk + ak], acc_z, 0, 0, 0);
                acc_hn = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Ws[(2u * 32u + ar) * GRU_PITCH + kk + ak], acc_hn, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const uint32_t col = n0 + (lane & 31u);
    if (col >= H) return;
    const float b_ir = a.b_ih ? a.b_ih[col] : 0.0f, b_iz = a.b_ih ? a.b_ih[H + col] : 0.0f, b_in = a.b_ih ? a.b_ih[2u * H + col] : 0.0f;
    const float b_hr = a.b_hh ? a.b_hh[col] : 0.0f, b_hz = a.b_hh ? a.b_hh[H + col] : 0.0f, b_hn = a.b_hh ? a.b_hh[2u * H + col] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t row = row0 + wave * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
        if (row >= M) continue;
        const bool reset = a.reset_mask && a.reset_mask[row];
        const float h = reset ? 0.0f : a.h_in[(size_t)row * a.h_in_stride + col];
        // the cell (rover_step.h): every line one rounding
        const float gr = gru_sigmoid((acc_r[r] + b_ir) + b_hr);
        const float gz = gru_sigmoid((acc_z[r] + b_iz) + b_hz);
        const float hn = acc_hn[r] + b_hn;
        const float gn = tanhf((acc_in[r] + b_in) + gr * hn);
        const float keep = gz * h;
        const float take = (1.0f - gz) * gn;
        a.h_out[(size_t)row * a.h_out_stride + col] = take + keep;
        if constexpr (TRAIN) {
            float* __restrict__ g = a.gates + (size_t)row * a.gates_stride + col;
            g[0] = gr; g[H] = gz; g[2u * H] = gn; g[3u * H] = hn;
        }
    }
}

// The one place that decides what a cell launches.  Four waves (128 rows) per workgroup once that still leaves two workgroups for
// each of the 256 CUs; below, one wave per workgroup, which puts four times as many workgroups on the chip.  H: the launch grid's y
// limit (65 535 tiles of 32 columns).  The switch point is reasoned from the workgroup count, NOT measured, and so is leaving
// gru_cell<1> at one wave per SIMD (320 registers): at 512 envs and H = 300 it is 160 single-wave workgroups with nothing but their
// own prefetch to hide the global loads (EXPERIMENTS.md §16 lists the timings that would settle both).
GruRoute gru_cell_route(int M, int K, int H) {
    if (M < 0 || K < 0 || H < 1 || H > 32 * 65535) return GruRoute{0};
    const int64_t tiles = (H + 31) / 32;
    return GruRoute{(((int64_t)M + 127) / 128) * tiles >= 512 ? 4 : 1};
}
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
// dh_in = dgh W_hh + g z is linear_dgrad_kernel's product (rover_train.hip: 32-row slabs of the left operand at the 33-word pitch, W_hh
// read as it lies, reduction over 3H in 32-wide slabs, one 32-column tile of dh_in per blockIdx.y) whose left operand dgh is formed from
// the stored gates while it is staged: no pass over [M, 3H] precedes the product.  Every workgroup forms the slabs it multiplies; the
// workgroups of column tile 0 (blockIdx.y == 0, a condition uniform over the workgroup) also store them as dgi / dgh.
// Arithmetic of element (m, c), every line one rounding (rover_step.h); h = h_in[m][c], 0 on a reset row:
//     g = dh_above + dh_next (dh_above alone without dh_next)
//     d_n = g (1 - z);  a_n = d_n (1 - n n);  d_z = g (h - n);  a_z = d_z (z (1 - z));  d_r = a_n q;  a_r = d_r (r (1 - r))
//     dgi = [a_r | a_z | a_n]     dgh = [a_r | a_z | a_n r]
//     dh_in = (sum over j < 3H of dgh_j W_hh[j][c], exact f32 MFMA in the order of j) + g z;   0 on a reset row
template <int NW>
__global__ void __launch_bounds__(64 * NW) gru_cell_backward_kernel(GruBwdArgs a) {
    constexpr uint32_t BM = 32u * NW, RSTEP = 2u * NW;
    __shared__ float As[BM * GRU_PITCH];                             // dgh[m][j slab]
    __shared__ float Ws[32 * 32];                                    // W_hh[j slab][column tile]: row reads, no padding needed
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t row0 = blockIdx.x * BM, c0 = blockIdx.y * 32u;
    const uint32_t H = (uint32_t)a.H, M = (uint32_t)a.M, G = 3u * H;
    const uint32_t ar = lane & 31u, ak = lane >> 5;
    const uint32_t sc = tid & 31u, sr = tid >> 5;
    const bool writer = blockIdx.y == 0;                             // uniform over the workgroup
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    float pa[BM / RSTEP], pi[BM / RSTEP], pw[32 / RSTEP];
    uint32_t live = 0u;                                              // bit j: staged row j of this thread keeps its h_in
#pragma unroll
    for (int j = 0; j < (int)(BM / RSTEP); ++j) {
        const uint32_t gr = row0 + sr + RSTEP * j;
        if (gr < M && !(a.reset_mask && a.reset_mask[gr])) live |= 1u << j;
    }
    auto fetch = [&](uint32_t j0) {
        const uint32_t gj = j0 + sc;                                 // index into [a_r | a_z | a_n r]
        const uint32_t blk = gj >= 2u * H ? 2u : (gj >= H ? 1u : 0u), c = gj - blk * H;
#pragma unroll
        for (int j = 0; j < (int)(BM / RSTEP); ++j) {
            const uint32_t gr = row0 + sr + RSTEP * j;
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
        }
#pragma unroll
        for (int j = 0; j < (int)(32 / RSTEP); ++j) {
            const uint32_t n = j0 + sr + RSTEP * j, col = c0 + sc;
            pw[j] = (n < G && col < H) ? a.w_hh[(size_t)n * H + col] : 0.0f;
        }
    };
    auto stash = [&](uint32_t j0) {
        const uint32_t gj = j0 + sc;
#pragma unroll
        for (int j = 0; j < (int)(BM / RSTEP); ++j) {
            As[(sr + RSTEP * j) * GRU_PITCH + sc] = pa[j];
            const uint32_t gr = row0 + sr + RSTEP * j;
            if (writer && gj < G && gr < M) {
                a.dgh[(size_t)gr * a.dgh_stride + gj] = pa[j];
                a.dgi[(size_t)gr * a.dgi_stride + gj] = pi[j];
            }
        }
#pragma unroll
        for (int j = 0; j < (int)(32 / RSTEP); ++j) Ws[(sr + RSTEP * j) * 32u + sc] = pw[j];
    };
    fetch(0);
    for (uint32_t j0 = 0; j0 < G; j0 += 32u) {                       // G is the same for every thread of the grid
        stash(j0);
        __syncthreads();
        if (j0 + 32u < G) fetch(j0 + 32u);                           // in flight during the MFMAs below
#pragma unroll 4
        for (uint32_t kk = 0; kk < 32u; kk += 2) {
            const float av = As[(wave * 32u + ar) * GRU_PITCH + kk + ak];
            const float bv = Ws[(kk + ak) * 32u + ar];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const uint32_t col = c0 + (lane & 31u);
    if (col >= H) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t row = row0 + wave * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
        if (row >= M) continue;
        float out = 0.0f;
        if (!(a.reset_mask && a.reset_mask[row])) {                  // nothing flows across an episode boundary
            float g = a.dh_above[(size_t)row * a.dh_above_stride + col];
            if (a.dh_next) g = g + a.dh_next[(size_t)row * a.dh_next_stride + col];
            const float gz = g * a.gates[(size_t)row * a.gates_stride + H + col];
            out = acc[r] + gz;
        }
        a.dh_in[(size_t)row * a.dh_in_stride + col] = out;
    }
}

// The forward cell's rule on the same grid (row slabs x 32-column tiles of the hidden state), reasoned from the workgroup count, not measured.
GruRoute gru_cell_backward_route(int M, int H) {
    if (M < 0 || H < 1 || H > 32 * 65535) return GruRoute{0};
    const int64_t tiles = (H + 31) / 32;
    return GruRoute{(((int64_t)M + 127) / 128) * tiles >= 512 ? 4 : 1};
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
