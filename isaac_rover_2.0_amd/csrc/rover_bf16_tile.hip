// rover_bf16_tile.hip — the student policy in bf16 (precision = "bf16"): the GRU cell and one Layer, on ONE staging and
// MFMA core.  The arithmetic is stated in rover_step.h at rover_gru_cell_bf16 / rover_linear_forward_bf16; the tests hold the kernels to it.
//
// b16_product is chain_bf16's first layer (rover_mlp.hip, b16_layer1) generalised: v_mfma_f32_16x16x32_bf16 transposed,
// D[n][m] = W[n][k] X^T[k][m].  A = 16 weight rows, B = 16 rows of the left operand, lane (m = lane & 15, g = lane >> 4) supplies k-slots
// 8 g .. 8 g + 7 of both as one 16-byte LDS read; D: lane (m, g) holds output columns 16 t + 4 g + r (r < 4) of row m.  The f32 rows are
// read 16 bytes at a time at any float address, rounded (bf16_rne) while they are staged, and kept in LDS as [row][32 k] bf16 at the pitch
// B16_P; the slab after the current one is in flight during its MFMAs, and two LDS buffers make one barrier per slab enough.
//   * a wave owns RT row tiles of 16 and all CT column tiles of each of the NG weight-row groups: an A read feeds RT MFMAs;
//   * the reduction is the slabs of x (zero-filled to a multiple of 32), then the slabs of h (likewise): a k-step never mixes the two.
// The kernels are bound by the bytes staged from L2, not by the matrix pipe: a workgroup of BM rows x BN columns stages
// 128 (BM + NG BN) bytes of f32 per slab for NG BM BN / 64 MFMA cycles (EXPERIMENTS.md §20 has the tile choice and the resource table).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rover_internal.h"
#include "rover_act.h"
#include "rover_bf16.h"

namespace rover {

// one side of the reduction: rows of the left operand [M][K] at a stride, and the weight rows [.][K] that multiply them
struct B16Side { const float* a; int64_t a_stride; const float* w; uint32_t K; };

// acc[gi][q][t] += W rows (gi N + n0 + 16 t ..) . left rows (row0 + 16 (RT wave + q) ..) over x's K then h's K.  SPLIT: the last group
// keeps the two sides apart — acc[NG - 1] over x, acc[NG] over h (the cell's s_in and s_hn).  live: bit j set = staged row j of this
// thread reads h (else zeros: a reset row); rows past M are zeros on both sides.
template <int NW, int RT, int CT, int NG, bool SPLIT>
__device__ __forceinline__ void b16_product(f32x4 (&acc)[SPLIT ? NG + 1 : NG][RT][CT], const B16Side& x, const B16Side& h, uint32_t M, uint32_t N,
                                            uint32_t row0, uint32_t n0, uint32_t live, __bf16* __restrict__ lds /* 2 x [BM + NG BN][B16_P] */) {
    constexpr uint32_t BM = 16u * RT * NW, BN = 16u * CT, WR = NG * BN, RS = 8u * NW;      // RS: rows staged per pass (8 threads per row)
    constexpr int XJ = BM / RS, WJ = WR / RS;
    constexpr uint32_t BUF = (BM + WR) * B16_P;
    static_assert(WR % RS == 0 && XJ <= 32 && (BN % RS == 0 || RS % BN == 0), "whole staging passes; one live bit per staged row");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, m = lane & 15u, g = lane >> 4;
    const uint32_t c4 = tid & 7u, r0 = tid >> 3;                     // 16-byte column of the f32 slab; first slab row of this thread
    const uint32_t sx = (x.K + 31u) / 32u, ns = sx + (h.K + 31u) / 32u;
    f32x4 px[XJ], pw[WJ];
    auto fetch = [&](uint32_t s) {
        const bool ph = s >= sx;
        const float* __restrict__ src = ph ? h.a : x.a;
        const float* __restrict__ w = ph ? h.w : x.w;
        const int64_t stride = ph ? h.a_stride : x.a_stride;
        const uint32_t Kp = ph ? h.K : x.K, k = (ph ? s - sx : s) * 32u + 4u * c4;
        // row j of this thread = its first row + j * (a uniform step): ONE 64-bit address per operand that moves with the slab, not XJ + WJ
        // loop-invariant row pointers per side held in registers across the MFMAs
        const float* __restrict__ pa = src + (size_t)(row0 + r0) * stride;
        const float* __restrict__ pb = w + (size_t)(n0 + r0 % BN) * Kp;
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const uint32_t gr = row0 + r0 + RS * j;
            px[j] = b16_load4(pa + (size_t)(RS * j) * stride, k, Kp, gr < M && (!ph || ((live >> j) & 1u)));
        }
#pragma unroll
        for (int j = 0; j < WJ; ++j) {
            // weight row (wl / BN) N + n0 + wl % BN, wl = r0 + RS j; RS divides BN or BN divides RS, so wl / BN and wl % BN - r0 % BN are uniform
            const uint32_t gi = RS <= BN ? (RS * j) / BN : r0 / BN + (RS / BN) * j, dn = RS <= BN ? (RS * j) % BN : 0u;
            pw[j] = b16_load4(pb + ((size_t)gi * N + dn) * Kp, k, Kp, n0 + r0 % BN + dn < N);
        }
    };
    if (ns) fetch(0);
    // one slab: stash what was fetched, prefetch the next, multiply.  LAST_H: the last group accumulates into acc[NG] (the h side)
    auto slab = [&](uint32_t s, auto last_h) {
        __bf16* __restrict__ Xs = lds + (s & 1u) * BUF;
        __bf16* __restrict__ Ws = Xs + BM * B16_P;
#pragma unroll
        for (int j = 0; j < XJ; ++j) *reinterpret_cast<bf16x4*>(Xs + (r0 + RS * j) * B16_P + 4u * c4) = b16_round4(px[j]);
#pragma unroll
        for (int j = 0; j < WJ; ++j) *reinterpret_cast<bf16x4*>(Ws + (r0 + RS * j) * B16_P + 4u * c4) = b16_round4(pw[j]);
        // one barrier per slab: whoever stores slab s + 1 into the other buffer has passed this one, so every wave is done with slab s - 1
        __syncthreads();
        if (s + 1 < ns) fetch(s + 1);                                // in flight during the MFMAs below
        bf16x8 xb[RT];
#pragma unroll
        for (int q = 0; q < RT; ++q) xb[q] = *reinterpret_cast<const bf16x8*>(Xs + ((wave * RT + q) * 16u + m) * B16_P + 8u * g);
        // the A reads of group gi + 1 are issued before the MFMAs of group gi and nothing moves across a group's end: two groups' operands
        // are live at a time, not all NG CT of them
        auto read_w = [&](bf16x8 (&wa)[CT], int gi) {
#pragma unroll
            for (int t = 0; t < CT; ++t) wa[t] = *reinterpret_cast<const bf16x8*>(Ws + (gi * BN + 16u * t + m) * B16_P + 8u * g);
        };
        auto group = [&](f32x4 (&d)[RT][CT], const bf16x8 (&wa)[CT]) {
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int q = 0; q < RT; ++q) d[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[t], xb[q], d[q][t], 0, 0, 0);
        };
        bf16x8 wa[2][CT];
        read_w(wa[0], 0);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            if (gi + 1 < NG) read_w(wa[(gi + 1) & 1], gi + 1);
            group(acc[decltype(last_h)::value && gi == NG - 1 ? NG : gi], wa[gi & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // two loops, the split accumulator a compile-time choice: as one loop with a uniform branch hipcc kept both targets live and spilled
    uint32_t s = 0;
    for (; s < sx; ++s) slab(s, std::false_type{});
    for (; s < ns; ++s) slab(s, std::integral_constant<bool, SPLIT>{});
}

template <int N0, int RT, int CT>
__device__ __forceinline__ void b16_zero(f32x4 (&acc)[N0][RT][CT]) {
#pragma unroll
    for (int i = 0; i < N0; ++i)
#pragma unroll
        for (int q = 0; q < RT; ++q)
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[i][q][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// ---- the cell -----------------------------------------------------------------------------------------------------------------------
// Four accumulator groups as in gru_cell_kernel (rover_gru.hip): r and z over K + H, s_in over the x slabs, s_hn over the h slabs.  The
// epilogue is that kernel's, operation for operation, on the UNROUNDED f32 h_in (0 on a reset row): the state never passes through bf16.
template <int NW, int RT, int CT>
__global__ void __launch_bounds__(64 * NW, 2) gru_cell_bf16_kernel(GruArgs a) {
    constexpr uint32_t BM = 16u * RT * NW, BN = 16u * CT, RS = 8u * NW;
    __shared__ __attribute__((aligned(16))) __bf16 lds[2u * (BM + 3u * BN) * B16_P];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, m = lane & 15u, g = lane >> 4;
    const uint32_t row0 = blockIdx.x * BM, n0 = blockIdx.y * BN;     // blockIdx.y: the BN-column tile of the hidden state
    const uint32_t H = (uint32_t)a.H, M = (uint32_t)a.M;
    uint32_t live = 0u;
#pragma unroll
    for (int j = 0; j < (int)(BM / RS); ++j) {
        const uint32_t gr = row0 + (tid >> 3) + RS * j;
        if (gr < M && !(a.reset_mask && a.reset_mask[gr])) live |= 1u << j;
    }
    f32x4 acc[4][RT][CT];                                            // r, z, in, hn
    b16_zero(acc);
    const B16Side sx{a.x, a.x_stride, a.w_ih, (uint32_t)a.K}, sh{a.h_in, a.h_in_stride, a.w_hh, H};
    b16_product<NW, RT, CT, 3, true>(acc, sx, sh, M, H, row0, n0, live, lds);
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const uint32_t c0 = n0 + 16u * t + 4u * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t col = c0 + r;
            if (col >= H) continue;
            const float b_ir = a.b_ih ? a.b_ih[col] : 0.0f, b_iz = a.b_ih ? a.b_ih[H + col] : 0.0f, b_in = a.b_ih ? a.b_ih[2u * H + col] : 0.0f;
            const float b_hr = a.b_hh ? a.b_hh[col] : 0.0f, b_hz = a.b_hh ? a.b_hh[H + col] : 0.0f, b_hn = a.b_hh ? a.b_hh[2u * H + col] : 0.0f;
#pragma unroll
            for (int q = 0; q < RT; ++q) {
                const uint32_t row = row0 + (wave * RT + q) * 16u + m;
                if (row >= M) continue;
                const bool reset = a.reset_mask && a.reset_mask[row];
                const float h = reset ? 0.0f : a.h_in[(size_t)row * a.h_in_stride + col];
                // the cell (rover_step.h): every line one rounding
                const float gr = gru_sigmoid((acc[0][q][t][r] + b_ir) + b_hr);
                const float gz = gru_sigmoid((acc[1][q][t][r] + b_iz) + b_hz);
                const float hn = acc[3][q][t][r] + b_hn;
                const float gn = tanhf((acc[2][q][t][r] + b_in) + gr * hn);
                const float keep = gz * h;
                const float take = (1.0f - gz) * gn;
                a.h_out[(size_t)row * a.h_out_stride + col] = take + keep;
            }
        }
    }
}

// ONE instantiation at every batch size: 8 waves x 1 row tile = 128 rows, 4 column tiles = 64 columns of the hidden state per workgroup
// (64 accumulator registers, 126 VGPRs: two workgroups per CU, four waves per SIMD).  Measured against 4 waves x 2 row tiles (the same
// 128 x 64 tile at half the LDS operand reads, 216 VGPRs, two waves per SIMD), 256 x 64 and 64 x 64: EXPERIMENTS.md §20 — the kernel waits
// on the slab it prefetched, not on LDS or the matrix pipe, and the waves per SIMD are what hides that.  The refusals are the f32 cell's.
#define GRU_B16_NW 8
#define GRU_B16_RT 1
#define GRU_B16_CT 4
const char* gru_cell_route_bf16_name(int M, int K, int H) {
    if (!gru_cell_route(M, K, H).nw) return nullptr;
    return "gru_cell_bf16<128,64>";
}

hipError_t launch_gru_cell_bf16(const GruArgs& a, hipStream_t s) {
    if (!gru_cell_route_bf16_name(a.M, a.K, a.H) || a.gates) return hipErrorInvalidValue;
    constexpr int BM = 16 * GRU_B16_RT * GRU_B16_NW, BN = 16 * GRU_B16_CT;
    const dim3 grid((uint32_t)(((int64_t)a.M + BM - 1) / BM), (uint32_t)((a.H + BN - 1) / BN));
    hipLaunchKernelGGL((gru_cell_bf16_kernel<GRU_B16_NW, GRU_B16_RT, GRU_B16_CT>), grid, dim3(64 * GRU_B16_NW), 0, s, a);
    return hipGetLastError();
}

// ---- one Layer ------------------------------------------------------------------------------------------------------------------------
// y = act(x W^T + b) with the same core and ONE accumulator group: 128 rows x 128 columns per workgroup (64 accumulator registers), the
// column tiles of N <= 256 on grid.y.  Bias and mlp_act in f32, f32 output: whoever reads y next rounds it as it reads.
template <int NW, int RT, int CT>
__global__ void __launch_bounds__(64 * NW, 2) linear_bf16_kernel(LinearArgs a) {
    constexpr uint32_t BM = 16u * RT * NW, BN = 16u * CT;
    __shared__ __attribute__((aligned(16))) __bf16 lds[2u * (BM + BN) * B16_P];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, m = lane & 15u, g = lane >> 4;
    const uint32_t row0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const uint32_t N = (uint32_t)a.N, M = (uint32_t)a.M;
    f32x4 acc[1][RT][CT];
    b16_zero(acc);
    const B16Side sx{a.x, a.x_stride, a.w, (uint32_t)a.K}, none{nullptr, 0, nullptr, 0u};
    b16_product<NW, RT, CT, 1, false>(acc, sx, none, M, N, row0, n0, 0u, lds);
#pragma unroll
    for (int t = 0; t < CT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t col = n0 + 16u * t + 4u * g + r;
            if (col >= N) continue;
            const float bias = a.b ? a.b[col] : 0.0f;
#pragma unroll
            for (int q = 0; q < RT; ++q) {
                const uint32_t row = row0 + (wave * RT + q) * 16u + m;
                if (row < M) a.y[(size_t)row * a.y_stride + col] = mlp_act(acc[0][q][t][r] + bias, a.act);
            }
        }
    }
}

#define LIN_B16_NW 4
#define LIN_B16_RT 2
#define LIN_B16_CT 8
const char* linear_route_bf16_name(int M, int N) {
    if (!linear_route(M, N).nw) return nullptr;                      // rover_linear_forward's refusals: M < 0, N outside 1 .. 256
    return "linear_bf16<128,128>";
}

hipError_t launch_linear_bf16(const LinearArgs& a, hipStream_t s) {
    if (!linear_route_bf16_name(a.M, a.N)) return hipErrorInvalidValue;
    constexpr int BM = 16 * LIN_B16_RT * LIN_B16_NW, BN = 16 * LIN_B16_CT;
    const dim3 grid((uint32_t)(((int64_t)a.M + BM - 1) / BM), (uint32_t)((a.N + BN - 1) / BN));
    hipLaunchKernelGGL((linear_bf16_kernel<LIN_B16_NW, LIN_B16_RT, LIN_B16_CT>), grid, dim3(64 * LIN_B16_NW), 0, s, a);
    return hipGetLastError();
}

}  // namespace rover
