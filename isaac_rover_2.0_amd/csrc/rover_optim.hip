// rover_optim.hip — the optimiser step of the PPO update on the device: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam
// (no weight decay, no amsgrad) over a list of tensors in two launches, with the KL early stop decided on the device (rover_optim_*
// of include/rover_step.h, which states the semantics; tests/optim_ref.py restates them independently in float64).
//
// Layout.  The tensors are cut into chunks of OPTIM_CHUNK elements (optim_plan: tensor order, then element order; the last chunk of
// a tensor is short, an empty tensor has none).  One workgroup of 256 threads owns one chunk in both launches; the device table holds
// per chunk the addresses of its first parameter and gradient element, its offset into the flat exp_avg / exp_avg_sq, its length and
// two alignment flags.  A chunk starts at a multiple of OPTIM_CHUNK elements of its tensor, so (p, g) can be moved 16 bytes at a time
// exactly when the tensor's bases are 16-byte aligned, and (m, v) when the tensor's offset into the flat state is a multiple of 4
// (after a tensor of 2 elements it is not: log_std_parameter comes first in the nets' list).  Each of the two groups takes the
// 16-byte path or the scalar path per chunk; thread t handles elements 4 t .. 4 t + 3 (+ 1 024 per round) either way, and the
// len % 4 tail elements are scalar, so the arithmetic and its order do not depend on the alignment.
//
// Launch 1, optim_prepare_kernel: workgroup c sums g*g of chunk c in f64 (an f32 square is exact in f64) — per thread in element
// order, then a fixed tree over the 64 lanes of a wave, then waves 0 .. 3 in order — and stores partials[c].  Thread 0 of workgroup 0
// evaluates the gate (header) and leaves (step, stopped) in the handle's record.
// Launch 2, optim_apply_kernel: every workgroup reads the record and returns if stopped.  Otherwise it adds the partials in one fixed
// order (thread i takes i, i + 256, ... in order, then a fixed tree: rover_ppo_loss's finishing kernel), forms the scalars in f64,
// rounds them to f32 once and runs the element update in f32 (-ffp-contract=off: one rounding per written operation).
// No floating-point atomics, no LDS beyond the two reductions: the same inputs give the same bits on every run.
#include "rover_internal.h"

#include <algorithm>

namespace rover {

int64_t optim_plan(int32_t n_tensors, const int64_t* numel, OptimChunkHost* out, int64_t capacity) {
    int64_t n = 0;
    for (int32_t t = 0; t < n_tensors; ++t)
        for (int64_t first = 0; first < numel[t]; first += OPTIM_CHUNK, ++n)
            if (n < capacity) out[n] = OptimChunkHost{t, (int32_t)first, (int32_t)std::min<int64_t>(OPTIM_CHUNK, numel[t] - first)};
    return n;
}

constexpr int OPTIM_BLOCK = 256;
static_assert(OPTIM_CHUNK % (4 * OPTIM_BLOCK) == 0, "a round of the workgroup covers 4 elements per thread");

// elements i .. i + 3 of q, as one 16-byte access or as four scalar ones
__device__ __forceinline__ float4 optim_load4(const float* q, uint32_t i, bool aligned) {
    if (aligned) return *reinterpret_cast<const float4*>(q + i);
    return make_float4(q[i], q[i + 1], q[i + 2], q[i + 3]);
}
__device__ __forceinline__ void optim_store4(float* q, uint32_t i, bool aligned, float4 v) {
    if (aligned) { *reinterpret_cast<float4*>(q + i) = v; return; }
    q[i] = v.x; q[i + 1] = v.y; q[i + 2] = v.z; q[i + 3] = v.w;
}

// the workgroup's sum of v: a fixed tree over the lanes of each wave, then the waves in order; valid in every thread
__device__ __forceinline__ double optim_block_sum(double v, double* sh /* [OPTIM_BLOCK / 64] */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int w = 1; w < OPTIM_BLOCK / 64; ++w) t += sh[w];
    return t;
}

__global__ void __launch_bounds__(OPTIM_BLOCK) optim_prepare_kernel(OptimArgs a) {
    __shared__ double sh[OPTIM_BLOCK / 64];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    if (c < a.n_chunks) {
        const OptimChunk ch = a.chunks[c];
        const uint32_t n4 = ch.len & ~3u;
        const bool al = (ch.flags & OPTIM_PG_ALIGNED) != 0;
        double s = 0.0;
        for (uint32_t i = tid * 4; i < n4; i += OPTIM_BLOCK * 4) {
            const float4 g = optim_load4(ch.g, i, al);
            s += (double)g.x * (double)g.x;
            s += (double)g.y * (double)g.y;
            s += (double)g.z * (double)g.z;
            s += (double)g.w * (double)g.w;
        }
        if (tid < ch.len - n4) {
            const double g = (double)ch.g[n4 + tid];
            s += g * g;
        }
        s = optim_block_sum(s, sh);
        if (tid == 0) a.partials[c] = s;
    }
    if (c == 0 && tid == 0) {
        bool stop = *a.stopped != 0;
        if (!stop && a.gate) stop = *a.gate > a.gate_threshold;       // a NaN gate does not stop
        int64_t step = *a.step;
        if (stop) {
            *a.stopped = 1;
        } else {
            step += 1;
            *a.step = step;
        }
        a.record->step = step;
        a.record->stopped = stop ? 1 : 0;
    }
}

// b^t for t >= 0 by repeated squaring (f64: a relative error of a few 2^-53 per squaring, far below the f32 rounding that follows)
__device__ __forceinline__ double optim_powi(double b, int64_t t) {
    double r = 1.0;
    for (; t > 0; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

// The element update (normative; all f32, one rounding per operation), with the scalars rounded to f32 once:
//     g' = g * coef;  m = m + (g' - m) * omb1;  v = beta2 * v + (omb2 * g') * g';  p = p - step_size * (m / (sqrtf(v) / sqrt_bc2 + eps))
struct OptimScalars { float coef, omb1, beta2, omb2, step_size, sqrt_bc2, eps; };
__device__ __forceinline__ void optim_update(const OptimScalars& k, float g, float& p, float& m, float& v) {
    const float gc = g * k.coef;
    m = m + (gc - m) * k.omb1;
    v = k.beta2 * v + (k.omb2 * gc) * gc;
    p = p - k.step_size * (m / (sqrtf(v) / k.sqrt_bc2 + k.eps));
}

__global__ void __launch_bounds__(OPTIM_BLOCK) optim_apply_kernel(OptimArgs a) {
    __shared__ double sh[OPTIM_BLOCK / 64];
    const OptimRecord rec = *a.record;
    if (rec.stopped) return;                           // parameters, state and step stay as they are
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    double total = 0.0;
    for (uint32_t i = tid; i < a.n_chunks; i += OPTIM_BLOCK) total += a.partials[i];
    total = optim_block_sum(total, sh);
    const double norm = sqrt(total);
    if (c == 0 && tid == 0 && a.norm_out) *a.norm_out = norm;
    if (c >= a.n_chunks) return;
    double coef = 1.0;
    if (a.clip > 0.0) {
        coef = a.clip / (norm + 1e-6);
        coef = coef > 1.0 ? 1.0 : coef;                // torch.clamp(max = 1): a NaN stays a NaN
    }
    const double bc1 = 1.0 - optim_powi(a.beta1, rec.step), bc2 = 1.0 - optim_powi(a.beta2, rec.step);
    OptimScalars k;
    k.coef = (float)coef; k.omb1 = (float)(1.0 - a.beta1); k.beta2 = (float)a.beta2; k.omb2 = (float)(1.0 - a.beta2);
    k.step_size = (float)(a.lr / bc1); k.sqrt_bc2 = (float)sqrt(bc2); k.eps = (float)a.eps;

    const OptimChunk ch = a.chunks[c];
    float* const mm = a.exp_avg + ch.state;
    float* const vv = a.exp_avg_sq + ch.state;
    const uint32_t n4 = ch.len & ~3u;
    const bool al = (ch.flags & OPTIM_PG_ALIGNED) != 0, sal = (ch.flags & OPTIM_STATE_ALIGNED) != 0;
    for (uint32_t i = tid * 4; i < n4; i += OPTIM_BLOCK * 4) {
        const float4 g = optim_load4(ch.g, i, al);
        float4 p = optim_load4(ch.p, i, al), m = optim_load4(mm, i, sal), v = optim_load4(vv, i, sal);
        optim_update(k, g.x, p.x, m.x, v.x);
        optim_update(k, g.y, p.y, m.y, v.y);
        optim_update(k, g.z, p.z, m.z, v.z);
        optim_update(k, g.w, p.w, m.w, v.w);
        optim_store4(ch.p, i, al, p);
        optim_store4(mm, i, sal, m);
        optim_store4(vv, i, sal, v);
    }
    if (tid < ch.len - n4) {
        const uint32_t i = n4 + tid;
        float p = ch.p[i], m = mm[i], v = vv[i];
        optim_update(k, ch.g[i], p, m, v);
        ch.p[i] = p; mm[i] = m; vv[i] = v;
    }
}

hipError_t launch_optim_step(const OptimArgs& a, hipStream_t s) {
    const uint32_t grid = a.n_chunks ? a.n_chunks : 1;     // no chunk at all: the gate and the counter still run
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(grid), dim3(OPTIM_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(optim_apply_kernel, dim3(grid), dim3(OPTIM_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace rover
