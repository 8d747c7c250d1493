// rover_obs.hip — observation assembly, metrics and done, the done compaction and the evaluation summaries (gfx950, wave64).
//
// Reference (pure PyTorch; paths relative to omniisaacgymenvs/):
//   tasks/rover.py:272-336 get_observations, :460-531 calculate_metrics, :610-647 is_done, :663-668 check_collision
// Built with -ffp-contract=off: see rover_rays.hip.
// Kernels (* = part of the fused step):
// * obs_metrics_kernel       assemble_obs (1 thread / 4 obs elements, coalesced rows) + metrics_done (1 thread / env: collision mask,
//                            stone mask, reward, extras, done, done count) in one launch                            (A1, A7, A8, A10)
//   assemble_obs_kernel / metrics_done_kernel   the same two passes on their own (the reference's method split)
// * compact_write_kernel     ballot/popc ordered stream compaction of the reset ids                                 (A12)
//   eval_summary / eval_clear kernels   rover_eval_read / rover_eval_clear
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"
#include "rover_stones.h"       // collides_grid
#include "rover_blockscan.h"    // block_count_flags

namespace rover {

// ---------------------------------------------------------------------------------------------------
// obs assembly: one thread per obs element -> coalesced row writes (rover.py:320-325)
// ---------------------------------------------------------------------------------------------------
#define OBS_ILP 4
__device__ __forceinline__ void assemble_obs_block(const ObsArgs& a, uint32_t bid, uint32_t n_blocks) {
    // One thread = OBS_ILP obs elements, a grid apart.  All loads come first and from addresses that are valid for every lane: a
    // wave holds the four proprioceptive columns of one or two envs next to heightmap columns, and with the loads inside the
    // five branches it waited for memory once per branch (six round trips in a row, 3.9 us per wave: 21 us for 21 MB).  Now the
    // chain is index -> distance with everything else beside it, four elements in flight per lane.
    const uint64_t total = (uint64_t)a.E * a.W, stride = (uint64_t)n_blocks * 256u;
    const uint64_t i0 = (uint64_t)bid * 256u + threadIdx.x;
    const bool small = total <= 0xffffffffull;      // (uniform) the usual case: no 64-bit division chain in front of the loads
    uint32_t e[OBS_ILP], col[OBS_ILP];
    int32_t p[OBS_ILP];
    bool on[OBS_ILP];
#pragma unroll
    for (int k = 0; k < OBS_ILP; ++k) {
        const uint64_t i = i0 + k * stride;
        on[k] = i < total;
        const uint64_t ic = on[k] ? i : 0;
        if (small) { e[k] = a.w_div.div((uint32_t)ic); col[k] = (uint32_t)ic - e[k] * a.W; }
        else { e[k] = (uint32_t)(ic / a.W); col[k] = (uint32_t)(ic % a.W); }
        p[k] = a.obs_idx[col[k] >= 4u ? col[k] - 4u : 0u];       // sparse then dense, heightmap_distribution.py:126-133
    }
    float sv[OBS_ILP], tx[OBS_ILP], ty[OBS_ILP], dv[OBS_ILP];
#pragma unroll
    for (int k = 0; k < OBS_ILP; ++k) {
        const uint64_t e3 = 3ull * e[k];
        const float* one = col[k] == 1u ? a.heading + e[k] : (col[k] == 2u ? a.lin_hist + e3 : a.ang_hist + e3);
        sv[k] = *one;
        tx[k] = a.target[e3] - a.pos[e3]; ty[k] = a.target[e3 + 1] - a.pos[e3 + 1];
        dv[k] = a.dist[(uint64_t)e[k] * a.R8 + 26u + (uint32_t)p[k]];
    }
#pragma unroll
    for (int k = 0; k < OBS_ILP; ++k) {
        float v;
        if (col[k] >= 4u) {
            v = dv[k] / 2.0f;
            if (a.fp16_div) v = (float)(_Float16)v;            // as shipped: `sparse / 2` is an fp16 division (rover.py:324-325)
        } else if (col[k] == 0u) {
            v = sqrtf(tx[k] * tx[k] + ty[k] * ty[k]) / 9.0f;   // :320
        } else if (col[k] == 1u) {
            v = sv[k] / 3.14159265358979323846f;               // :321
        } else {
            v = sv[k];                                         // :322 lin_hist, :323 ang_hist
        }
        if (on[k]) a.obs[(uint64_t)e[k] * a.obs_stride + col[k]] = v;
    }
}
__global__ void __launch_bounds__(256) assemble_obs_kernel(ObsArgs a) { assemble_obs_block(a, blockIdx.x, gridDim.x); }

// ---------------------------------------------------------------------------------------------------
// collision mask + reward + extras + done: one thread per env (rover.py:663-668, 460-531, 610-647)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void metrics_done_env(const MetricsArgs& a, uint32_t e, bool& done_flag) {
    // Every load of the env first, every store after: the compiler may not move a load above a store it cannot prove
    // disjoint, so loads placed where they are used made the thread wait for memory five or six times in a row (one env per
    // thread: 1 024 waves, nothing else to run meanwhile).
    const bool eval = a.eval_res != nullptr;                               // evaluation latch (rover.py:620-641,670-672)
    const bool need_progress = a.do_increment | a.do_metrics | a.do_done | eval;
    int64_t progress = need_progress ? a.progress[e] : 0;
    const int64_t code0 = eval ? a.eval_res[e] : 0;                         // once set, a code never changes
    int64_t code = code0;
    const bool cast = a.do_collision && a.curriculum_level >= 2;
    float4 dw[6];
    float2 db = make_float2(0.0f, 0.0f);
    if (cast) {                                                             // rows are 32-byte aligned (R8 is a multiple of 8)
        const float4* d4 = reinterpret_cast<const float4*>(a.dist + (uint64_t)e * a.R8);
#pragma unroll
        for (int r = 0; r < 6; ++r) dw[r] = d4[r];
        db = *reinterpret_cast<const float2*>(a.dist + (uint64_t)e * a.R8 + 24u);
    }
    const float px = a.pos[3ull * e], py = a.pos[3ull * e + 1];
    const float tx = a.target[3ull * e] - px, ty = a.target[3ull * e + 1] - py;
    int64_t coll = a.do_collision ? 0 : a.rock_collision[e];
    float hd = 0.0f, j0 = 0.0f, j1 = 0.0f, j2 = 0.0f, lin = 0.0f, lin_prev = 0.0f, ang = 0.0f, ang_prev = 0.0f;
    if (a.do_metrics) {
        hd = a.heading[e];
        const float* jn = a.joints + 13ull * e;
        j0 = jn[0]; j1 = jn[1]; j2 = jn[2];
        lin = a.lin_hist[3ull * e]; lin_prev = a.lin_hist[3ull * e + 1];
        ang = a.ang_hist[3ull * e]; ang_prev = a.ang_hist[3ull * e + 1];
    }
    float ep0 = 0.0f, ep1 = 0.0f;
    if (a.do_done) { ep0 = a.euler_pre[3ull * e]; ep1 = a.euler_pre[3ull * e + 1]; }
    // additional output (not in the reference's step): stone_info occupancy mask at the rover's position,
    // the clearance test of rover.py:536-539 through the stone-occupancy grid (a chain of dependent loads: started here)
    const bool stone = (a.do_collision && a.stone_collision) ? collides_grid(a.sgrid, a.info7, px, py, a.stone_margin) : false;

    if (a.do_increment) { progress += 1; a.progress[e] = progress; }       // rl_task.py:250
    if (a.do_collision) {                                                   // check_collision, rover.py:663-668
        if (cast) {
            float mw = dw[0].x;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                if (r) mw = (dw[r].x < mw) ? dw[r].x : mw;
                mw = (dw[r].y < mw) ? dw[r].y : mw;
                mw = (dw[r].z < mw) ? dw[r].z : mw;
                mw = (dw[r].w < mw) ? dw[r].w : mw;
            }
            float mb = (db.y < db.x) ? db.y : db.x;
            coll = (fabsf(mw) < a.wheel_thr) ? 1 : 0;            // 0.8 / 0.45, as fp16 values in the as-shipped mode
            if (fabsf(mb) < a.body_thr) coll = 1;
        }
        a.rock_collision[e] = coll;
        if (a.stone_collision) a.stone_collision[e] = stone ? 1 : 0;
        if (eval && cast && code == 0) code = coll;                         // :670-672 (check_collision runs at level >= 2 only)
    }
    float td = sqrtf(tx * tx + ty * ty);                                    // :482 / :617
    if (a.do_metrics) {
        float heading_pen = ((lin < 0.0f) ? -1.0f : 0.0f) * a.heading_contraint_reward;           // :486
        float boogie = (fabsf(j0) + fabsf(j1) + fabsf(j2)) * a.boogie_contraint_reward;       // :492
        float goal_pen = (fabsf(hd) > 2.0f) ? -fabsf(hd * 0.3f * a.goal_angle_reward) : 0.0f;      // :495
        float dl = fabsf(lin * 3.0f - 3.0f * lin_prev), da = fabsf(ang * 3.0f - 3.0f * ang_prev);
        float p1 = (dl > 0.05f) ? dl * dl : 0.0f;                                                  // :498
        float p2 = (da > 0.05f) ? da * da : 0.0f;                                                  // :499
        float motion = (p1 * p1) * a.motion_contraint_reward;                                      // :500
        motion = motion + (p2 * p2) * a.motion_contraint_reward;                                   // :502
        float pos_rew = (1.0f / (1.0f + ((float)(0.33 * 0.33) * td) * td)) * a.pos_reward;         // :505
        if (td <= 0.18f) pos_rew = 1.03f * (float)((int64_t)a.max_episode_length - progress);      // :506
        float reward = pos_rew + heading_pen + motion + goal_pen;                                  // :512
        int64_t tracker = 0;
        if (a.curriculum_level >= 2 && coll == 1) { tracker = a.num_envs_global; reward = reward - 300.0f; }  // :517-519
        reward = reward / 3000.0f;                                                                 // :522
        a.rew[e] = reward;
        if (a.ex_pos_reward) a.ex_pos_reward[e] = pos_rew;
        if (a.ex_collision) a.ex_collision[e] = tracker;
        if (a.ex_upright) a.ex_upright[e] = boogie;
        if (a.ex_heading) a.ex_heading[e] = heading_pen;
        if (a.ex_motion) a.ex_motion[e] = motion;
        if (a.ex_goal_angle) a.ex_goal_angle[e] = goal_pen;
        if (a.ex_lin) a.ex_lin[e] = lin;
        if (a.ex_ang) a.ex_ang[e] = ang;
    }
    if (a.do_done) {                                                        // is_done, rover.py:610-647
        const float tilt = (float)(0.78 * 1.5);
        int64_t reset = (progress >= (int64_t)a.max_episode_length) ? 1 : 0;
        if (fabsf(ep0) >= tilt) reset = 1;
        if (fabsf(ep1) >= tilt) reset = 1;
        if (td >= 11.0f) reset = 1;
        if (td <= 0.18f) reset = 1;
        if (a.curriculum_level >= 2 && coll == 1) reset = 1;
        a.reset[e] = reset;
        if (a.done_u8) a.done_u8[e] = (uint8_t)reset;
        done_flag = reset != 0;
        if (eval) {                                                         // :620-631, each only while the code is still 0
            if (code == 0 && td >= 9.5f) code = 1;                          // out of area counts as a collision (no reset below 11)
            if (code == 0 && td <= 0.18f) code = 2;                         // reached the goal
            if (code == 0 && progress >= (int64_t)a.max_episode_length) code = 3;   // timed out
        }
    }
    if (eval && code != code0) { a.eval_res[e] = code; a.eval_step[e] = progress; }
}

__device__ __forceinline__ void metrics_done_block(const MetricsArgs& a, uint32_t bid) {
    uint32_t e = bid * 256u + threadIdx.x;
    bool done_flag = false;
    if (e < a.E) metrics_done_env(a, e, done_flag);
    if (a.block_cnt) block_count_flags(done_flag, a.block_cnt, bid);      // per-block done count for the compaction
}
__global__ void __launch_bounds__(256) metrics_done_kernel(MetricsArgs a) { metrics_done_block(a, blockIdx.x); }

// rover_step: both consumers of the ray distances in ONE launch — the first n_met workgroups are metrics_done_kernel's (one env per
// thread, a long chain of dependent loads: they start first), the rest assemble_obs_kernel's.  Neither reads what the other
// writes; side by side the 9 us of the metrics pass hide behind the obs pass instead of following it.
__global__ void __launch_bounds__(256) obs_metrics_kernel(ObsArgs o, MetricsArgs m, uint32_t n_met) {
    if (blockIdx.x < n_met) metrics_done_block(m, blockIdx.x);
    else assemble_obs_block(o, blockIdx.x - n_met, gridDim.x - n_met);
}

// ---------------------------------------------------------------------------------------------------
// done compaction: nonzero(reset_buf) ascending, no host sync.  Two passes over 256-env blocks:
//   count  (fused into metrics_done_kernel, or compact_count_kernel for the stand-alone call): per-block popcount
//   write  each block sums the counts of the blocks before it, ranks its own flags with ballot + popcount
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) compact_count_kernel(const int64_t* __restrict__ reset, uint32_t n,
                                                            uint32_t* __restrict__ block_cnt) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    block_count_flags((i < n) && (reset[i] != 0), block_cnt, blockIdx.x);
}

__global__ void __launch_bounds__(256) compact_write_kernel(const int64_t* __restrict__ reset, uint32_t n, int64_t offset,
                                                            const uint32_t* __restrict__ block_cnt, int64_t* __restrict__ ids,
                                                            int32_t* __restrict__ count) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t wcnt[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    // exclusive prefix of the preceding blocks' counts (<= a few thousand values: one strided pass)
    uint32_t part = 0;
    for (uint32_t b = tid; b < blockIdx.x; b += 256u) part += block_cnt[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    uint32_t i = blockIdx.x * 256u + tid;
    bool flag = (i < n) && (reset[i] != 0);
    unsigned long long ballot = __ballot(flag);
    if (lane == 0u) { wsum[w] = part; wcnt[w] = __popcll(ballot); }
    __syncthreads();
    uint32_t base = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    uint32_t woff = 0;
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) woff += (v < w) ? wcnt[v] : 0u;
    if (flag) ids[base + woff + __popcll(ballot & ((1ull << lane) - 1ull))] = offset + (int64_t)i;
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *count = (int32_t)(base + wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
}

// ---------------------------------------------------------------------------------------------------
// evaluation bookkeeping (rover_eval_read / rover_eval_clear): summary = [count of codes 0..3 | sum of eval_step over codes 0..3]
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) eval_summary_kernel(const int64_t* __restrict__ eval_res, const int64_t* __restrict__ eval_step,
                                                           uint32_t E, unsigned long long* __restrict__ summary8) {
    __shared__ unsigned long long part[8];
    if (threadIdx.x < 8u) part[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long cnt[4] = {0ull, 0ull, 0ull, 0ull}, sum[4] = {0ull, 0ull, 0ull, 0ull};
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < E; e += gridDim.x * 256u) {
        const int64_t c = eval_res[e];
        const unsigned long long st = (unsigned long long)eval_step[e];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cnt[k] += (c == k) ? 1ull : 0ull;
            sum[k] += (c == k) ? st : 0ull;
        }
    }
    // integer sums (two's complement, mod 2^64): exact and independent of the order of the atomics
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt[k] += __shfl_xor(cnt[k], off, 64);
            sum[k] += __shfl_xor(sum[k], off, 64);
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { atomicAdd(&part[k], cnt[k]); atomicAdd(&part[4 + k], sum[k]); }
    }
    __syncthreads();
    if (threadIdx.x < 8u) atomicAdd(&summary8[threadIdx.x], part[threadIdx.x]);
}

__global__ void __launch_bounds__(256) eval_clear_kernel(int64_t* __restrict__ eval_res, int64_t* __restrict__ eval_step, uint32_t E,
                                                         const int64_t* __restrict__ ids, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int64_t e = ids ? ids[i] : (int64_t)i;
    if (e < 0 || e >= (int64_t)E) return;                                   // (the host validated the ids; never write outside)
    eval_res[e] = 0;
    eval_step[e] = 0;
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t launch_assemble_obs(const ObsArgs& a_in, hipStream_t s) {
    ObsArgs a = a_in;
    a.w_div = make_fastdiv(a.W);
    hipLaunchKernelGGL(assemble_obs_kernel, dim3(blocks_for((uint64_t)a.E * a.W, 256 * OBS_ILP)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_obs_metrics(const ObsArgs& o_in, const MetricsArgs& m, hipStream_t s) {
    ObsArgs o = o_in;
    o.w_div = make_fastdiv(o.W);
    const uint32_t n_met = blocks_for(m.E, 256), n_obs = blocks_for((uint64_t)o.E * o.W, 256 * OBS_ILP);
    hipLaunchKernelGGL(obs_metrics_kernel, dim3(n_met + n_obs), dim3(256), 0, s, o, m, n_met);
    return hipGetLastError();
}

hipError_t launch_metrics_done(const MetricsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(metrics_done_kernel, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_compact(const int64_t* reset, uint32_t n, int64_t offset, uint32_t* block_cnt, bool counted, int64_t* ids,
                          int32_t* count, hipStream_t s) {
    const uint32_t nb = blocks_for(n, 256);
    if (!counted) hipLaunchKernelGGL(compact_count_kernel, dim3(nb), dim3(256), 0, s, reset, n, block_cnt);
    hipLaunchKernelGGL(compact_write_kernel, dim3(nb), dim3(256), 0, s, reset, n, offset, block_cnt, ids, count);
    return hipGetLastError();
}

hipError_t launch_eval_summary(const int64_t* eval_res, const int64_t* eval_step, uint32_t E, int64_t* summary8, hipStream_t s) {
    hipError_t err = hipMemsetAsync(summary8, 0, 8 * sizeof(int64_t), s);
    if (err != hipSuccess) return err;
    uint32_t nb = blocks_for(E, 256);
    if (nb > 1024u) nb = 1024u;                                             // grid-stride: at most 1 024 x 8 atomics on the result
    hipLaunchKernelGGL(eval_summary_kernel, dim3(nb), dim3(256), 0, s, eval_res, eval_step, E,
                       reinterpret_cast<unsigned long long*>(summary8));
    return hipGetLastError();
}

hipError_t launch_eval_clear(int64_t* eval_res, int64_t* eval_step, uint32_t E, const int64_t* ids, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(eval_clear_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, eval_res, eval_step, E, ids, n);
    return hipGetLastError();
}

}  // namespace rover
