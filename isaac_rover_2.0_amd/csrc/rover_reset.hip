// rover_reset.hip — the reset path and the action side: clearance, spawn shift, height samples, goal draws, reset_idx, pre_physics_step,
// Ackermann, quat -> euler (gfx950, wave64).
//
// Reference (pure PyTorch; paths relative to omniisaacgymenvs/):
//   tasks/rover.py:338-453 pre_physics_step, reset_idx, :533-608 goals, clearance, heights, :649-661 avoid_pos_rock_collision
//   tasks/utils/kinematics.py:13-67
//   tasks/utils/math/tensor_quat_to_euler.py:6-31
// Built with -ffp-contract=off: see rover_rays.hip.
// Kernels:
//   clearance / shift_spawns / sample_height / goals_draw / goals_env0 / reset_envs kernels                          (A9, f-2)
//   pre_physics / ackermann / quat_to_euler kernels                                                                  (f-1)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"
#include "rover_philox.h"
#include "rover_height.h"      // cell_coord, height_at
#include "rover_pose.h"        // quat_to_euler
#include "rover_stones.h"

namespace rover {

__global__ void __launch_bounds__(256) quat_to_euler_kernel(const float* __restrict__ q, float* __restrict__ eul, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r, p, y;
    quat_to_euler(q + 4ull * i, r, p, y);
    eul[3ull * i] = r; eul[3ull * i + 1] = p; eul[3ull * i + 2] = y;
}

__global__ void __launch_bounds__(256) clearance_kernel(const float* __restrict__ info7, uint32_t S, const float* __restrict__ xy,
                                                        uint32_t n, float* __restrict__ out) {
    __shared__ float sx[STONE_TILE], sy[STONE_TILE], sr[STONE_TILE];
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool live = i < n;
    float x = live ? xy[2ull * i] : 0.0f, y = live ? xy[2ull * i + 1] : 0.0f;
    float c = clearance_tiles(info7, S, x, y, live, sx, sy, sr);
    if (live) out[i] = c;
}

// avoid_pos_rock_collision rover.py:649-661: per env, x += 0.05 while the stone clearance is <= 1.4.  (The reference
// iterates over all envs until nothing moves; per env that is this loop.)
__global__ void __launch_bounds__(256) shift_spawns_kernel(StoneGridDev g, const float* __restrict__ info7, float* __restrict__ pos3,
                                                           uint32_t n, int32_t max_iter) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = pos3[3ull * i], y = pos3[3ull * i + 1];
    for (int32_t it = 0; it < max_iter && collides_grid(g, info7, x, y, 1.4f); ++it) x = x + 0.05f;   // :660
    pos3[3ull * i] = x;
}

// get_pos_height rover.py:588-608
__global__ void __launch_bounds__(256) sample_height_kernel(HeightDev h, const float* __restrict__ xy, uint32_t n,
                                                            float* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t ix = cell_coord(xy[2ull * i], h.shift_x, h.hscale, h.inv_hscale, h.rcp, h.N0);
    uint32_t iy = cell_coord(xy[2ull * i + 1], h.shift_y, h.hscale, h.inv_hscale, h.rcp, h.N0);
    if (iy > (uint32_t)(h.N1 - 1)) iy = (uint32_t)(h.N1 - 1);
    out[i] = h.hm[(uint64_t)ix * h.N1 + iy] * h.vscale;
}

// Philox4x32-10 (Salmon et al. 2011), used when the caller supplies no uniforms
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint32_t draw, uint32_t idx) {
    uint32_t c[4] = {idx, draw, 0u, 0u};                                   // word 3 = 0: the policy's action noise uses 0x50000000 | pair
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(c[0] >> 8) * (1.0f / 16777216.0f);                      // [0,1) with 24 bits, like torch.rand f32
}

// generate_goals rover.py:544-549 (+ random_goals :554-564, check_goal_collision :533-542, goal z :581-583).
//
// The reference loops globally: draw goals for every listed env, test them against the stone list, and — the
// env_ids = mask*env_ids aliasing of :540 — turn the id of every ACCEPTED entry into 0, so accepted entries keep
// re-randomising env 0's goal and the loop also waits for env 0's goal to be clear.  Unrolled per entry this is:
//   * entry i keeps its own first clear draw u[t_i][i] (later iterations no longer write its env);
//   * the loop ends at the first iteration T >= max_i t_i at which env 0's goal — written by the LAST zero-id entry
//     of that iteration ("last writer wins", what a sequential index_put gives) — is clear, or at max_i t_i when no
//     zero-id entry exists yet.
// goals_draw_kernel does the per-entry part in parallel over all workgroups (stones staged through LDS tiles);
// goals_env0_kernel replays env 0's part on one workgroup.  Same draws, same results as the sequential loop
// (oracle_generate_goals); n may come from device memory so no host sync is needed.
__device__ __forceinline__ void goal_from_draw(float u, float radius, const float* __restrict__ initial_pos3, int64_t id,
                                               float& x, float& y) {
    float alpha = (float)(2 * 3.14159265358979323846) * u;                  // :556
    float gx = radius * cosf(alpha) + 0.0f, gy = radius * sinf(alpha) + 0.0f;   // :560-561
    x = gx + initial_pos3[3ull * id];                                       // :563-564
    y = gy + initial_pos3[3ull * id + 1];
}

// GOAL_LANES lanes share one entry and test GOAL_LANES consecutive draws at once (the first clear one wins, exactly what the
// sequential loop finds): with dense stones most draws collide and the per-entry chain of draw -> grid lookup was the cost.
#define GOAL_LANES 8u

__global__ void __launch_bounds__(256) goals_draw_kernel(GoalArgs a) {
    const uint32_t n = a.n_dev ? (uint32_t)max(*a.n_dev, 0) : a.n_host;
    const uint32_t gt = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = gt / GOAL_LANES, j = gt % GOAL_LANES;
    const uint32_t shift = (threadIdx.x & 63u) & ~(GOAL_LANES - 1u);             // first lane of this entry's group
    const bool live = i < n;
    const int64_t id = live ? a.env_ids[i] - a.id_offset : 0;
    if (live && id == 0 && j == 0) a.t_acc[i] = -1;                            // zero-id entry from the start
    bool active = live && id != 0;
    // whole waves iterate together (ballot); finished / idle groups just stop contributing
    for (int32_t t0 = 0; t0 < a.max_draws; t0 += (int32_t)GOAL_LANES) {
        if (__builtin_amdgcn_ballot_w64(active) == 0) break;
        const int32_t t = t0 + (int32_t)j;
        bool clear = false;
        float x = 0.0f, y = 0.0f;
        if (active && t < a.max_draws) {
            // library RNG: keyed by the entry's GLOBAL env id, so that the shards of a multi-GPU run draw different streams
            float u = a.draws ? a.draws[(uint64_t)t * n + i] : philox_uniform(a.seed + (a.seed_dev ? *a.seed_dev : 0ull), (uint32_t)t, (uint32_t)a.env_ids[i]);
            goal_from_draw(u, a.radius, a.initial_pos3, id, x, y);
            clear = !collides_grid(a.grid, a.info7, x, y, 1.0f);               // :539: redraw while nearest_rock <= 1.0
        }
        const uint32_t m = (uint32_t)(__builtin_amdgcn_ballot_w64(clear) >> shift) & ((1u << GOAL_LANES) - 1u);
        if (active) {
            const bool last_trip = t0 + (int32_t)GOAL_LANES >= a.max_draws;
            int32_t winner = -1;                                               // lane of the group whose draw is kept
            if (m) winner = (int32_t)__builtin_ctz(m);
            else if (last_trip) winner = a.max_draws - 1 - t0;                 // never clear: the last draw stays (t_acc = max)
            if (winner >= 0) {
                if ((int32_t)j == winner) {
                    a.t_acc[i] = m ? t : a.max_draws;
                    a.target3[3ull * id] = x; a.target3[3ull * id + 1] = y;
                    a.target3[3ull * id + 2] = height_at(a.h, x, y);            // set_targets :581-583
                }
                active = false;
            }
        }
    }
}

__global__ void __launch_bounds__(1024) goals_env0_kernel(GoalArgs a) {
    __shared__ int s_tmax, s_lz, s_has_zero, s_fail;
    const uint32_t tid = threadIdx.x;
    const uint32_t n = a.n_dev ? (uint32_t)max(*a.n_dev, 0) : a.n_host;
    if (n == 0) { if (tid == 0 && a.n_draws_used) *a.n_draws_used = 0; return; }
    if (tid == 0) { s_tmax = -1; s_lz = -1; s_has_zero = 0; s_fail = 0; }
    __syncthreads();
    // per-thread partial results, one wave reduction, one LDS atomic per wave (n can be all 65 536 envs)
    int my_tmax = -1;
    bool my_zero = false, my_fail = false;
    for (uint32_t i = tid; i < n; i += blockDim.x) {
        int32_t t = a.t_acc[i];
        if (t >= a.max_draws) my_fail = true;
        else if (t < 0) my_zero = true;
        else my_tmax = max(my_tmax, t);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) my_tmax = max(my_tmax, __shfl_xor(my_tmax, o));
    const bool w_zero = __builtin_amdgcn_ballot_w64(my_zero) != 0, w_fail = __builtin_amdgcn_ballot_w64(my_fail) != 0;
    if ((tid & 63u) == 0u) {
        if (my_tmax >= 0) atomicMax(&s_tmax, my_tmax);
        if (w_zero) s_has_zero = 1;
        if (w_fail) s_fail = 1;
    }
    __syncthreads();
    if (s_fail) { if (tid == 0 && a.n_draws_used) *a.n_draws_used = -1; return; }
    const int tmax = s_tmax;                          // -1 when every entry was a zero-id entry
    // zero-id set before the draw of iteration max(tmax, 0): original zeros and entries accepted earlier
    int my_lz = -1;
    for (uint32_t i = tid; i < n; i += blockDim.x) {
        int32_t t = a.t_acc[i];
        if (t < 0 || t < tmax) my_lz = max(my_lz, (int)i);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) my_lz = max(my_lz, __shfl_xor(my_lz, o));
    if ((tid & 63u) == 0u && my_lz >= 0) atomicMax(&s_lz, my_lz);
    __syncthreads();
    if (tid >= 64u) return;
    // env 0's own sequence, 64 iterations per trip on one wave: iteration t0 is written by entry lz, every later one by
    // entry n - 1 (from iteration tmax + 1 on every entry has id 0); the first clear draw ends the loop.
    const int32_t t0 = max(tmax, 0);
    const int lz0 = s_lz;
    int32_t used = -1;
    float x = 0.0f, y = 0.0f;
    bool wrote = false;
    if (lz0 < 0) {
        used = t0 + 1;                                // nobody writes env 0 in this iteration: bad == 0
    } else {
        for (int32_t base = t0; base < a.max_draws; base += 64) {
            const int32_t t = base + (int32_t)tid;
            const uint32_t src = (t == t0) ? (uint32_t)lz0 : n - 1u;
            bool clear = false;
            float cx = 0.0f, cy = 0.0f;
            if (t < a.max_draws) {
                float u = a.draws ? a.draws[(uint64_t)t * n + src] : philox_uniform(a.seed + (a.seed_dev ? *a.seed_dev : 0ull), (uint32_t)t, (uint32_t)a.env_ids[src]);
                goal_from_draw(u, a.radius, a.initial_pos3, 0, cx, cy);
                clear = !collides_grid(a.grid, a.info7, cx, cy, 1.0f);
            }
            const uint64_t m = __builtin_amdgcn_ballot_w64(clear);
            const bool last_trip = base + 64 >= a.max_draws;
            int32_t winner = -1;
            if (m) winner = (int32_t)__builtin_ctzll(m);
            else if (last_trip) winner = a.max_draws - 1 - base;
            if (winner >= 0) {
                x = __shfl(cx, winner); y = __shfl(cy, winner);
                wrote = true;
                if (m) used = base + winner + 1;
                break;
            }
        }
    }
    if (tid != 0) return;
    if (wrote) {
        a.target3[0] = x; a.target3[1] = y;
        if (s_has_zero) a.target3[2] = height_at(a.h, x, y);               // env 0 was listed: set_targets :581-583
    }
    if (a.n_draws_used) *a.n_draws_used = used;
}

// reset_idx rover.py:416-453 for the compacted reset ids, count read from device memory (no host sync).
// Orientation: the reference feeds scipy's (x,y,z,w) of a rotation about x to Isaac as (w,x,y,z) (:429-431,:449),
// i.e. w = sin(d/2), z = cos(d/2) with d = randint(0, 360) degrees.  yaw_deg (optional) replaces the draw.
__global__ void __launch_bounds__(256) reset_envs_kernel(ResetArgs a) {
    const uint32_t n = a.n_dev ? (uint32_t)max(*a.n_dev, 0) : a.n_host;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = a.ids[i] - a.id_offset;
    float deg = a.yaw_deg ? (float)a.yaw_deg[i]
                          : floorf(philox_uniform((a.seed + (a.seed_dev ? *a.seed_dev : 0ull)) ^ 0x9E3779B97F4A7C15ull, 0u, (uint32_t)a.ids[i]) * 361.0f);   // global id
    float half = (deg * (3.14159265358979323846f / 180.0f)) / 2.0f;
    a.quat4[4ull * id] = sinf(half); a.quat4[4ull * id + 1] = 0.0f; a.quat4[4ull * id + 2] = 0.0f; a.quat4[4ull * id + 3] = cosf(half);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = a.initial_pos3[3ull * id + c];
        a.pos3[3ull * id + c] = v;
        if (a.base_pos3) a.base_pos3[3ull * id + c] = v;
    }
    for (int j = 0; j < 13; ++j) {
        if (a.joint_pos13) a.joint_pos13[13ull * id + j] = 0.0f;
        if (a.joint_vel13) a.joint_vel13[13ull * id + j] = 0.0f;
    }
    a.reset[id] = 0;                                                        // :452-453
    a.progress[id] = 0;
}

// pre_physics_step rover.py:338-414 without the reset branch: pre-physics euler (:343), Memory.input_state x2
// (:379-380), Ackermann (:391) and the scatter into the joint-target layout (:400-414, rover_view.py:45-46).
__global__ void __launch_bounds__(256) pre_physics_kernel(PrePhysicsArgs a) {
    uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    if (a.euler_pre) {
        float r, p, y;
        quat_to_euler(a.quat + 4ull * e, r, p, y);
        a.euler_pre[3ull * e] = r; a.euler_pre[3ull * e + 1] = p; a.euler_pre[3ull * e + 2] = y;
    }
    float lin = a.actions[2ull * e], ang = a.actions[2ull * e + 1];
    float l0 = a.lin_hist[3ull * e], l1 = a.lin_hist[3ull * e + 1];
    a.lin_hist[3ull * e] = lin; a.lin_hist[3ull * e + 1] = l0; a.lin_hist[3ull * e + 2] = l1;
    float g0 = a.ang_hist[3ull * e], g1 = a.ang_hist[3ull * e + 1];
    a.ang_hist[3ull * e] = ang; a.ang_hist[3ull * e + 1] = g0; a.ang_hist[3ull * e + 2] = g1;
    if (a.actions_nn) {                         // rover.py:366: cat((actions[:, :, None], actions_nn), 2)[:, :, 0:3]
        float* n = a.actions_nn + 6ull * e;
        const float n0 = n[0], n1 = n[1], n3 = n[3], n4 = n[4];
        n[0] = lin; n[1] = n0; n[2] = n1; n[3] = ang; n[4] = n3; n[5] = n4;
    }
    if (!a.pos_targets13 && !a.vel_targets13) return;
    // Ackermann, tasks/utils/kinematics.py:13-67 (same operation order as ackermann_kernel)
    const float wl[6][2] = {{-0.385, 0.438}, {0.385, 0.438}, {-0.447, 0.0}, {0.447, 0.0}, {-0.385, -0.411}, {0.385, -0.411}};
    const float side[6] = {-1.0f, 1.0f, -1.0f, 1.0f, -1.0f, 1.0f};
    float Px = copysignf(lin / ang, -ang);
    Px = (fabsf(Px) > 0.45f) ? Px : 0.0f;
    lin = (Px != 0.0f) ? lin : 0.0f;
    float steer[6], vel[6];
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        float dx = Px - wl[w][0], dy = 0.0f - wl[w][1];
        float dist = sqrtf(dx * dx + dy * dy);
        float av = (lin != 0.0f) ? copysignf(ang, lin) : ang * side[w];
        float mv = dist * av;
        if (dist > 1000.0f) mv = lin;
        vel[w] = mv / 0.2f;
        float sa = atan2f(wl[w][1], wl[w][0] - Px);
        if (sa < (float)(-3.14 / 2)) sa = sa + 3.14159265358979323846f;
        if (sa > (float)(3.14 / 2)) sa = sa - 3.14159265358979323846f;
        steer[w] = sa;
    }
    if (a.pos_targets13) {                      // positions [FR, RR, FL, RL] = steer[1,5,0,4] -> joints [6,8,4,7]
        float* p = a.pos_targets13 + 13ull * e;
        p[6] = steer[1]; p[8] = steer[5]; p[4] = steer[0]; p[7] = steer[4];
    }
    if (a.vel_targets13) {                      // velocities [FR,CR,RR,FL,CL,RL] = vel[1,3,5,0,2,4] -> joints [10,5,12,9,3,11]
        float* v = a.vel_targets13 + 13ull * e;
        v[10] = vel[1]; v[5] = vel[3]; v[12] = vel[5]; v[9] = vel[0]; v[3] = vel[2]; v[11] = vel[4];
    }
}

// Ackermann, tasks/utils/kinematics.py:13-67
__global__ void __launch_bounds__(256) ackermann_kernel(const float* __restrict__ lin_in, const float* __restrict__ ang_in,
                                                        uint32_t n, float* __restrict__ steer, float* __restrict__ vel) {
    const float wl[6][2] = {{-0.385, 0.438}, {0.385, 0.438}, {-0.447, 0.0}, {0.447, 0.0}, {-0.385, -0.411}, {0.385, -0.411}};
    const float side[6] = {-1.0f, 1.0f, -1.0f, 1.0f, -1.0f, 1.0f};
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float lin = lin_in[i], ang = ang_in[i];
    float Px = copysignf(lin / ang, -ang);
    Px = (fabsf(Px) > 0.45f) ? Px : 0.0f;
    lin = (Px != 0.0f) ? lin : 0.0f;
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        float dx = Px - wl[w][0], dy = 0.0f - wl[w][1];
        float dist = sqrtf(dx * dx + dy * dy);
        float av = (lin != 0.0f) ? copysignf(ang, lin) : ang * side[w];
        float mv = dist * av;
        if (dist > 1000.0f) mv = lin;
        vel[6ull * i + w] = mv / 0.2f;
        float sa = atan2f(wl[w][1], wl[w][0] - Px);
        if (sa < (float)(-3.14 / 2)) sa = sa + 3.14159265358979323846f;
        if (sa > (float)(3.14 / 2)) sa = sa - 3.14159265358979323846f;
        steer[6ull * i + w] = sa;
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t launch_quat_to_euler(const float* q, float* eul, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(quat_to_euler_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, q, eul, n);
    return hipGetLastError();
}

hipError_t launch_clearance(const float* info7, uint32_t S, const float* xy, uint32_t n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(clearance_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, info7, S, xy, n, out);
    return hipGetLastError();
}

hipError_t launch_shift_spawns(const StoneGridDev& g, const float* info7, float* pos3, uint32_t n, int32_t max_iter, hipStream_t s) {
    hipLaunchKernelGGL(shift_spawns_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, g, info7, pos3, n, max_iter);
    return hipGetLastError();
}

hipError_t launch_sample_height(const HeightDev& h, const float* xy, uint32_t n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(sample_height_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, h, xy, n, out);
    return hipGetLastError();
}

hipError_t launch_generate_goals(const GoalArgs& a, uint32_t n_max, hipStream_t s) {
    hipLaunchKernelGGL(goals_draw_kernel, dim3(blocks_for((uint64_t)n_max * GOAL_LANES, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(goals_env0_kernel, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_reset_envs(const ResetArgs& a, uint32_t n_max, hipStream_t s) {
    hipLaunchKernelGGL(reset_envs_kernel, dim3(blocks_for(n_max, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pre_physics(const PrePhysicsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pre_physics_kernel, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ackermann(const float* lin, const float* ang, uint32_t n, float* steer, float* vel, hipStream_t s) {
    hipLaunchKernelGGL(ackermann_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, lin, ang, n, steer, vel);
    return hipGetLastError();
}

}  // namespace rover
