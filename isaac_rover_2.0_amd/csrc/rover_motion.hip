// rover_motion.hip — the terrain-following motion model (rover_motion_step; the definition is written out in include/rover_step.h and
// DESIGN.md §4.16): a deterministic, stateless, kinematic pose feeder that keeps the six wheels on the heightfield.
//
// One launch per control step, one thread per env.  Per sub-step a thread turns its commands into a body twist (turn on the spot as
// kinematics.py:34-39), integrates yaw and position, reads the terrain height under the six wheel contacts through height_at — six
// independent gathers, all issued before the first is used —, fits the plane z = z_c + p a + q b through them with the constant 3 x 6
// pseudo-inverse of the wheel layout and writes the ZYX pose whose body x and y axes lie in that plane.  The pose stays in registers
// across sub-steps; nothing is shared between threads: no LDS, no atomics.  After the last sub-step the block copies its envs' rows of
// the joint targets into the joint state (ideal actuators), as one contiguous range.
//
// Built with -ffp-contract=off: every written f32 operation is one IEEE rounding, in the written order (tests/motion_ref.py restates it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"
#include "rover_height.h"

namespace rover {

// (z_c, p, q) = C z with C = pinv(A), A = [1, a_i, b_i] (6 x 3), a_i = f_i (forward), b_i = -r_i (left): C = (A^T A)^-1 A^T in double
// (A has full rank, condition number 2.9), each entry rounded to f32 once.
void motion_plane_fit(float out[3][MOTION_WHEELS]) {
    const double wl[MOTION_WHEELS][2] = {{-0.385, 0.438}, {0.385, 0.438}, {-0.447, 0.0}, {0.447, 0.0}, {-0.385, -0.411}, {0.385, -0.411}};   // (right, forward): kinematics.py:20-25
    double A[MOTION_WHEELS][3], G[3][3] = {}, inv[3][3];
    for (int i = 0; i < MOTION_WHEELS; ++i) { A[i][0] = 1.0; A[i][1] = wl[i][1]; A[i][2] = -wl[i][0]; }
    for (int i = 0; i < MOTION_WHEELS; ++i)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) G[r][c] += A[i][r] * A[i][c];
    const double det = G[0][0] * (G[1][1] * G[2][2] - G[1][2] * G[2][1]) - G[0][1] * (G[1][0] * G[2][2] - G[1][2] * G[2][0]) +
                       G[0][2] * (G[1][0] * G[2][1] - G[1][1] * G[2][0]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {          // the adjugate's entry (r, c) is the cofactor of (c, r); indices taken cyclically carry the sign
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            inv[r][c] = (G[r1][c1] * G[r2][c2] - G[r1][c2] * G[r2][c1]) / det;
        }
    for (int r = 0; r < 3; ++r)
        for (int i = 0; i < MOTION_WHEELS; ++i) out[r][i] = (float)(inv[r][0] * A[i][0] + inv[r][1] * A[i][1] + inv[r][2] * A[i][2]);
}

struct MotionKernelArgs {
    MotionArgs m;
    int32_t quat_vec, joint_vec;           // 16-byte loads and stores of the quaternion rows / of the joint copy (the bases are aligned)
};

// dst[0 .. n) = src[0 .. n): the block's share is the 256 * 13 floats of its own envs' rows, contiguous in both arrays
__device__ __forceinline__ void copy_joint_rows(const float* __restrict__ src, float* __restrict__ dst, uint64_t n, bool vec) {
    const uint64_t per_block = 256ull * 13ull;
    const uint64_t first = (uint64_t)blockIdx.x * per_block;
    const uint64_t last = (first + per_block < n) ? first + per_block : n;
    if (vec) {                                 // per_block is a multiple of 4: the block's range starts on a 16-byte boundary
        const uint64_t last4 = first + ((last - first) & ~3ull);
        for (uint64_t i = first + 4ull * threadIdx.x; i < last4; i += 4ull * 256ull)
            *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
        const uint64_t i = last4 + threadIdx.x;
        if (i < last) dst[i] = src[i];
    } else {
        for (uint64_t i = first + threadIdx.x; i < last; i += 256ull) dst[i] = src[i];
    }
}

// RCP: the heightfield's cell_index_mode as a compile-time value — cell_coord's choice between the division and the reciprocal is
// then no branch, the six lookups of a sub-step stand in one basic block and their loads are issued back to back
template <int RCP>
__global__ void __launch_bounds__(256) rover_motion_kernel(MotionKernelArgs k) {
    const MotionArgs& a = k.m;
    HeightDev hf = a.h;
    hf.rcp = RCP;
    const float wl[MOTION_WHEELS][2] = {{-0.385, 0.438}, {0.385, 0.438}, {-0.447, 0.0}, {0.447, 0.0}, {-0.385, -0.411}, {0.385, -0.411}};
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e < a.E) {
        float* pp = a.pos3 + 3ull * e;
        float* qp = a.quat4 + 4ull * e;
        float px = pp[0], py = pp[1], pz = pp[2];
        float qw, qx, qy, qz;
        if (k.quat_vec) {
            const float4 q = *reinterpret_cast<const float4*>(qp);
            qw = q.x; qx = q.y; qy = q.z; qz = q.w;
        } else {
            qw = qp[0]; qx = qp[1]; qy = qp[2]; qz = qp[3];
        }
        // 1. commands; turn on the spot where the turning point lies between the wheels (v / 0 = +-inf keeps v, 0 / 0 = NaN gives 0)
        const float v = a.lin[(uint64_t)e * (uint32_t)a.cmd_stride] * a.max_lin;
        const float w = a.ang[(uint64_t)e * (uint32_t)a.cmd_stride] * a.max_ang;
        const float v_eff = (fabsf(v / w) > 0.45f) ? v : 0.0f;
        const float dyaw = w * a.dt;
        for (int32_t s = 0; s < a.substeps; ++s) {
            // 2. heading: the yaw of tensor_quat_to_eul (tensor_quat_to_euler.py:27-29), valid for a tilted body
            const float yaw0 = atan2f(2.0f * (qw * qz + qx * qy), 1.0f - (2.0f * (qy * qy + qz * qz)));
            const float yaw = yaw0 + dyaw;
            const float cs = cosf(yaw), sn = sinf(yaw);
            // 3. position
            px = px + (v_eff * cs) * a.dt;
            py = py + (v_eff * sn) * a.dt;
            // 4. the six wheel contacts: every lookup is issued before the first one is used
            float z[MOTION_WHEELS];
#pragma unroll
            for (int i = 0; i < MOTION_WHEELS; ++i) {
                const float r = wl[i][0], f = wl[i][1];
                const float wx = (px + f * cs) + r * sn;
                const float wy = (py + f * sn) - r * cs;
                z[i] = height_at(hf, wx, wy);
            }
            // 5. plane fit
            float zc = a.fit[0][0] * z[0], p = a.fit[1][0] * z[0], q = a.fit[2][0] * z[0];
#pragma unroll
            for (int i = 1; i < MOTION_WHEELS; ++i) {
                zc = zc + a.fit[0][i] * z[i];
                p = p + a.fit[1][i] * z[i];
                q = q + a.fit[2][i] * z[i];
            }
            // 6. orientation: ZYX euler (roll, pitch, yaw) -> quaternion
            const float pitch = -atanf(p);
            const float roll = atanf(q * cosf(pitch));
            const float hr = roll * 0.5f, hp = pitch * 0.5f, hy = yaw * 0.5f;
            const float cr = cosf(hr), sr = sinf(hr), cp = cosf(hp), sp = sinf(hp), cy = cosf(hy), sy = sinf(hy);
            qw = (cr * cp) * cy + (sr * sp) * sy;
            qx = (sr * cp) * cy - (cr * sp) * sy;
            qy = (cr * sp) * cy + (sr * cp) * sy;
            qz = (cr * cp) * sy - (sr * sp) * cy;
            // 7. pose
            pz = zc + a.ride_height;
        }
        pp[0] = px; pp[1] = py; pp[2] = pz;
        if (k.quat_vec) {
            *reinterpret_cast<float4*>(qp) = make_float4(qw, qx, qy, qz);
        } else {
            qp[0] = qw; qp[1] = qx; qp[2] = qy; qp[3] = qz;
        }
    }
    if (a.joint_pos13) {                       // ideal actuators: all 13 columns (the targets' non-actuated columns are always 0)
        const uint64_t n = 13ull * a.E;
        copy_joint_rows(a.joint_pos_targets13, a.joint_pos13, n, k.joint_vec != 0);
        copy_joint_rows(a.joint_vel_targets13, a.joint_vel13, n, k.joint_vec != 0);
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

hipError_t launch_motion(const MotionArgs& a, hipStream_t s) {
    if (a.E == 0) return hipSuccess;
    MotionKernelArgs k{a, aligned16(a.quat4) ? 1 : 0,
                       (a.joint_pos13 && aligned16(a.joint_pos13) && aligned16(a.joint_vel13) && aligned16(a.joint_pos_targets13) &&
                        aligned16(a.joint_vel_targets13)) ? 1 : 0};
    if (a.h.rcp) hipLaunchKernelGGL(rover_motion_kernel<1>, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, k);
    else hipLaunchKernelGGL(rover_motion_kernel<0>, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, k);
    return hipGetLastError();
}

}  // namespace rover
