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
// rover_motion_bogie_kernel is the rocker-bogie posture mode (rover_motion_step_bogie): the same steps 1-3, the contacts
// at the wheel rays' layout, and in place of the plane fit the six unknowns (z_c, roll, pitch, j0, j1, j2) that put all six wheel-frame
// origins on their targets, by a chord iteration with the constant inverse of the Jacobian at rest.  The three joint angles go to columns
// 0-2 of the joint state.  rover_motion_kernel is not touched by it.
//
// rover_motion_drive_kernel is the wheel-level drive mode (rover_motion_step_drive): rate-limited steering and drive
// joints, the body twist fitted to the six wheel velocity vectors, and either posture through the device functions the two kernels above
// use (plane_posture, bogie_posture).  It stages the four joint arrays in LDS; the other two kernels use none.
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

// Steps 4-7 of rover_motion_step on the new position (px, py) and heading yaw (cs, sn its cosine and sine): the body's z and quaternion.
// rover_motion_kernel and the plane instances of rover_motion_drive_kernel both go through it, so the same (px, py, yaw) gives the same bits.
__device__ __forceinline__ void plane_posture(const HeightDev& hf, const float (&fit)[3][MOTION_WHEELS], float ride_height, float px, float py,
                                              float yaw, float cs, float sn, float& pz, float& qw, float& qx, float& qy, float& qz) {
    const float wl[MOTION_WHEELS][2] = {{-0.385, 0.438}, {0.385, 0.438}, {-0.447, 0.0}, {0.447, 0.0}, {-0.385, -0.411}, {0.385, -0.411}};
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
    float zc = fit[0][0] * z[0], p = fit[1][0] * z[0], q = fit[2][0] * z[0];
#pragma unroll
    for (int i = 1; i < MOTION_WHEELS; ++i) {
        zc = zc + fit[0][i] * z[i];
        p = p + fit[1][i] * z[i];
        q = q + fit[2][i] * z[i];
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
    pz = zc + ride_height;
}

// RCP: the heightfield's cell_index_mode as a compile-time value — cell_coord's choice between the division and the reciprocal is
// then no branch, the six lookups of a sub-step stand in one basic block and their loads are issued back to back
template <int RCP>
__global__ void __launch_bounds__(256) rover_motion_kernel(MotionKernelArgs k) {
    const MotionArgs& a = k.m;
    HeightDev hf = a.h;
    hf.rcp = RCP;
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
            plane_posture(hf, a.fit, a.ride_height, px, py, yaw, cs, sn, pz, qw, qx, qy, qz);
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

// ---- the rocker-bogie posture mode ------------------------------------------------------------------------------------------------------
// rock_detect.py:201-215: the wheel frame's origin is T1 + Rsus(T0) in the body frame (FL, FR, CL, CR, RL, RR); T0's z is -0.197 and
// T1's z 0.03 for every wheel, T1's x is 0.153 on the four bogie wheels and 0 on the rear pair, T1's y is 0
#define BOGIE_T0 {{0.286, 0.385}, {0.286, -0.385}, {-0.146, 0.447}, {-0.146, -0.447}, {-0.440, 0.385}, {-0.440, -0.385}}
// (forward a_i, left b_i) of the origins with all joints at 0: T0 + T1
#define BOGIE_LAYOUT {{0.439, 0.385}, {0.439, -0.385}, {0.007, 0.447}, {0.007, -0.447}, {-0.440, 0.385}, {-0.440, -0.385}}

// out = inv(g) by cofactors, as motion_plane_fit inverts its normal matrix
static void inv3(const double g[3][3], double out[3][3]) {
    const double det = g[0][0] * (g[1][1] * g[2][2] - g[1][2] * g[2][1]) - g[0][1] * (g[1][0] * g[2][2] - g[1][2] * g[2][0]) +
                       g[0][2] * (g[1][0] * g[2][1] - g[1][1] * g[2][0]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            out[r][c] = (g[r1][c1] * g[r2][c2] - g[r1][c2] * g[r2][c1]) / det;
        }
}

// D = inv(J), J = dF/du at u = 0 for u = (z_c, roll, pitch, j0, j1, j2): dF_i/dz_c = 1, dF_i/droll = b_i, dF_i/dpitch = -a_i, and a wheel
// swings about its pivot: dF/dj0 = -x0 (FL, CL: susY = -j0), dF/dj1 = +x0 (FR, CR: susY = j1), dF/dj2 = y0 (RL, RR: susX = -j2).
// The layout is mirror-symmetric, so J splits into two 3 x 3 systems over the three axles k = front, centre, rear: the half sums of the
// left and right rows determine (z_c, pitch, p = (j1 - j0) / 2) through S = [1, -a_k, x0_k | 0 for the rear], the half differences
// determine (roll, m = (j0 + j1) / 2, j2) through A = [b_k, -x0_k | 0, 0 | y0 for the rear]; j0 = m - p, j1 = m + p.  Inverted by
// cofactors in double, each entry of D rounded to f32 once; the entries that are 0 by symmetry (roll does not answer to the rear pair)
// come out as exact zeros.
void motion_bogie_fit(float out[MOTION_WHEELS][MOTION_WHEELS]) {
    const double t0[MOTION_WHEELS][2] = BOGIE_T0, ab[MOTION_WHEELS][2] = BOGIE_LAYOUT;
    double S[3][3], A[3][3], Si[3][3], Ai[3][3];
    for (int k = 0; k < 3; ++k) {
        const int i = 2 * k;                   // the axle's left wheel
        S[k][0] = 1.0; S[k][1] = -ab[i][0]; S[k][2] = (k < 2) ? t0[i][0] : 0.0;
        A[k][0] = ab[i][1]; A[k][1] = (k < 2) ? -t0[i][0] : 0.0; A[k][2] = (k < 2) ? 0.0 : t0[i][1];
    }
    inv3(S, Si);
    inv3(A, Ai);
    for (int k = 0; k < 3; ++k)
        for (int side = 0; side < 2; ++side) {
            const int i = 2 * k + side;
            const double sg = side ? -0.5 : 0.5;
            const double zc = 0.5 * Si[0][k], pitch = 0.5 * Si[1][k], p = 0.5 * Si[2][k];
            const double roll = sg * Ai[0][k], m = sg * Ai[1][k], j2 = sg * Ai[2][k];
            out[0][i] = (float)zc; out[1][i] = (float)roll; out[2][i] = (float)pitch;
            out[3][i] = (float)(m - p); out[4][i] = (float)(m + p); out[5][i] = (float)j2;
            for (int n = 0; n < MOTION_WHEELS; ++n) out[n][i] += 0.0f;         // a zero is +0
        }
}

struct BogieKernelArgs {
    MotionArgs m;                          // m.fit is not used
    int32_t quat_vec, joint_vec;
    float inv[MOTION_WHEELS][MOTION_WHEELS];       // motion_bogie_fit()
    int32_t iters;
    float max_bogie;
};

// Steps 4-6 of rover_motion_step_bogie on the new position (px, py) and heading yaw: the unknowns u = (z_c, roll, pitch, j0, j1, j2) of
// this sub-step's solve (z1 = u[0], the joints unclamped) and the quaternion; off = ride_height - 0.167f.  Shared by
// rover_motion_bogie_kernel and the bogie instances of rover_motion_drive_kernel.
__device__ __forceinline__ void bogie_posture(const HeightDev& hf, const float (&inv)[MOTION_WHEELS][MOTION_WHEELS], int32_t iters, float off,
                                              float px, float py, float yaw, float cs, float sn, float (&u)[MOTION_WHEELS], float& qw, float& qx,
                                              float& qy, float& qz) {
    const float ab[MOTION_WHEELS][2] = BOGIE_LAYOUT, t0[MOTION_WHEELS][2] = BOGIE_T0;
    const float t0z = -0.197f, t1x = 0.153f, t1z = 0.03f;
    // 4. the six wheel contacts, sampled at yaw only: every lookup is issued before the first one is used
    float t[MOTION_WHEELS];
#pragma unroll
    for (int i = 0; i < MOTION_WHEELS; ++i) {
        const float wx = (px + ab[i][0] * cs) - ab[i][1] * sn;
        const float wy = (py + ab[i][0] * sn) + ab[i][1] * cs;
        t[i] = height_at(hf, wx, wy);
    }
#pragma unroll
    for (int i = 0; i < MOTION_WHEELS; ++i) t[i] = t[i] + off;
    // 5. posture: the chord iteration u <- u + D (t - F(u)) from u = 0
#pragma unroll
    for (int i = 0; i < MOTION_WHEELS; ++i) u[i] = 0.0f;
    for (int32_t it = 0; it < iters; ++it) {
        const float sr = sinf(u[1]), cr = cosf(u[1]), sp = sinf(u[2]), cp = cosf(u[2]);
        const float sus[3] = {-u[3], u[4], -u[5]};          // susY of FL and CL, susY of FR and CR, susX of RL and RR
        float ss[3], cc[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { ss[j] = sinf(sus[j]); cc[j] = cosf(sus[j]); }
        float r[MOTION_WHEELS];
#pragma unroll
        for (int i = 0; i < MOTION_WHEELS; ++i) {
            float bx, by, bz;                               // the wheel frame's origin in the body frame: rock_detect.py:275-277
            if (i < 4) {                                    // susX = 0
                const float ssy = ss[i & 1], csy = cc[i & 1];
                bx = (t1x + t0[i][0] * csy) - ssy * t0z;
                by = t0[i][1];
                bz = (t1z + t0[i][0] * ssy) + csy * t0z;
            } else {                                        // susY = 0, T1's x is 0
                const float c1 = t0z * cc[2] - t0[i][1] * ss[2];
                bx = t0[i][0];
                by = t0[i][1] * cc[2] + t0z * ss[2];
                bz = t1z + c1;
            }
            const float h = bz * cr + by * sr;              // the ZYX rotation's third row: (-sin pitch, cos pitch sin roll, cos pitch cos roll)
            r[i] = t[i] - ((u[0] - bx * sp) + cp * h);
        }
#pragma unroll
        for (int n = 0; n < MOTION_WHEELS; ++n) {
            float acc = inv[n][0] * r[0];
#pragma unroll
            for (int i = 1; i < MOTION_WHEELS; ++i) acc = acc + inv[n][i] * r[i];
            u[n] = u[n] + acc;
        }
    }
    // 6. orientation: roll and pitch are the unknowns themselves
    const float hr = u[1] * 0.5f, hp = u[2] * 0.5f, hy = yaw * 0.5f;
    const float chr = cosf(hr), shr = sinf(hr), chp = cosf(hp), shp = sinf(hp), cy = cosf(hy), sy = sinf(hy);
    qw = (chr * chp) * cy + (shr * shp) * sy;
    qx = (shr * chp) * cy - (chr * shp) * sy;
    qy = (chr * shp) * cy + (shr * chp) * sy;
    qz = (chr * chp) * sy - (shr * shp) * cy;
}

template <int RCP>
__global__ void __launch_bounds__(256) rover_motion_bogie_kernel(BogieKernelArgs k) {
    const MotionArgs& a = k.m;
    HeightDev hf = a.h;
    hf.rcp = RCP;
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    float u[MOTION_WHEELS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};        // (z_c, roll, pitch, j0, j1, j2) of the last sub-step
    if (e < a.E) {
        float* pp = a.pos3 + 3ull * e;
        float* qp = a.quat4 + 4ull * e;
        float px = pp[0], py = pp[1];
        float qw, qx, qy, qz;
        if (k.quat_vec) {
            const float4 q = *reinterpret_cast<const float4*>(qp);
            qw = q.x; qx = q.y; qy = q.z; qz = q.w;
        } else {
            qw = qp[0]; qx = qp[1]; qy = qp[2]; qz = qp[3];
        }
        // 1. commands, as rover_motion_kernel
        const float v = a.lin[(uint64_t)e * (uint32_t)a.cmd_stride] * a.max_lin;
        const float w = a.ang[(uint64_t)e * (uint32_t)a.cmd_stride] * a.max_ang;
        const float v_eff = (fabsf(v / w) > 0.45f) ? v : 0.0f;
        const float dyaw = w * a.dt;
        const float off = a.ride_height - 0.167f;                  // the origins lie at body z = -0.167
        for (int32_t s = 0; s < a.substeps; ++s) {
            // 2. heading, 3. position
            const float yaw0 = atan2f(2.0f * (qw * qz + qx * qy), 1.0f - (2.0f * (qy * qy + qz * qz)));
            const float yaw = yaw0 + dyaw;
            const float cs = cosf(yaw), sn = sinf(yaw);
            px = px + (v_eff * cs) * a.dt;
            py = py + (v_eff * sn) * a.dt;
            bogie_posture(hf, k.inv, k.iters, off, px, py, yaw, cs, sn, u, qw, qx, qy, qz);
        }
        // 7. pose: z = z_c
        pp[0] = px; pp[1] = py; pp[2] = u[0];
        if (k.quat_vec) {
            *reinterpret_cast<float4*>(qp) = make_float4(qw, qx, qy, qz);
        } else {
            qp[0] = qw; qp[1] = qx; qp[2] = qy; qp[3] = qz;
        }
    }
    if (a.joint_pos13) {
        // the block copies its envs' rows, all 13 columns; a barrier, then each env's thread overwrites columns 0-2 of its position row
        // with the clamped joint angles (the barrier is in uniform control flow: joint_pos13 is a kernel argument)
        const uint64_t n = 13ull * a.E;
        copy_joint_rows(a.joint_pos_targets13, a.joint_pos13, n, k.joint_vec != 0);
        copy_joint_rows(a.joint_vel_targets13, a.joint_vel13, n, k.joint_vec != 0);
        __syncthreads();
        if (e < a.E) {
            float* jp = a.joint_pos13 + 13ull * e;
#pragma unroll
            for (int j = 0; j < 3; ++j) jp[j] = fminf(fmaxf(u[3 + j], -k.max_bogie), k.max_bogie);
        }
    }
}

static int32_t joint_vec_of(const MotionArgs& a) {
    return (a.joint_pos13 && aligned16(a.joint_pos13) && aligned16(a.joint_vel13) && aligned16(a.joint_pos_targets13) &&
            aligned16(a.joint_vel_targets13)) ? 1 : 0;
}

hipError_t launch_motion_bogie(const MotionArgs& a, int32_t iters, float max_bogie, hipStream_t s) {
    if (a.E == 0) return hipSuccess;
    BogieKernelArgs k{a, aligned16(a.quat4) ? 1 : 0, joint_vec_of(a), {}, iters, max_bogie};
    motion_bogie_fit(k.inv);
    if (a.h.rcp) hipLaunchKernelGGL(rover_motion_bogie_kernel<1>, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, k);
    else hipLaunchKernelGGL(rover_motion_bogie_kernel<0>, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, k);
    return hipGetLastError();
}

hipError_t launch_motion(const MotionArgs& a, hipStream_t s) {
    if (a.E == 0) return hipSuccess;
    MotionKernelArgs k{a, aligned16(a.quat4) ? 1 : 0,
                       (a.joint_pos13 && aligned16(a.joint_pos13) && aligned16(a.joint_vel13) && aligned16(a.joint_pos_targets13) &&
                        aligned16(a.joint_vel_targets13)) ? 1 : 0};
    if (a.h.rcp) hipLaunchKernelGGL(rover_motion_kernel<1>, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, k);
    else hipLaunchKernelGGL(rover_motion_kernel<0>, dim3(blocks_for(a.E, 256)), dim3(256), 0, s, k);
    return hipGetLastError();
}

// ---- the wheel-level drive mode ---------------------------------------------------------------------------------------------------------
// rover_motion_step_drive (include/rover_step.h): the joint state follows the joint targets at a limited rate, the six
// wheels' velocity vectors give the body twist by a constant least-squares fit, and the posture is the plane's or the bogie's.

// (vx, vy, w) = P t with P = pinv(M), M [12][3] with rows (1, 0, -b_i), (0, 1, a_i): P = (M^T M)^-1 M^T in double (condition number 1.87),
// each entry rounded to f32 once.  sum b_i = 0 exactly, so vx is the mean of the x components and the entries that pair vx with a y
// component, or vy and w with nothing of theirs, come out as exact +0.
void motion_drive_fit(float out[3][2 * MOTION_WHEELS]) {
    const double wl[MOTION_WHEELS][2] = {{-0.385, 0.438}, {0.385, 0.438}, {-0.447, 0.0}, {0.447, 0.0}, {-0.385, -0.411}, {0.385, -0.411}};   // (right, forward)
    double M[2 * MOTION_WHEELS][3], G[3][3] = {}, inv[3][3];
    for (int i = 0; i < MOTION_WHEELS; ++i) {
        M[2 * i][0] = 1.0; M[2 * i][1] = 0.0; M[2 * i][2] = wl[i][0];                 // -b_i = r_i
        M[2 * i + 1][0] = 0.0; M[2 * i + 1][1] = 1.0; M[2 * i + 1][2] = wl[i][1];     // a_i = f_i
    }
    for (int j = 0; j < 2 * MOTION_WHEELS; ++j)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) G[r][c] += M[j][r] * M[j][c];
    inv3(G, inv);
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 2 * MOTION_WHEELS; ++j)
            out[r][j] = (float)(inv[r][0] * M[j][0] + inv[r][1] * M[j][1] + inv[r][2] * M[j][2]) + 0.0f;      // a zero is +0
}

#define DRIVE_TILE (256 * 13)              // floats: one workgroup's rows of one [E, 13] array

struct DriveKernelArgs {
    MotionArgs m;                          // lin, ang, cmd_stride, max_lin, max_ang are not read; fit only by the plane instances
    int32_t quat_vec, joint_vec;
    float P[3][2 * MOTION_WHEELS];         // motion_drive_fit()
    float wheel_radius, steer_rate, wheel_accel;
    float* slip;                           // [E] or NULL
    float inv[MOTION_WHEELS][MOTION_WHEELS];       // motion_bogie_fit(); the bogie instances only
    int32_t iters;
    float max_bogie;
};

// The workgroup's `cnt` floats of one [E, 13] array, global -> LDS and back.  cnt = 13 * (the block's envs); the block's range starts at
// a multiple of 4 floats, so with 16-byte aligned bases every float4 is aligned in global memory and in the tile.  The loads of the
// aligned path are held in registers so that the four tiles' loads are all in flight before the first LDS write waits for one.
__device__ __forceinline__ float4 tile_fetch4(const float* __restrict__ src, uint32_t cnt, int k) {
    const uint32_t i = 4u * (threadIdx.x + 256u * k);
    return (i < (cnt & ~3u)) ? *reinterpret_cast<const float4*>(src + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ float tile_fetch_tail(const float* __restrict__ src, uint32_t cnt) {
    const uint32_t i = (cnt & ~3u) + threadIdx.x;
    return (i < cnt) ? src[i] : 0.0f;
}
__device__ __forceinline__ void tile_put4(float* tile, uint32_t cnt, int k, float4 v) {
    const uint32_t i = 4u * (threadIdx.x + 256u * k);
    if (i < (cnt & ~3u)) *reinterpret_cast<float4*>(tile + i) = v;
}
__device__ __forceinline__ void tile_put_tail(float* tile, uint32_t cnt, float v) {
    const uint32_t i = (cnt & ~3u) + threadIdx.x;
    if (i < cnt) tile[i] = v;
}
__device__ __forceinline__ void tile_store(const float* tile, float* __restrict__ dst, uint32_t cnt, bool vec) {
    if (vec) {
        const uint32_t cnt4 = cnt & ~3u;
        for (uint32_t i = 4u * threadIdx.x; i < cnt4; i += 4u * 256u) *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(tile + i);
        if (cnt4 + threadIdx.x < cnt) dst[cnt4 + threadIdx.x] = tile[cnt4 + threadIdx.x];
    } else {
        for (uint32_t i = threadIdx.x; i < cnt; i += 256u) dst[i] = tile[i];
    }
}

// state <- target where it is within `step`, else one step towards it.  Written with > so that a NaN difference takes the (NaN) target;
// fl(state + step) never passes the target, because |target - state| > step and rounding is monotone.
__device__ __forceinline__ float rate_limit(float state, float target, float step) {
    const float d = target - state;
    return (fabsf(d) > step) ? state + copysignf(step, d) : target;
}

// One thread per env, as the two kernels above; the workgroup stages its rows of the four joint arrays in LDS (4 x 13 KB): the
// cooperative loads and stores are contiguous, and a thread's own row is read at a stride of 13 words, which is odd and so free of bank
// conflicts.  The target tiles double as the output: a thread writes its new actuator states (and, BOGIE, the solved angles) over its
// row's targets, and the block stores the two tiles to joint_pos13 / joint_vel13 — every other column is then the targets' copy.
template <int RCP, int BOGIE>
__global__ void __launch_bounds__(256) rover_motion_drive_kernel(DriveKernelArgs k) {
    __shared__ __align__(16) float tiles[4][DRIVE_TILE];           // position targets, velocity targets, positions, velocities
    const MotionArgs& a = k.m;
    HeightDev hf = a.h;
    hf.rcp = RCP;
    const float wl[MOTION_WHEELS][2] = {{-0.385, 0.438}, {0.385, 0.438}, {-0.447, 0.0}, {0.447, 0.0}, {-0.385, -0.411}, {0.385, -0.411}};
    const int steer_col[4] = {4, 6, 7, 8};                         // FL, FR, RL, RR: the columns pre_physics_step writes
    const int steer_wheel[4] = {0, 1, 4, 5};
    const int drive_col[MOTION_WHEELS] = {9, 10, 3, 5, 11, 12};    // FL, FR, ML, MR, RL, RR
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * DRIVE_TILE;
    const uint64_t left = 13ull * a.E - first;
    const uint32_t cnt = left < DRIVE_TILE ? (uint32_t)left : (uint32_t)DRIVE_TILE;
    const float* src[4] = {a.joint_pos_targets13 + first, a.joint_vel_targets13 + first, a.joint_pos13 + first, a.joint_vel13 + first};
    if (k.joint_vec) {
        float4 r[4][4];
        float tail[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) r[t][q] = tile_fetch4(src[t], cnt, q);
            tail[t] = tile_fetch_tail(src[t], cnt);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) tile_put4(tiles[t], cnt, q, r[t][q]);
            tile_put_tail(tiles[t], cnt, tail[t]);
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            for (uint32_t i = threadIdx.x; i < cnt; i += 256u) tiles[t][i] = src[t][i];
    }
    __syncthreads();
    if (e < a.E) {
        float* pt = tiles[0] + 13u * threadIdx.x;
        float* vt = tiles[1] + 13u * threadIdx.x;
        const float* jp = tiles[2] + 13u * threadIdx.x;
        const float* jv = tiles[3] + 13u * threadIdx.x;
        float dl[4], dl_t[4], om[MOTION_WHEELS], om_t[MOTION_WHEELS];      // steering angles and wheel speeds, states and targets
#pragma unroll
        for (int j = 0; j < 4; ++j) { dl[j] = jp[steer_col[j]]; dl_t[j] = pt[steer_col[j]]; }
#pragma unroll
        for (int i = 0; i < MOTION_WHEELS; ++i) { om[i] = jv[drive_col[i]]; om_t[i] = vt[drive_col[i]]; }
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
        const float step_s = k.steer_rate * a.dt, step_w = k.wheel_accel * a.dt;
        const float off = a.ride_height - 0.167f;
        float u[MOTION_WHEELS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float t[2 * MOTION_WHEELS], tw[3] = {0.0f, 0.0f, 0.0f};    // the last sub-step's wheel velocity vectors and twist (vx, vy, w)
        for (int32_t s = 0; s < a.substeps; ++s) {
            // 1. actuators
#pragma unroll
            for (int j = 0; j < 4; ++j) dl[j] = rate_limit(dl[j], dl_t[j], step_s);
#pragma unroll
            for (int i = 0; i < MOTION_WHEELS; ++i) om[i] = rate_limit(om[i], om_t[i], step_w);
            // 2. wheel velocity vectors; the centre wheels do not steer
#pragma unroll
            for (int i = 0; i < MOTION_WHEELS; ++i) { t[2 * i] = k.wheel_radius * om[i]; t[2 * i + 1] = 0.0f; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = steer_wheel[j];
                const float sp = t[2 * i];
                t[2 * i] = sp * cosf(dl[j]);
                t[2 * i + 1] = sp * sinf(dl[j]);
            }
            // 3. body twist
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float acc = k.P[r][0] * t[0];
#pragma unroll
                for (int j = 1; j < 2 * MOTION_WHEELS; ++j) acc = acc + k.P[r][j] * t[j];
                tw[r] = acc;
            }
            // 5. heading and position
            const float yaw0 = atan2f(2.0f * (qw * qz + qx * qy), 1.0f - (2.0f * (qy * qy + qz * qz)));
            const float yaw = yaw0 + tw[2] * a.dt;
            const float cs = cosf(yaw), sn = sinf(yaw);
            px = px + ((tw[0] * cs) - (tw[1] * sn)) * a.dt;
            py = py + ((tw[0] * sn) + (tw[1] * cs)) * a.dt;
            // 6. posture
            if (BOGIE) {
                bogie_posture(hf, k.inv, k.iters, off, px, py, yaw, cs, sn, u, qw, qx, qy, qz);
                pz = u[0];
            } else {
                plane_posture(hf, a.fit, a.ride_height, px, py, yaw, cs, sn, pz, qw, qx, qy, qz);
            }
        }
        pp[0] = px; pp[1] = py; pp[2] = pz;
        if (k.quat_vec) {
            *reinterpret_cast<float4*>(qp) = make_float4(qw, qx, qy, qz);
        } else {
            qp[0] = qw; qp[1] = qx; qp[2] = qy; qp[3] = qz;
        }
        // 4. slip of the last sub-step: the root mean square of the wheels' velocity against the rigid motion (vx, vy, w)
        if (k.slip) {
            float sum = 0.0f;
#pragma unroll
            for (int i = 0; i < MOTION_WHEELS; ++i) {
                const float dx = (tw[0] + tw[2] * wl[i][0]) - t[2 * i];        // vx - w b_i, b_i = -r_i
                const float dy = (tw[1] + tw[2] * wl[i][1]) - t[2 * i + 1];    // vy + w a_i
                const float q = dx * dx + dy * dy;
                sum = (i == 0) ? q : sum + q;
            }
            k.slip[e] = sqrtf(sum / 6.0f);
        }
        // the new states over the targets of the thread's own row
#pragma unroll
        for (int j = 0; j < 4; ++j) pt[steer_col[j]] = dl[j];
#pragma unroll
        for (int i = 0; i < MOTION_WHEELS; ++i) vt[drive_col[i]] = om[i];
        if (BOGIE) {
#pragma unroll
            for (int j = 0; j < 3; ++j) pt[j] = fminf(fmaxf(u[3 + j], -k.max_bogie), k.max_bogie);
        }
    }
    __syncthreads();
    tile_store(tiles[0], a.joint_pos13 + first, cnt, k.joint_vec != 0);
    tile_store(tiles[1], a.joint_vel13 + first, cnt, k.joint_vec != 0);
}

hipError_t launch_motion_drive(const MotionArgs& a, const DriveArgs& d, hipStream_t s) {
    if (a.E == 0) return hipSuccess;
    DriveKernelArgs k{a, aligned16(a.quat4) ? 1 : 0, joint_vec_of(a), {}, d.wheel_radius, d.steer_rate, d.wheel_accel, d.slip, {}, d.iters, d.max_bogie};
    motion_drive_fit(k.P);
    if (d.bogie) motion_bogie_fit(k.inv);
    const dim3 grid(blocks_for(a.E, 256)), block(256);
    if (d.bogie) {
        if (a.h.rcp) hipLaunchKernelGGL((rover_motion_drive_kernel<1, 1>), grid, block, 0, s, k);
        else hipLaunchKernelGGL((rover_motion_drive_kernel<0, 1>), grid, block, 0, s, k);
    } else {
        if (a.h.rcp) hipLaunchKernelGGL((rover_motion_drive_kernel<1, 0>), grid, block, 0, s, k);
        else hipLaunchKernelGGL((rover_motion_drive_kernel<0, 0>), grid, block, 0, s, k);
    }
    return hipGetLastError();
}

}  // namespace rover
