// rover_pose.h — the pose's device maths: quaternion -> euler angles, their sin / cos, the body transform and the wheel joint chain.
// Users: the ray preparation (rover_rays.hip) and quat_to_euler / pre_physics (rover_reset.hip).  One definition, text as it stood in
// the step's kernel file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rover {

// ---------------------------------------------------------------------------------------------------
// shared device maths (same operation order as oracle/rover_oracle.c, which cites the reference lines)
// ---------------------------------------------------------------------------------------------------

// tensor_quat_to_euler.py:17-29, one angle at a time (prep_rays_kernel gives each to a wave of its own)
__device__ __forceinline__ float quat_roll(const float* __restrict__ q) {
    float w = q[0], x = q[1], y = q[2], z = q[3];
    float sinr = 2.0f * (w * x + y * z);
    float cosr = 1.0f - (2.0f * (x * x + y * y));
    return atan2f(sinr, cosr);
}
__device__ __forceinline__ float quat_pitch(const float* __restrict__ q) {
    const float half_pi = 3.1415927410125732f / 2.0f;
    float w = q[0], x = q[1], y = q[2], z = q[3];
    float sinp = 2.0f * (w * y - z * x);
    float t = sinp - 1.0f;
    return (t >= 0.0f) ? copysignf(half_pi, sinp) : asinf(sinp);
}
__device__ __forceinline__ float quat_yaw(const float* __restrict__ q) {
    float w = q[0], x = q[1], y = q[2], z = q[3];
    float siny = 2.0f * (w * z + x * y);
    float cosy = 1.0f - (2.0f * (y * y + z * z));
    return atan2f(siny, cosy);
}
__device__ __forceinline__ void quat_to_euler(const float* __restrict__ q, float& roll, float& pitch, float& yaw) {
    roll = quat_roll(q); pitch = quat_pitch(q); yaw = quat_yaw(q);
}

struct Trig6 { float sx, cx, sy, cy, sz, cz; };

__device__ __forceinline__ Trig6 euler_trig(float roll, float pitch, float yaw) {
    Trig6 t;
    t.sx = sinf(-roll);  t.cx = cosf(-roll);
    t.sy = sinf(-pitch); t.cy = cosf(-pitch);
    t.sz = sinf(-yaw);   t.cz = cosf(-yaw);
    return t;
}

// rock_detect.py:305-307 / :356-358 — f32 body transform
__device__ __forceinline__ void body_xf(float x, float y, float z, const Trig6& t, float px, float py, float pz,
                                        float& ox, float& oy, float& oz) {
    float A = y * t.cx + z * t.sx;
    float C = z * t.cx - y * t.sx;
    float B = x * t.cy - t.sy * C;
    ox = px + t.sz * A + t.cz * B;
    oy = py + t.cz * A - t.sz * B;
    oz = pz + x * t.sy + t.cy * C;
}

// rock_detect.py:256-258,275-277 then body_xf: wheel-local point -> world (translations zeroed for directions)
__device__ __forceinline__ void wheel_chain(float x, float y, float z, const float* t0, const float* t1,
                                            float sst, float cst, float ssx, float csx, float ssy, float csy,
                                            const Trig6& t, float px, float py, float pz,
                                            float& ox, float& oy, float& oz) {
    float x1 = t0[0] + x * cst + y * sst;
    float y1 = t0[1] + y * cst - x * sst;
    float z1 = t0[2] + z;
    float c1 = z1 * csx - y1 * ssx;
    float x2 = t1[0] + x1 * csy - ssy * c1;
    float y2 = t1[1] + y1 * csx + z1 * ssx;
    float z2 = t1[2] + x1 * ssy + csy * c1;
    body_xf(x2, y2, z2, t, px, py, pz, ox, oy, oz);
}

}  // namespace rover
