// rover_rays.hip — hand-written HIP kernels (gfx950 / CDNA4, wave64) for the rover env.step() hot path: ray preparation, the two
// every-triangle ray casts, the ray exports / import.
//
// Reference (pure PyTorch; paths relative to omniisaacgymenvs/):
//   tasks/utils/camera/camera.py:60-145,165-212,233-264     (terrain ray cast)
//   tasks/utils/camera/ray_casting.py:3-66                   (ray/triangle)
//   tasks/utils/rock_detection/rock_detect.py:52-149,160-371 (wheel/body rays)
//   tasks/utils/math/tensor_quat_to_euler.py:6-31
//
// Built with -ffp-contract=off: every f32 +,-,*,/ and sqrt is one IEEE rounding, in the reference's own
// evaluation order, so that given identical rays the ray kernel agrees bit for bit with the CPU oracle and
// differs from the reference's fp32 mode only through sin/cos/atan2/asin ulps.
//
// Kernels (one fused step = the launches marked * — seven with the default 37 + 26 rays, where prep_rays_kernel counts the
// sort's coarse buckets itself and bucket_hist_kernel is not launched; the ray cast of full batches is rover_cull.hip's):
// (the sort's kernels are rover_sort.hip's, obs_metrics_kernel and compact_write_kernel rover_obs.hip's: marked * there)
//   repack_knn_kernel        init: (map_idx, tris, verts) -> per-cell contiguous fp16 block [cell][9][K8], near/far halves per lane
// * prep_rays_kernel         64 envs x a range of ray slots per block: quat -> euler, heading, the pose's and the wheels' sin/cos and the
//                            direction per ray kind once per block, then per slot origin, cell id, bin key [+ the sort's first pass] (A2, A4, A6)
// * cull_scan_kernel         (rover_cull.hip) the culled ray cast: 1 wave / run of sorted rays                      (A4, A5) <- roofline kernel
//   raycast_binned_kernel    variant 2: 1 wave / run of sorted rays, 4 triangles per lane in registers, every triangle evaluated,
//                            conservative early out (round 1's roofline kernel; the bit-for-bit reference of the culled one);
//                            <1>: the same in the reference's as-shipped fp16 arithmetic (ray_precision 2)
//   raycast_kernel           variant 1: env order, half-wave per ray, streams the cell blocks (small batches, K8 > 256)
//   export_dist / export_rays / import_rays kernels   the optional intermediates and rover_cast_rays' caller-supplied rays
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rover_internal.h"
#include "rover_raymath.h"
#include "rover_height.h"      // cell_coord
#include "rover_pose.h"

namespace rover {

// The ray's normal-cone bound for the culled ray cast (rover_cull.hip), a 16-bit fraction rounded up, 0xffff = none; (dx, dy, dz) = the
// ray record's direction.  f32 proof: a cell whose triangles all have |N_z| / |N| above ROVER_CONE_TAU |d_z| + |d_xy| meets test (B) as a whole.
// As-shipped fp16 arithmetic (precision 2): (B)'s threshold is per triangle, the cell stores the largest angle from the vertical a ray
// may have (as a fraction of pi / 2) and the ray its angle beta (d is normalised in fp16 there: re-normalised here).
__device__ __forceinline__ uint32_t ray_cone_bound(float dx, float dy, float dz, int precision) {
    uint32_t qq = 0xffffu;
    if (precision == 2) {
        const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
        const float beta = acosf(fminf(1.0f, fabsf(dz) * inv)) * 0.63661977f + 4.0e-5f;      // / (pi / 2), rounded up
        if (beta < 0.9999f) qq = (uint32_t)ceilf(beta * 65535.0f);                            // NaN -> 0xffff
    } else {
        const float qm = (float)ROVER_CONE_TAU * fabsf(dz) + sqrtf(dx * dx + dy * dy) + 2.0e-5f;
        if (qm < 0.9999f) qq = (uint32_t)ceilf(qm * 65535.0f);                                // NaN -> 0xffff
    }
    return qq;
}

// -(F.normalize(dir)), ray_casting.py:31
__device__ __forceinline__ void neg_normalize(float dx, float dy, float dz, float& ox, float& oy, float& oz) {
    float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    if (nrm < 1e-12f) nrm = 1e-12f;
    ox = -(dx / nrm); oy = -(dy / nrm); oz = -(dz / nrm);
}

// ---------------------------------------------------------------------------------------------------
// init: re-pack the reference's three tables into per-cell contiguous fp16 blocks [cell][9][K8]
// component q = 3*vertex + coord; padding triangles (K..K8) are NaN so every test on them fails.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) repack_knn_kernel(const int32_t* __restrict__ map_idx, const int32_t* __restrict__ tris,
                                                         const uint16_t* __restrict__ verts, uint64_t n_cells, uint32_t K,
                                                         uint32_t K8, uint32_t T, uint32_t V, uint16_t* __restrict__ table) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;       // one thread per (cell, k8)
    if (i >= n_cells * K8) return;
    uint64_t cell = i / K8;
    uint32_t slot = (uint32_t)(i % K8);
    // Slot order inside a cell block: lane l of the binned ray cast reads slots 4l..4l+3 as two packed pairs.  Its first
    // pair holds the list entries 2l, 2l+1 (the NEARER half of the K-nearest list), its second pair the entries
    // K8/2 + 2l, K8/2 + 2l + 1 (the farther half): a ray almost never reaches the far half, so the wave can drop that
    // pair as a whole after a cheap conservative test (cast_pairs).  The min over a cell is order-free, so the other
    // consumers (raycast_kernel) do not care.
    const uint32_t lane = slot >> 2, j = slot & 3u;
    const uint32_t k = (j < 2u) ? 2u * lane + j : (K8 >> 1) + 2u * lane + (j - 2u);
    uint16_t v[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) v[q] = 0x7e00u;                         // fp16 NaN
    if (k < K) {
        uint32_t t = (uint32_t)map_idx[cell * K + k];
        if (t < T) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                uint32_t vi = (uint32_t)tris[3 * (uint64_t)t + a];
                if (vi < V) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[3 * a + c] = verts[3 * (uint64_t)vi + c];
                }
            }
        }
    }
    uint16_t* dst = table + cell * 9ull * K8 + slot;
#pragma unroll
    for (int q = 0; q < 9; ++q) dst[(uint64_t)q * K8] = v[q];
}

// ---------------------------------------------------------------------------------------------------
// prep: one thread per (env, slot).  slots 0..23 wheel rays, 24..25 body rays, 26..26+P-1 terrain rays,
// rest padding to a multiple of 8 (a ray-cast workgroup then never straddles two envs).
// ---------------------------------------------------------------------------------------------------
__constant__ float c_wheel_ray[5][3] = {{0.215 / 2, 0.130 / 2, 0.1}, {0.215 / 2, -0.130 / 2, 0.1},
                                        {-0.215 / 2, 0.130 / 2, 0.1}, {-0.215 / 2, -0.130 / 2, 0.1}, {0, 0, -1}};
__constant__ float c_wp0[6][3] = {{0.286, 0.385, -0.197}, {0.286, -0.385, -0.197}, {-0.146, 0.447, -0.197},
                                  {-0.146, -0.447, -0.197}, {-0.440, 0.385, -0.197}, {-0.440, -0.385, -0.197}};
__constant__ float c_wp1[6][3] = {{0.153, 0, 0.03}, {0.153, 0, 0.03}, {0.153, 0, 0.03}, {0.153, -0.0, 0.03},
                                  {0, 0, 0.03}, {0, 0, 0.03}};
__constant__ float c_body_pt[2][3] = {{0.340, 0, -0.01}, {-0.485, 0, -0.01}};

// per (env, slot): ray origin, unit direction, cell id, bin key.
// A workgroup takes 64 envs and a range of slot groups (8 slots each): in a group wave w works on ONE slot (8 g + w) of the 64 envs, so the
// three kinds of slot — wheel rays (f32 joint chain), body rays, heightmap rays (f64 transform) — never share a wave and the slot's constants
// are wave-uniform.  (One wave per env, lane = slot, ran all three branches in every wave: 373 VALU instructions for work of ~120, 46 us.)
// The 64 x 8 records of a group leave through LDS: per env the 8 slots are 256 contiguous bytes.
//
// What depends on the POSE only is built once per block, before the loop over its slot groups (the kernel is bound by its arithmetic —
// 20 M VALU instructions per launch at 65 536 envs x 64 slots when every block of 8 slots rebuilt it, 37 us; its stores are not what it
// waits for: 16-byte records made it 1 us faster):
//  phase 1  the tasks {roll, pitch, yaw (+ heading), one per wheel the block's slots touch} dealt over the 8 waves: an euler angle
//           (tensor_quat_to_euler.py:17-29) with its sin / cos, or the six sin / cos of a wheel's steer / suspension joints
//           (rock_detect.py:248-272); the block of slot range 0 writes euler / heading out.  (Until round 4 a kernel of its own,
//           prep_env_kernel, wrote a 240-byte record per env that this kernel read back: one launch more.)
//  phase 2  a ray's DIRECTION is its kind's — the four rays of a wheel share one (rock_detect.py:305-319), the two body rays one
//           (:356-371), all heightmap rays of a rover one (camera.py:179-181,202-212): wave k < 6 builds wheel k's, wave 6 the body
//           rays', wave 7 the heightmap rays' record — un-normalised direction, the fp16 rounding of the as-shipped modes, -normalize
//           (ray_casting.py:31), the ray's normal-cone bound for the culled ray cast.
//  phase 3  per slot group: origin, cell, bin key; the records leave through LDS.
#define PREP_SLOTS 8
__global__ void __launch_bounds__(64 * PREP_SLOTS) prep_rays_kernel(PrepArgs a, uint32_t groups_per_block) {
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t e0 = blockIdx.x * 64u, e = e0 + lane;
    const uint32_t n_groups = a.R8 / PREP_SLOTS, g0 = blockIdx.y * groups_per_block, g1 = min(g0 + groups_per_block, n_groups);
    const uint32_t s_lo = g0 * PREP_SLOTS, s_hi = g1 * PREP_SLOTS;                        // the block's slots
    const uint32_t wh_lo = min(6u, s_lo >> 2), wh_hi = min(6u, s_hi >> 2);                // the wheels they touch
    const bool live = e < a.E;
    const uint32_t n_real = 26u + a.P;
    const uint32_t ec = min(e, a.E - 1u);                                                 // loads come from clamped (always valid) addresses
    const float px = a.pos[3ull * ec], py = a.pos[3ull * ec + 1], pz = a.pos[3ull * ec + 2];
    // the distribution point of a heightmap slot: a SCALAR load (the address is wave-uniform) — as a vector load its s_waitcnt vmcnt
    // would also wait for the previous slot group's stores to be acknowledged
    auto dist_of = [&](uint32_t slot, double& x, double& y, double& z) {
        const double* p = a.dist + 3ull * (slot - 26u);
        asm volatile("s_load_dwordx2 %0, %3, 0x0\n\ts_load_dwordx2 %1, %3, 0x8\n\ts_load_dwordx2 %2, %3, 0x10\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(x), "=&s"(y), "=&s"(z) : "s"(p) : "memory");
    };
    __shared__ float2 s_trig[3][64];            // (sin, cos) of -roll, -pitch, -yaw of the block's 64 envs
    __shared__ float2 s_wheel[6][3][64];        // [wheel][(sin, cos) of -steer | susX | susY][env]
    __shared__ float4 s_dir[8][64];             // [kind] {dx, dy, dz, flags: map | valid << 1 | cone bound << 16}
    // optionally the first pass of the bucket sort (launch_bin_rays): the block's keys counted per coarse bucket in LDS, then added to the
    // row of the sort tile the block's 64 envs lie in (a few blocks per row; the table is all zero when the kernel starts)
    extern __shared__ uint32_t s_hist[];        // [a.hist_buckets] when a.hist
    if (a.hist) for (uint32_t i = threadIdx.x; i < a.hist_buckets; i += 64u * PREP_SLOTS) s_hist[i] = 0u;
    const uint32_t n_tasks = 3u + (wh_hi - wh_lo);
    for (uint32_t task = w; task < n_tasks; task += PREP_SLOTS) {
        if (task < 3u) {
            // one atan2 / asin and one sin / cos pair (yaw: also the heading): a third of the dependent chain each (one wave doing all
            // three angles kept the other seven waiting 1.5 us at the barrier)
            float ang;
            if (a.euler_in) {                   // (wave-uniform) the pose's euler angles as given: rover_get_depths / rover_get_collisions
                ang = a.euler_in[3ull * ec + task];
            } else {
                const float* qp = a.quat + 4ull * ec;
                const float q[4] = {qp[0], qp[1], qp[2], qp[3]};
                ang = task == 0u ? quat_roll(q) : (task == 1u ? quat_pitch(q) : quat_yaw(q));
            }
            s_trig[task][lane] = make_float2(sinf(-ang), cosf(-ang));
            if (blockIdx.y == 0u && live) {
                if (a.euler) a.euler[3ull * e + task] = ang;
                if (task == 2u && a.heading) {
                    const float* tp = a.target ? a.target : a.pos;
                    const float tx = tp[3ull * ec] - px, ty = tp[3ull * ec + 1] - py;
                    const float hx = cosf(ang), hy = sinf(ang);                           // heading_diff, rover.py:279-283
                    a.heading[e] = -atan2f(tx * hy - ty * hx, tx * hx + ty * hy);
                }
            }
        } else {
            const uint32_t wh = wh_lo + (task - 3u);
            const float* j = a.joints ? a.joints + 13ull * ec : nullptr;
            const float j0 = j ? j[0] : 0.0f, j1 = j ? j[1] : 0.0f, j2 = j ? j[2] : 0.0f, j4 = j ? j[4] : 0.0f, j6 = j ? j[6] : 0.0f,
                        j7 = j ? j[7] : 0.0f, j8 = j ? j[8] : 0.0f;
            const float steer = (wh == 0) ? j4 : (wh == 1) ? j6 : (wh == 4) ? -j7 : (wh == 5) ? j8 : 0.0f;         // :248
            const float susY = (wh == 0 || wh == 2) ? -j0 : (wh == 1 || wh == 3) ? j1 : 0.0f;                      // :263
            const float susX = (wh >= 4) ? -j2 : 0.0f;                                                           // :264
            s_wheel[wh][0][lane] = make_float2(sinf(-steer), cosf(-steer));
            s_wheel[wh][1][lane] = make_float2(sinf(susX), cosf(susX));
            s_wheel[wh][2][lane] = make_float2(sinf(susY), cosf(susY));
        }
    }
    __syncthreads();
    Trig6 t;
    {
        const float2 tr = s_trig[0][lane], tp2 = s_trig[1][lane], ty2 = s_trig[2][lane];
        t.sx = tr.x; t.cx = tr.y; t.sy = tp2.x; t.cy = tp2.y; t.sz = ty2.x; t.cz = ty2.y;
    }
    // the pose in float64 for the heightmap rays (camera.py:165-212 works in the distribution tensor's float64; widened where it is
    // used: eighteen registers held through the loop would cost the kernel its eighth wave per SIMD)
#define PREP_POSE_F64                                                                                                                    \
    const double dsx = (double)t.sx, dcx = (double)t.cx, dsy = (double)t.sy, dcy = (double)t.cy, dsz = (double)t.sz, dcz = (double)t.cz; \
    const double X = (double)px, Y = (double)py, Z = (double)pz
    if (w < 6u ? (w >= wh_lo && w < wh_hi) : (w == 6u ? (s_lo < 26u && s_hi > 24u) : s_hi > 26u)) {
        float ux, uy, uz;
        uint32_t fl;
        if (w < 6u) {                           // wheel w: rock_detect.py:305-319
            const float2 d0 = s_wheel[w][0][lane], d1 = s_wheel[w][1][lane], d2 = s_wheel[w][2][lane];
            const float zero3[3] = {0.0f, 0.0f, 0.0f};
            wheel_chain(c_wheel_ray[4][0], c_wheel_ray[4][1], c_wheel_ray[4][2], zero3, zero3, d0.x, d0.y, d1.x, d1.y, d2.x, d2.y, t, 0.0f, 0.0f,
                        0.0f, ux, uy, uz);
            fl = 3u;
        } else if (w == 6u) {                   // the body rays: rock_detect.py:356-371
            float qx, qy, qz;
            body_xf(0.0f, 1.0f, 0.0f, t, px, py, pz, qx, qy, qz);
            ux = qx - px; uy = qy - py; uz = qz - pz;
            fl = 3u;
        } else {                                // the heightmap rays: the appended (0,0,-1) point, camera.py:179-181,202-204, float64
            PREP_POSE_F64;
            const double xn = 0.0, yn = 0.0, zn = -1.0;
            const double A = yn * dcx + zn * dsx, C = zn * dcx - yn * dsx, B = xn * dcy - dsy * C;
            ux = (float)((X + dsz * A + dcz * B) - X);
            uy = (float)((Y + dcz * A - dsz * B) - Y);
            uz = (float)((Z + xn * dsy + dcy * C) - Z);
            fl = 2u;
        }
        if (a.precision >= 1) { ux = (float)(_Float16)ux; uy = (float)(_Float16)uy; uz = (float)(_Float16)uz; }      // rover_dir.type(float16): camera.py:212, rock_detect.py:319,371
        float dx, dy, dz;
        if (a.precision == 2) {         // F.normalize on a float16 tensor: f32-accumulated norm rounded to fp16, fp16 division
            float nrm = (float)(_Float16)sqrtf(ux * ux + uy * uy + uz * uz);     // (eps 1e-12 is 0 in fp16)
            dx = -(float)(_Float16)(ux / nrm); dy = -(float)(_Float16)(uy / nrm); dz = -(float)(_Float16)(uz / nrm);
        } else {
            neg_normalize(ux, uy, uz, dx, dy, dz);
        }
        const uint32_t qq = ray_cone_bound(dx, dy, dz, a.precision);
        s_dir[w][lane] = make_float4(dx, dy, dz, __uint_as_float(fl | (qq << 16)));
    }
    // The group's 64 x 8 records and bin keys, env-major through LDS (rows of 17 float4 / 9 dwords: a wave's 64 rows spread over the banks):
    // a store instruction then writes four envs' 256-byte groups — whole lines — instead of 64 records 2 KB apart.
    __shared__ float4 s_t[64 * (2 * PREP_SLOTS + 1)];
    __shared__ uint32_t s_b[64 * (PREP_SLOTS + 1)];
    float4* const rays4 = reinterpret_cast<float4*>(a.rays);
    const Trig6& t_ = t;
    const float px_ = px, py_ = py, pz_ = pz;
    for (uint32_t g = g0; g < g1; ++g) {
        const uint32_t slot0 = g * PREP_SLOTS, slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(slot0 + w));
        RayRec rec;
        rec.sx = rec.sy = rec.sz = 0.0f; rec.cell = 0u; rec.dx = rec.dy = 0.0f; rec.dz = 1.0f; rec.flags = 0u;
        uint32_t bin = 0xffffffffu;
        const bool real = live && slot < n_real;
        uint32_t kind = 0u;
        if (real) {
            float sx, sy, sz;                  // origin
            const bool rk = slot < 26u;         // the ray's map: rocks, or the terrain
            const float m_shift_x = rk ? a.rocks.shift_x : a.terrain.shift_x, m_shift_y = rk ? a.rocks.shift_y : a.terrain.shift_y;
            const float m_cell = rk ? a.rocks.cell : a.terrain.cell, m_inv_cell = rk ? a.rocks.inv_cell : a.terrain.inv_cell;
            const int32_t m_X = rk ? a.rocks.X : a.terrain.X, m_Y = rk ? a.rocks.Y : a.terrain.Y;
            if (slot < 24u) {                   // rock_detect.py:160-319
                const uint32_t wh = slot >> 2, r = slot & 3u;
                const float2 d0 = s_wheel[wh][0][lane], d1 = s_wheel[wh][1][lane], d2 = s_wheel[wh][2][lane];
                wheel_chain(c_wheel_ray[r][0], c_wheel_ray[r][1], c_wheel_ray[r][2], c_wp0[wh], c_wp1[wh], d0.x, d0.y, d1.x, d1.y,
                            d2.x, d2.y, t, px, py, pz, sx, sy, sz);
                kind = wh;
            } else if (slot < 26u) {            // rock_detect.py:321-371
                const uint32_t r = slot - 24u;
                body_xf(c_body_pt[r][0], c_body_pt[r][1], c_body_pt[r][2], t, px, py, pz, sx, sy, sz);
                kind = 6u;
            } else {                            // camera.py:165-212, float64 like the distribution tensor
                Trig6 t = t_;                   // (opaque copies: hoisted out of the loop the widened pose is those eighteen registers)
                float px = px_, py = py_, pz = pz_;
                asm volatile("" : "+v"(t.sx), "+v"(t.cx), "+v"(t.sy), "+v"(t.cy), "+v"(t.sz), "+v"(t.cz), "+v"(px), "+v"(py), "+v"(pz));
                PREP_POSE_F64;
                double x, y, z;
                dist_of(slot, x, y, z);
                const double A = y * dcx + z * dsx, C = z * dcx - y * dsx, B = x * dcy - dsy * C;
                sx = (float)(X + dsz * A + dcz * B);
                sy = (float)(Y + dcz * A - dsz * B);
                sz = (float)(Z + x * dsy + dcy * C);
                kind = 7u;
            }
            if (a.precision >= 1) { sx = (float)(_Float16)sx; sy = (float)(_Float16)sy; sz = (float)(_Float16)sz; }      // sources.type(float16): camera.py:212
            rec.sx = sx; rec.sy = sy; rec.sz = sz;
            uint32_t ix = cell_coord(sx, m_shift_x, m_cell, m_inv_cell, a.cell_rcp, m_X);
            uint32_t iy = cell_coord(sy, m_shift_y, m_cell, m_inv_cell, a.cell_rcp, m_X);
            if (iy > (uint32_t)(m_Y - 1)) iy = (uint32_t)(m_Y - 1);        // memory safety only
            rec.cell = ix * (uint32_t)m_Y + iy;
            bin = (rk ? a.rocks_bin_offset : 0u) + rec.cell;
            if (a.hist) atomicAdd(&s_hist[bin >> a.hist_low_bits], 1u);
        }
        // the direction records are written (first group: the waves that did not build one have worked on their origins meanwhile);
        // the previous group's records have left s_t / s_b
        __syncthreads();
        if (real) {
            const float4 dr = s_dir[kind][lane];
            rec.dx = dr.x; rec.dy = dr.y; rec.dz = dr.z; rec.flags = __float_as_uint(dr.w);
        }
        s_t[lane * (2 * PREP_SLOTS + 1) + 2u * w] = make_float4(rec.sx, rec.sy, rec.sz, __uint_as_float(rec.cell));
        s_t[lane * (2 * PREP_SLOTS + 1) + 2u * w + 1u] = make_float4(rec.dx, rec.dy, rec.dz, __uint_as_float(rec.flags));
        s_b[lane * (PREP_SLOTS + 1) + w] = bin;                  // key of the bucket sort; 0xffffffff for padding slots
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < 2u; ++r) {
            const uint32_t idx = threadIdx.x + r * 64u * PREP_SLOTS, el = idx / (2u * PREP_SLOTS), q = idx % (2u * PREP_SLOTS);
            if (e0 + el < a.E) rays4[((size_t)(e0 + el) * a.R8 + slot0) * 2u + q] = s_t[el * (2 * PREP_SLOTS + 1) + q];
        }
        {       // (four groups' keys gathered in LDS and written as whole 128-byte lines: 45 KB of LDS, three blocks per CU, +2.6 us)
            const uint32_t el = threadIdx.x / PREP_SLOTS, q = threadIdx.x % PREP_SLOTS;
            if (a.bin_out && e0 + el < a.E) a.bin_out[(size_t)(e0 + el) * a.R8 + slot0 + q] = s_b[el * (PREP_SLOTS + 1) + q];
        }
    }
#undef PREP_POSE_F64
    if (a.hist) {
        __syncthreads();
        uint32_t* const row = a.hist + (size_t)(blockIdx.x / a.hist_blocks_per_tile) * a.hist_buckets;
        for (uint32_t i = threadIdx.x; i < a.hist_buckets; i += 64u * PREP_SLOTS) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(row + i, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// ray cast — the roofline kernel.  32 lanes per ray; a lane owns 8 consecutive triangles of the cell per
// pass: nine 16-byte loads (one per vertex component) straight to VGPRs, fp16 -> f32, Möller–Trumbore with
// the reference's padded barycentric test, running min; 5-step shuffle min over the 32 lanes.
// Algorithmic traffic: 18 B per (ray, triangle).
// ---------------------------------------------------------------------------------------------------
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float tri_test(float v0x, float v0y, float v0z, float v1x, float v1y, float v1z,
                                          float ax, float ay, float az, float sx, float sy, float sz,
                                          float dx, float dy, float dz) {
    // ray_casting.py:34-59; a = v2
    float bx = v1x - ax, by = v1y - ay, bz = v1z - az;
    float cx = v0x - ax, cy = v0y - ay, cz = v0z - az;
    float gx = sx - ax, gy = sy - ay, gz = sz - az;
    float bcx = by * cz - bz * cy, bcy = bz * cx - bx * cz, bcz = bx * cy - by * cx;
    float det = bcx * dx + bcy * dy + bcz * dz;
    float gcx = gy * cz - gz * cy, gcy = gz * cx - gx * cz, gcz = gx * cy - gy * cx;
    float n = (gcx * dx + gcy * dy + gcz * dz) / det;
    float bgx = by * gz - bz * gy, bgy = bz * gx - bx * gz, bgz = bx * gy - by * gx;
    float m = (bgx * dx + bgy * dy + bgz * dz) / det;
    float k = (bcx * gx + bcy * gy + bcz * gz) / det;
    bool ok = (n >= RAY_NEG_EPS) && (m >= RAY_NEG_EPS) && (n + m <= RAY_ONE_EPS)
              && (det != RAY_NEG_EPS) && (det != RAY_ONE_EPS);       // :46,:51,:56 guards
    return ok ? k : RAY_MISS;
}

__global__ void __launch_bounds__(256) raycast_kernel(const RayRec* __restrict__ rays, uint32_t n_rays,
                                                      const _Float16* __restrict__ tab0, const _Float16* __restrict__ tab1,
                                                      uint32_t kp0, uint32_t kp1, float* __restrict__ out) {
    const uint32_t ray = (blockIdx.x * 256u + threadIdx.x) >> 5;
    const uint32_t l = threadIdx.x & 31u;
    float best = __builtin_inff();
    const bool active = ray < n_rays;
    if (active) {
        const float4* rp = reinterpret_cast<const float4*>(rays + ray);
        const float4 ra = rp[0], rb = rp[1];
        const uint32_t cell = __float_as_uint(ra.w), flags = __float_as_uint(rb.w);
        if (flags & 2u) {
            const uint32_t kp = (flags & 1u) ? kp1 : kp0;
            const _Float16* base = ((flags & 1u) ? tab1 : tab0) + (size_t)cell * 9u * kp;
            for (uint32_t c = l * 8u; c < kp; c += 256u) {
                half8 v[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) v[q] = *reinterpret_cast<const half8*>(base + (size_t)q * kp + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float r = tri_test((float)v[0][j], (float)v[1][j], (float)v[2][j], (float)v[3][j], (float)v[4][j],
                                       (float)v[5][j], (float)v[6][j], (float)v[7][j], (float)v[8][j],
                                       ra.x, ra.y, ra.z, rb.x, rb.y, rb.z);
                    best = (r < best) ? r : best;
                }
            }
        }
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        float o = __shfl_xor(best, off, 32);
        best = (o < best) ? o : best;
    }
    if (active && l == 0u) out[ray] = best;
}

// optional intermediates: the per-ray distances by kind, and the other two return values of Camera.get_depths (camera.py:145) —
// the ray origins (camera.py:212) and the "intersection points" sources - d * k (ray_casting.py:63: d = -normalize(direction), the
// ray record's direction; k = the ray's distance, 11.0 for a miss).  As shipped (precision 2) the product and the difference are
// fp16 operations on fp16 values: rounded once each (the f32 product of two fp16 values is exact, and rounding an f32 difference of
// fp16 values to fp16 equals the fp16 difference: 24 >= 2 * 11 + 2 bits).
__global__ void __launch_bounds__(256) export_dist_kernel(const float* __restrict__ dist, const RayRec* __restrict__ rays, uint32_t E,
                                                          uint32_t R8, uint32_t P, int precision, float* __restrict__ ray_dist,
                                                          float* __restrict__ wheel, float* __restrict__ body,
                                                          float* __restrict__ ray_src, float* __restrict__ hit_pt) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n = 26u + P;
    if (i >= (uint64_t)E * n) return;
    uint32_t e = (uint32_t)(i / n), s = (uint32_t)(i % n);
    float v = dist[(uint64_t)e * R8 + s];
    if (s < 24u) { if (wheel) wheel[24ull * e + s] = v; }
    else if (s < 26u) { if (body) body[2ull * e + (s - 24u)] = v; }
    else {
        const uint64_t o = (uint64_t)e * P + (s - 26u);
        if (ray_dist) ray_dist[o] = v;
        if (ray_src || hit_pt) {
            const RayRec r = rays[(uint64_t)e * R8 + s];
            if (ray_src) { ray_src[3 * o] = r.sx; ray_src[3 * o + 1] = r.sy; ray_src[3 * o + 2] = r.sz; }
            if (hit_pt) {
                float tx = r.dx * v, ty = r.dy * v, tz = r.dz * v;
                if (precision == 2) { tx = (float)(_Float16)tx; ty = (float)(_Float16)ty; tz = (float)(_Float16)tz; }
                float hx = r.sx - tx, hy = r.sy - ty, hz = r.sz - tz;
                if (precision == 2) { hx = (float)(_Float16)hx; hy = (float)(_Float16)hy; hz = (float)(_Float16)hz; }
                hit_pt[3 * o] = hx; hit_pt[3 * o + 1] = hy; hit_pt[3 * o + 2] = hz;
            }
        }
    }
}

// The ray records of the last cast in slot order (24 wheel, 2 body, P heightmap rays per env): origin, the record's direction
// (-normalize(direction), ray_casting.py:31), cell id, distance — what a test feeds to the oracle's per-ray arithmetic.
__global__ void __launch_bounds__(256) export_rays_kernel(const RayRec* __restrict__ rays, const float* __restrict__ dist, uint32_t E, uint32_t R8,
                                                          uint32_t n_real, float* __restrict__ src, float* __restrict__ dir,
                                                          int32_t* __restrict__ cell, float* __restrict__ out_dist) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)E * n_real) return;
    const uint32_t e = (uint32_t)(i / n_real), sl = (uint32_t)(i % n_real);
    const RayRec r = rays[(uint64_t)e * R8 + sl];
    if (src) { src[3 * i] = r.sx; src[3 * i + 1] = r.sy; src[3 * i + 2] = r.sz; }
    if (dir) { dir[3 * i] = r.dx; dir[3 * i + 1] = r.dy; dir[3 * i + 2] = r.dz; }
    if (cell) cell[i] = (int32_t)r.cell;
    if (out_dist) out_dist[i] = dist[(uint64_t)e * R8 + sl];
}

// Caller-supplied rays into the step's workspace (rover_cast_rays): origin and record direction as given, cell id, map flag, cone bound
// and bin key as prep_rays_kernel derives them from an origin / a direction (camera.py:233-264 for the cell).
__global__ void __launch_bounds__(256) import_rays_kernel(const float* __restrict__ src, const float* __restrict__ dir, uint32_t E, uint32_t R8,
                                                          uint32_t n_real, KnnDev terrain, KnnDev rocks, uint32_t rocks_bin_offset,
                                                          int precision, int cell_rcp, RayRec* __restrict__ rays, uint32_t* __restrict__ bin_out,
                                                          uint32_t* __restrict__ not_unit) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)E * R8) return;
    const uint32_t e = (uint32_t)(i / R8), sl = (uint32_t)(i % R8);
    RayRec rec;
    rec.sx = rec.sy = rec.sz = 0.0f; rec.cell = 0u; rec.dx = rec.dy = 0.0f; rec.dz = 1.0f; rec.flags = 0u;
    uint32_t bin = 0xffffffffu;
    if (sl < n_real) {
        const uint64_t o = 3ull * ((uint64_t)e * n_real + sl);
        const bool rk = sl < 26u;
        const KnnDev& m = rk ? rocks : terrain;
        rec.sx = src[o]; rec.sy = src[o + 1]; rec.sz = src[o + 2];
        rec.dx = dir[o]; rec.dy = dir[o + 1]; rec.dz = dir[o + 2];
        // the rejection proofs of the culled / staged ray cast take |d|^2 <= 1.00001 (f32; as shipped, normalised in fp16: within 4e-3 of 1),
        // what -normalize() gives: a finite direction of another length is counted, rover_cast_rays refuses the call (NaN compares false
        // in every test: such a ray keeps all its candidates by itself)
        if (not_unit) {
            const float dd = rec.dx * rec.dx + rec.dy * rec.dy + rec.dz * rec.dz;
            if (fabsf(dd - 1.0f) > (precision == 2 ? 4.0e-3f : 1.0e-5f)) atomicAdd(not_unit, 1u);
        }
        const uint32_t ix = cell_coord(rec.sx, m.shift_x, m.cell, m.inv_cell, cell_rcp, m.X);
        uint32_t iy = cell_coord(rec.sy, m.shift_y, m.cell, m.inv_cell, cell_rcp, m.X);
        if (iy > (uint32_t)(m.Y - 1)) iy = (uint32_t)(m.Y - 1);
        rec.cell = ix * (uint32_t)m.Y + iy;
        rec.flags = (rk ? 3u : 2u) | (ray_cone_bound(rec.dx, rec.dy, rec.dz, precision) << 16);
        bin = (rk ? rocks_bin_offset : 0u) + rec.cell;
    }
    rays[i] = rec;
    if (bin_out) bin_out[i] = bin;
}

// ---------------------------------------------------------------------------------------------------
// ray cast over the binned rays.  One wave walks RUN consecutive sorted rays.  When the cell changes the
// wave loads the cell block (4 triangles per lane, 9 x 8-byte loads) and sets up a, b = v1-a, c = v0-a, b x c
// in registers; every further ray of the same cell only pays the ray-dependent part of ray_casting.py:37-59.
// The three quotients share one reciprocal refinement: the exact instruction sequence of the IEEE f32
// division expansion without its range scaling (den and quotients here are far from the f32 range ends),
// so results stay bit-identical to n = N/det, m = M/det, k = K/det.
// H = 1: the reference's AS-SHIPPED arithmetic (option ray_precision = 2): Camera.dtype = float16, so every elementwise ATen op
// of ray_casting.py:31-59 rounds to fp16.  The per-pair maths in packed fp16 (v_pk_mul_f16 / v_pk_add_f16, one rounding per op,
// no contraction); the three quotients are taken in f32 (IEEE, shared reciprocal) and rounded to fp16, which equals the fp16
// quotient (24 >= 2*11 + 2 bits).  Bit-identical to the oracle's fp16 mode, which the as-shipped golden fixture pins bit for bit.
// (the fp16 (ray, triangle) arithmetic — CellRegsH, set_pair_h, cast_pairs_h — lives in rover_raymath.h: one definition for this
// kernel and the culled ray cast's exact phase)
// ---------------------------------------------------------------------------------------------------
template <int H>
__global__ void __launch_bounds__(256) raycast_binned_kernel(const RayRec* __restrict__ rays, const uint32_t* __restrict__ sorted,
                                                             uint32_t n_sorted, const _Float16* __restrict__ tab0,
                                                             const _Float16* __restrict__ tab1, uint32_t kp0, uint32_t kp1,
                                                             uint32_t run, uint32_t n_blocks, uint32_t nb8,
                                                             uint32_t pre_terrain, uint32_t pre_rocks, float* __restrict__ out) {
    // XCD-aware order: blocks b, b+8, b+16.. run on one XCD (round-robin dispatch) -> give each XCD one
    // contiguous eighth of the sorted rays so a cell's rays meet in one L2.  Speed only, never correctness.
    const uint32_t lb = (blockIdx.x & 7u) * nb8 + (blockIdx.x >> 3);
    if (lb >= n_blocks) return;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(lb * 4u + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t i = wave * run;
    if (i >= n_sorted) return;
    const uint32_t i_end = min(i + run, n_sorted);
    uint32_t cur_cell = 0xffffffffu, cur_map = 0xffffffffu;
    std::conditional_t<H != 0, CellRegsH<2>, CellRegs<2>> t;      // per lane: 4 triangles as 2 packed pairs
    t.poison();
    uint64_t vmask[2][2] = {{0, 0}, {0, 0}};
    for (; i < i_end; ++i) {
        const uint32_t gid = __builtin_amdgcn_readfirstlane(sorted[i]);
        const float4* rp = reinterpret_cast<const float4*>(rays + gid);
        const float4 ra = rp[0], rb = rp[1];
        const uint32_t cell = __builtin_amdgcn_readfirstlane(__float_as_uint(ra.w));
        const uint32_t map = __builtin_amdgcn_readfirstlane(__float_as_uint(rb.w)) & 1u;
        if (cell != cur_cell || map != cur_map) {
            if (map != cur_map && cur_map != 0xffffffffu && kp0 != kp1) t.poison();   // lanes past the new map's K
            cur_cell = cell; cur_map = map;
            const uint32_t kp = map ? kp1 : kp0;
            const _Float16* base = (map ? tab1 : tab0) + (size_t)cell * 9u * kp + lane * 4u;
            if (lane * 4u < kp) {
                half4 v[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) v[q] = *reinterpret_cast<const half4*>(base + (size_t)q * kp);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int t0 = 2 * p, t1 = 2 * p + 1;
                    if constexpr (H) {
                        h2 vv[9];
#pragma unroll
                        for (int q = 0; q < 9; ++q) vv[q] = h2{v[q][t0], v[q][t1]};
                        set_pair_h(t, p, vv);
                    } else {
                        f2 w[9];
#pragma unroll
                        for (int q = 0; q < 9; ++q) w[q] = f2{(float)v[q][t0], (float)v[q][t1]};
                        set_pair(t, p, w);
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {                     // real (non-NaN) triangles per pair element, all lanes vote
                vmask[p][0] = __builtin_amdgcn_ballot_w64(t.ax[p].x == t.ax[p].x);
                vmask[p][1] = __builtin_amdgcn_ballot_w64(t.ax[p].y == t.ax[p].y);
            }
        }
        float best;
        if constexpr (H) {
            // the record holds fp16 values widened to f32 (prep_rays_kernel, precision 2): the casts are exact
            const _Float16 hsx = (_Float16)ra.x, hsy = (_Float16)ra.y, hsz = (_Float16)ra.z;
            const _Float16 hdx = (_Float16)rb.x, hdy = (_Float16)rb.y, hdz = (_Float16)rb.z;
            best = cast_pairs_h<2>(t, h2{hsx, hsx}, h2{hsy, hsy}, h2{hsz, hsz}, h2{hdx, hdx}, h2{hdy, hdy}, h2{hdz, hdz}, vmask,
                                   map ? pre_rocks : pre_terrain);
        } else {
            const f2 sx = {ra.x, ra.x}, sy = {ra.y, ra.y}, sz = {ra.z, ra.z};
            const f2 dx = {rb.x, rb.x}, dy = {rb.y, rb.y}, dz = {rb.z, rb.z};
            best = cast_pairs<2>(t, sx, sy, sz, dx, dy, dz, vmask, map ? pre_rocks : pre_terrain);
        }
        best = wave_min_to_lane63(best);
        if (lane == 63u) out[gid] = best;
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t launch_repack(const int32_t* map_idx, const int32_t* tris, const uint16_t* verts, uint64_t n_cells, uint32_t K,
                         uint32_t K8, uint32_t T, uint32_t V, uint16_t* table, hipStream_t s) {
    uint64_t n = n_cells * K8;
    hipLaunchKernelGGL(repack_knn_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, map_idx, tris, verts, n_cells, K, K8, T, V, table);
    return hipGetLastError();
}

hipError_t launch_prep(const PrepArgs& a, hipStream_t s) {
    // 64 envs x a range of slot groups per block: as many groups as still leave ~1 024 blocks (the pose work is per block; with the
    // fused histogram's LDS above 40 KB — more than 576 buckets — three blocks fit a CU, not four: 2 048 blocks then)
    const uint32_t target = (a.hist && a.hist_buckets > 576u) ? 2048u : 1024u;
    const uint32_t xb = blocks_for(a.E, 64), n_groups = a.R8 / PREP_SLOTS;                // (R8 is a multiple of 8)
    const uint32_t yb = max(1u, min(n_groups, (target + xb - 1u) / xb)), gpb = (n_groups + yb - 1u) / yb;
    hipLaunchKernelGGL(prep_rays_kernel, dim3(xb, (n_groups + gpb - 1u) / gpb), dim3(64 * PREP_SLOTS), a.hist ? a.hist_buckets * 4u : 0u, s, a, gpb);
    return hipGetLastError();
}

hipError_t launch_raycast(const RayRec* rays, uint32_t n_rays, const uint16_t* tab0, const uint16_t* tab1, uint32_t kp0,
                          uint32_t kp1, float* out, hipStream_t s) {
    hipLaunchKernelGGL(raycast_kernel, dim3(blocks_for(n_rays, 8)), dim3(256), 0, s, rays, n_rays,
                       reinterpret_cast<const _Float16*>(tab0), reinterpret_cast<const _Float16*>(tab1), kp0, kp1, out);
    return hipGetLastError();
}

hipError_t launch_raycast_binned(const RayRec* rays, const uint32_t* sorted, uint32_t n_sorted, const uint16_t* tab0,
                                 const uint16_t* tab1, uint32_t kp0, uint32_t kp1, uint32_t run, bool fp16_math, uint32_t early_out,
                                 float* out, hipStream_t s) {
    const uint32_t n_waves = blocks_for(n_sorted, run);
    const uint32_t n_blocks = blocks_for(n_waves, 4);
    const uint32_t nb8 = blocks_for(n_blocks, 8);
    const _Float16* t0 = reinterpret_cast<const _Float16*>(tab0);
    const _Float16* t1 = reinterpret_cast<const _Float16*>(tab1);
    // pair 1 = the far half of a cell's list: tested on both maps; pair 0 (near half) only on the rocks map, where most
    // rays are far from any rock triangle
    // (A/B in one process, 65 536 envs, f32 kernel: none 1.424 ms, far pair only 1.228, every pair 1.249, this choice 1.169)
    const uint32_t pre_terrain = early_out ? 2u : 0u, pre_rocks = early_out ? 3u : 0u;
    if (fp16_math)
        hipLaunchKernelGGL(raycast_binned_kernel<1>, dim3(nb8 * 8u), dim3(256), 0, s, rays, sorted, n_sorted, t0, t1, kp0, kp1, run,
                           n_blocks, nb8, pre_terrain, pre_rocks, out);
    else
        hipLaunchKernelGGL(raycast_binned_kernel<0>, dim3(nb8 * 8u), dim3(256), 0, s, rays, sorted, n_sorted, t0, t1, kp0, kp1, run,
                           n_blocks, nb8, pre_terrain, pre_rocks, out);
    return hipGetLastError();
}

hipError_t launch_export_dist(const float* dist, const RayRec* rays, uint32_t E, uint32_t R8, uint32_t P, int precision, float* ray_dist,
                              float* wheel, float* body, float* ray_src, float* hit_pt, hipStream_t s) {
    hipLaunchKernelGGL(export_dist_kernel, dim3(blocks_for((uint64_t)E * (26u + P), 256)), dim3(256), 0, s, dist, rays, E, R8, P, precision,
                       ray_dist, wheel, body, ray_src, hit_pt);
    return hipGetLastError();
}

hipError_t launch_export_rays(const RayRec* rays, const float* dist, uint32_t E, uint32_t R8, uint32_t P, float* src, float* dir, int32_t* cell,
                              float* out_dist, hipStream_t s) {
    hipLaunchKernelGGL(export_rays_kernel, dim3(blocks_for((uint64_t)E * (26u + P), 256)), dim3(256), 0, s, rays, dist, E, R8, 26u + P, src, dir,
                       cell, out_dist);
    return hipGetLastError();
}

hipError_t launch_import_rays(const float* src, const float* dir, uint32_t E, uint32_t R8, uint32_t P, const KnnDev& terrain, const KnnDev& rocks,
                              uint32_t rocks_bin_offset, int precision, int cell_rcp, RayRec* rays, uint32_t* bin_out, hipStream_t s,
                              uint32_t* not_unit) {
    hipLaunchKernelGGL(import_rays_kernel, dim3(blocks_for((uint64_t)E * R8, 256)), dim3(256), 0, s, src, dir, E, R8, 26u + P, terrain, rocks,
                       rocks_bin_offset, precision, cell_rcp, rays, bin_out, not_unit);
    return hipGetLastError();
}

}  // namespace rover
