// rover_occlusion.hip — the sensor model's line-of-sight stage: which heightmap columns a camera on the rover's mast cannot see.
//
// The task's heightmap is cast straight down from just above the ground and sees behind every rock; a mast camera does not.  The
// reference has no camera model (tasks/utils/camera/rover_depth.py is a vestige of one); the definition this file implements is the
// project's own and is written out in include/rover_step.h (rover_obs_occlusion): per env and column, the point T the ray cast measured
// is rebuilt from the clean observation, the sight line from the camera to T is cut into n intervals, and the column is hidden when the
// heightfield rises more than `clearance` above the line at one of the n - 1 inner samples.
//
// One launch.  One workgroup of 256 threads per env, grid-strided over envs beyond OCC_MAX_GROUPS.  Thread 0 turns the pose into the
// rotation, Cam and the tile window's origin once per env (LDS); every thread then takes the column slots tid, tid + 256, ...
// Route 0 (TILES = false): slot = column, every sample reads its node.
// Route 1 (TILES = true): slot -> column through rover_set_occlusion's order (far first: the 64 lanes of a wave march about equally
// long), and a sample first asks the tile-max table — where tilemax <= line + clearance the node cannot hide and is not read.  The
// OCC_WIN x OCC_WIN tiles around the camera are staged in LDS (4 KB); a sample outside the window asks the table in memory.  The window
// only decides WHERE the tile's maximum is read from, and h <= tilemax holds for every node of the tile, so both routes give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rover_internal.h"
#include "rover_height.h"

namespace rover {

#define OCC_WIN 32                  // tiles per side of the LDS window: 32 x 8 nodes = 6.4 m at 0.025 m per node
#define OCC_MAX_GROUPS 4096u        // most workgroups; more envs than that are walked with a grid stride (256 CUs x 8 workgroups x 2)

// maxima of the OCC_TILE x OCC_TILE-node tiles of hm * vscale: one thread per tile, NaN nodes ignored (fmaxf), -inf when all are NaN
__global__ void __launch_bounds__(256) occlusion_tiles_kernel(HeightDev h, float* tilemax, int32_t TN0, int32_t TN1) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)TN0 * (uint32_t)TN1) return;
    const int32_t tx = (int32_t)(i / (uint32_t)TN1), ty = (int32_t)(i % (uint32_t)TN1);
    float m = -INFINITY;
    for (int32_t x = tx * OCC_TILE; x < (tx + 1) * OCC_TILE && x < h.N0; ++x)
        for (int32_t y = ty * OCC_TILE; y < (ty + 1) * OCC_TILE && y < h.N1; ++y)
            m = fmaxf(m, h.hm[(uint64_t)x * h.N1 + y] * h.vscale);
    tilemax[i] = m;
}

hipError_t launch_occlusion_tiles(const HeightDev& h, float* tilemax, int32_t TN0, int32_t TN1, hipStream_t s) {
    hipLaunchKernelGGL(occlusion_tiles_kernel, dim3(blocks_for((uint64_t)TN0 * (uint64_t)TN1, 256u)), dim3(256), 0, s, h, tilemax, TN0, TN1);
    return hipGetLastError();
}

// s_pose: r00 r01 r02 r10 r11 r12 r20 r21 r22, p, Cam
enum { OCC_R = 0, OCC_P = 9, OCC_CAM = 12, OCC_POSE = 15 };

__device__ __forceinline__ float occ_rot(const float* r, float v0, float v1, float v2) { return (r[0] * v0 + r[1] * v1) + r[2] * v2; }

template <bool TILES>
__global__ void __launch_bounds__(256) obs_occlusion_kernel(OcclusionArgs a) {
    __shared__ float s_pose[OCC_POSE];
    __shared__ int32_t s_org[2];
    __shared__ float s_win[TILES ? OCC_WIN * OCC_WIN : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t M = (uint32_t)a.M, first = (uint32_t)a.first, C = (uint32_t)(a.F - a.first);
    const HeightDev h = a.h;
    const bool in_place = a.in == a.out;
    for (uint32_t r = blockIdx.x; r < M; r += gridDim.x) {
        if (tid == 0) {
            const float* q4 = a.quat4 + (uint64_t)r * 4u;
            const float* p3 = a.pos3 + (uint64_t)r * 3u;
            const float w = q4[0], x = q4[1], y = q4[2], z = q4[3];
            float* R = s_pose + OCC_R;
            R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - w * z);        R[2] = 2.0f * (x * z + w * y);
            R[3] = 2.0f * (x * y + w * z);        R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - w * x);
            R[6] = 2.0f * (x * z - w * y);        R[7] = 2.0f * (y * z + w * x);        R[8] = 1.0f - 2.0f * (x * x + y * y);
            for (int i = 0; i < 3; ++i) {
                s_pose[OCC_P + i] = p3[i];
                s_pose[OCC_CAM + i] = p3[i] + occ_rot(R + 3 * i, a.camera[0], a.camera[1], a.camera[2]);
            }
            if (TILES) {                    // the window is centred on the camera's tile
                uint32_t ix = cell_coord(s_pose[OCC_CAM], h.shift_x, h.hscale, h.inv_hscale, h.rcp, h.N0);
                uint32_t iy = cell_coord(s_pose[OCC_CAM + 1], h.shift_y, h.hscale, h.inv_hscale, h.rcp, h.N0);
                if (iy > (uint32_t)(h.N1 - 1)) iy = (uint32_t)(h.N1 - 1);
                s_org[0] = (int32_t)(ix / OCC_TILE) - OCC_WIN / 2;
                s_org[1] = (int32_t)(iy / OCC_TILE) - OCC_WIN / 2;
            }
        }
        __syncthreads();
        if (TILES) {
            const int32_t ox = s_org[0], oy = s_org[1];
            for (uint32_t i = tid; i < OCC_WIN * OCC_WIN; i += 256u) {
                const int32_t tx = ox + (int32_t)(i / OCC_WIN), ty = oy + (int32_t)(i % OCC_WIN);
                const bool inside = tx >= 0 && tx < a.TN0 && ty >= 0 && ty < a.TN1;      // (no sample falls into a tile outside the table)
                s_win[i] = inside ? a.tilemax[(uint64_t)tx * a.TN1 + ty] : -INFINITY;
            }
            __syncthreads();
        }
        const float* R = s_pose + OCC_R;
        const float camx = s_pose[OCC_CAM], camy = s_pose[OCC_CAM + 1], camz = s_pose[OCC_CAM + 2];
        const float* clean = a.clean + (uint64_t)r * (uint64_t)a.clean_stride + first;
        const float* src = a.in + (uint64_t)r * (uint64_t)a.in_stride + first;
        float* dst = a.out + (uint64_t)r * (uint64_t)a.out_stride + first;
        for (uint32_t slot = tid; slot < C; slot += 256u) {
            const uint32_t c = TILES ? (uint32_t)a.order[slot] : slot;
            const float v = clean[c];
            bool hid = false;
            if (fabsf(v) < a.miss) {
                const float b0 = a.body3[3u * c], b1 = a.body3[3u * c + 1u], b2 = a.body3[3u * c + 2u];
                const float d = 2.0f * v;
                const float tx = (s_pose[OCC_P] + occ_rot(R, b0, b1, b2)) + d * (-R[2]);
                const float ty = (s_pose[OCC_P + 1] + occ_rot(R + 3, b0, b1, b2)) + d * (-R[5]);
                const float tz = (s_pose[OCC_P + 2] + occ_rot(R + 6, b0, b1, b2)) + d * (-R[8]);
                if (a.target3) {
                    float* t3 = a.target3 + ((uint64_t)r * C + c) * 3u;
                    t3[0] = tx; t3[1] = ty; t3[2] = tz;
                }
                const float dx = tx - camx, dy = ty - camy, dz = tz - camz;
                const float L = sqrtf(dx * dx + dy * dy);
                const float u = ceilf(L / a.step);
                const int32_t n = u < (float)a.max_steps ? (int32_t)u : a.max_steps;
                const float fn = (float)n;
                for (int32_t k = 1; k < n; ++k) {
                    const float t = (float)k / fn;
                    const float line = (camz + t * dz) + a.clearance;
                    uint32_t ix = cell_coord(camx + t * dx, h.shift_x, h.hscale, h.inv_hscale, h.rcp, h.N0);
                    uint32_t iy = cell_coord(camy + t * dy, h.shift_y, h.hscale, h.inv_hscale, h.rcp, h.N0);
                    if (iy > (uint32_t)(h.N1 - 1)) iy = (uint32_t)(h.N1 - 1);
                    if (TILES) {
                        const int32_t gx = (int32_t)(ix / OCC_TILE), gy = (int32_t)(iy / OCC_TILE);
                        const uint32_t lx = (uint32_t)(gx - s_org[0]), ly = (uint32_t)(gy - s_org[1]);
                        const float top = (lx < OCC_WIN && ly < OCC_WIN) ? s_win[lx * OCC_WIN + ly] : a.tilemax[(uint64_t)gx * a.TN1 + gy];
                        if (!(top > line)) continue;       // no node of the tile can hide here
                    }
                    if (h.hm[(uint64_t)ix * h.N1 + iy] * h.vscale > line) { hid = true; break; }
                }
            }
            const float keep = src[c];                     // read before the store: out may be exactly in
            dst[c] = hid ? a.drop_value : keep;
            if (a.hidden) a.hidden[(uint64_t)r * (uint64_t)a.hidden_stride + c] = hid ? 1u : 0u;
        }
        if (!in_place)                                     // the proprioceptive columns
            for (uint32_t col = tid; col < first; col += 256u) dst[(int64_t)col - (int64_t)first] = src[(int64_t)col - (int64_t)first];
        __syncthreads();                                   // s_pose / s_org / s_win are rewritten for the next env
    }
}

hipError_t launch_obs_occlusion(const OcclusionArgs& a, hipStream_t s) {
    const dim3 grid((uint32_t)a.M < OCC_MAX_GROUPS ? (uint32_t)a.M : OCC_MAX_GROUPS);
    if (a.route) hipLaunchKernelGGL((obs_occlusion_kernel<true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((obs_occlusion_kernel<false>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rover
