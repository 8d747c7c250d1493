// rover_internal.h — structs shared by the kernels (rover_*.hip) and the C-ABI layer (rover_capi*.cpp, through rover_ctx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rover_plan.h"      // the integer helpers plan_step shares with the launchers (bin_*, cull_queue_entries, cull_stat_slots, lane_*)

// Test (B) for a whole set of triangles by its normal cone (rover_cull.hip, header comment): the ray-side constant of the f32 proof.
#define ROVER_CONE_TAU 1.25e-2

namespace rover {

// One ray as the ray-cast kernel consumes it (32 B, two 16-byte loads).
struct RayRec {
    float sx, sy, sz;    // origin
    uint32_t cell;       // ix * Y + iy into the map the flags select
    float dx, dy, dz;    // -normalize(direction), ray_casting.py:31
    uint32_t flags;      // bit0: rocks map, bit1: valid; bits 16..31: the ray's normal-cone bound (rover_cull.hip), 0xffff = none
};
static_assert(sizeof(RayRec) == 32, "RayRec must be 32 bytes");

// One re-packed KNN map: per-cell contiguous fp16 block [X*Y][9][K8]
struct KnnDev {
    const uint16_t* table;
    int32_t X, Y, K, K8;         // K8: row pitch of one component inside a cell block (K rounded up to a multiple of 8)
    float cell, shift_x, shift_y;
    float inv_cell;              // 1.0f / cell rounded to f32: the factor of cell_index_mode 1 (cuda_rcp)
};

struct HeightDev {
    const float* hm;
    int32_t N0, N1;
    float hscale, vscale, shift_x, shift_y;
    float inv_hscale;            // 1.0f / hscale (cell_index_mode 1)
    int32_t rcp;                 // cell_index_mode
};

// stone-occupancy grid (built on the host at rover_set_stones): CSR lists of the stones that can matter per grid cell
struct StoneGridDev {
    const uint32_t* cell_start;  // [nx*ny + 1]
    const float4* stone_xyr;     // per list entry: (x, y, radius, stone id as float bits) — one independent 16-B load per stone
    float x0, y0, inv_cell;
    int32_t nx, ny;
};

struct PrepArgs {
    uint32_t E, P, R8;
    const float *pos, *quat, *joints, *target;
    const double* dist;          // [P][3]
    KnnDev terrain, rocks;
    RayRec* rays;                // [E*R8]
    float *euler, *heading;      // [E,3], [E]
    uint32_t* bin_out;           // optional [E*R8]: bin = (map, cell) key of every slot for the bucket sort (binned ray cast)
    uint32_t rocks_bin_offset;   // first bin of the rocks map (= terrain X*Y)
    int32_t precision;           // 0 fp32 mode; 1 fp16-rounded ray origins / directions; 2 as shipped (fp16 ray maths too)
    int32_t cell_rcp;            // cell_index_mode: 0 = (v - shift) / cell (ATen CPU), 1 = (v - shift) * (1 / cell) (ATen CUDA)
    const float* euler_in;       // optional [E,3]: the pose's euler angles as given (rover_get_depths) instead of quat -> euler
    // optional: the first pass of the bucket sort (bin_hist_fused) — counts[tile][bucket] += the block's keys per coarse bucket
    uint32_t* hist;              // [tiles][hist_buckets], all zero when the kernel starts (bucket_sort_kernel clears it again)
    uint32_t hist_low_bits, hist_buckets, hist_blocks_per_tile;     // a tile of the sort = the keys of this many 64-env blocks
};

// constants of the culled ray cast's rejection proof for the as-shipped fp16 arithmetic, derived from its one free parameter eta
struct CullProofH { double kappa, c_rho; float c_a, tau2; };
CullProofH cull_proof_h(double eta, double split);

struct LaneTables { float4* lvl; uint4* lrec; uint2* lid; };      // the staged ray cast's tables of one map for one proof (null: not built)

// raycast_culled_kernel (rover_cull.hip)
struct CullArgs {
    const RayRec* rays;
    const uint32_t* sorted;      // ray slots sorted by (map, cell)
    uint32_t n_sorted;
    uint32_t n_terrain;          // the first n_terrain sorted rays are terrain rays (bins are (map, cell): terrain first)
    const int32_t *idx0, *idx1;  // [cell][K8/4][4] triangle ids of the cell (-1 = empty slot)
    const uint4 *ctab0, *ctab1;  // [T] 16 B: bounding-sphere centre + scaled unit normal per triangle (phase 1)
    const uint16_t *rtab0, *rtab1; // [T] 20 B: the triangle's nine fp16 vertex components (exact arithmetic, phase 2)
    uint32_t kp0, kp1, run, n_blocks;
    float* out;                  // [E*R8] distances
    uint2* queue;                // candidate queue: one region of CULL_QCAP 8-byte entries per wave of a launch
    uint64_t queue_entries;      // its size: a step whose regions would not fit is cast in several launches
    int half;                    // the exact phase runs the reference's as-shipped fp16 arithmetic (ctab / qrow are then that proof's tables)
    float c_a_h, tau2_h;         // test constants of that proof (CullProofH)
    const float4 *far0, *far1;   // [cell][2]: the bound of the cell's far pairs (FarRec, rover_cull.hip) for the proof in force
    const float4 *near0, *near1; // [cell]: the same bound for the cell's near pairs (behind the far records in the same allocation)
    float k2_far;                // and the ray-side constant of the far skip
    int lazy_far;                // set up a bin's far pairs only when one of its rays tests them (few rays per bin)
    int skip_clear;              // (eager kernel) do not scan rays that clear their whole cell — the on-demand kernel always does
    uint4* stats;                // [waves] per-wave counters of the last launch {queue entries, rays, rays with both tests, bins}
};
// the staged ray cast (raycast variant 4, rover_cull.hip): lane = (ray, chunk of 8 pairs) over per-cell record rows in group-bound order
struct LaneArgs {
    const RayRec* rays;
    const uint32_t* sorted;
    uint32_t n_sorted, n_terrain;
    const float4* lvl[2];        // per map [cell][lane_lvl_stride()]: header, 16 suffix bounds (fp16), the suffixes' cones
    const uint4* lrec[2];        // [cell][2][pp]: pair records of test (A), then of test (B), in G order
    const uint2* lid[2];         // [cell][pp]: the pairs' triangle ids
    const uint16_t* rtab[2];
    uint32_t pp[2], run;
    float* out;
    uint4* stats;
    int half;                    // the tables are the as-shipped fp16 arithmetic's, the exact phase runs it
    float c_a_h, k2_far;         // test (A)'s constant of that proof; the level bound's ray-side constant (cull_far_k2)
    uint32_t forms;              // bit w (f32 proof) = map w's pair records are boxes (launch_lane_box), else two spheres; bit 2 + w = map w's tables are in shared-row form; bit 4 = the level loop measures a ray from where its line crosses the row's height ("lane_rebase")
    uint32_t y[2];               // per map: its Y (cell = ix * Y + iy), what the shared-row form finds a cell's row with
};
uint32_t lane_lvl_stride();
hipError_t launch_raycast_lane(LaneArgs a, hipStream_t s);

// n / d for every 32-bit n with a multiply-high and two shifts (Granlund & Montgomery's round-up method): the compiler's own
// expansion of a division by a run-time value is ~30 (32-bit) / ~110 (64-bit) dependent instructions per thread.
struct FastDiv {
    uint32_t m, s1, s2;
#if defined(__HIPCC__)
    __device__ __forceinline__ uint32_t div(uint32_t n) const {
        const uint32_t t = __umulhi(m, n);
        return (t + ((n - t) >> s1)) >> s2;
    }
#endif
};
inline FastDiv make_fastdiv(uint32_t d) {           // d >= 1
    uint32_t L = 0;
    while (L < 32 && (1ull << L) < d) ++L;
    FastDiv f;
    f.m = (uint32_t)((((1ull << L) - d) << 32) / d + 1ull);
    f.s1 = L < 1 ? L : 1; f.s2 = L > 1 ? L - 1 : 0;
    return f;
}

struct ObsArgs {
    uint32_t E, W, R8;
    FastDiv w_div;               // by W (filled in by launch_assemble_obs)
    int64_t obs_stride;
    const float *pos, *target, *heading, *lin_hist, *ang_hist, *dist;
    int32_t fp16_div;            // as-shipped mode: round dist / 2 to fp16
    const int32_t* obs_idx;      // [Ns+Nd] ray index per heightmap column
    float* obs;
};

struct MetricsArgs {
    uint32_t E, R8;
    int32_t curriculum_level, max_episode_length;
    int64_t num_envs_global;
    int do_increment, do_collision, do_metrics, do_done;
    float pos_reward, heading_contraint_reward, motion_contraint_reward, goal_angle_reward, boogie_contraint_reward;
    float wheel_thr, body_thr;   // rover.py:667-668 thresholds (0.8 / 0.45; their fp16 roundings in the as-shipped mode)
    const float *pos, *target, *joints, *lin_hist, *ang_hist, *euler_pre, *heading, *dist;
    int64_t* progress;
    int64_t* rock_collision;
    float* rew;
    int64_t* reset;
    uint32_t* block_cnt;         // optional [ceil(E/256)]: per-block done count for the compaction
    float* ex_pos_reward; int64_t* ex_collision; float *ex_upright, *ex_heading, *ex_motion, *ex_goal_angle, *ex_lin, *ex_ang;
    uint8_t* done_u8;            // optional: reset != 0 as one byte per env (the form that travels in the multi-GPU gather)
    int64_t* stone_collision;    // optional additional output: stone_info occupancy mask at pos_xy (collision stage)
    float stone_margin;
    StoneGridDev sgrid;
    const float* info7;
    // optional evaluation latch (rover_set_evaluation, rover.py:620-641,670-672): the host passes it to the collision stage at
    // curriculum level >= 2 and to the done stage only; null = off.  eval_step: progress at the step the code latched.
    int64_t* eval_res;
    int64_t* eval_step;
};

struct ResetArgs {
    const int64_t* ids;          // compacted reset ids (global)
    int64_t id_offset;           // env_offset: global -> local
    uint32_t n_host;
    const int32_t* n_dev;        // optional: count in device memory
    const float* initial_pos3;
    float *pos3, *quat4, *joint_pos13, *joint_vel13, *base_pos3;
    int64_t *reset, *progress;
    const int32_t* yaw_deg;      // optional [n]
    uint64_t seed;
    const uint64_t* seed_dev;    // optional [1]: added to seed on the device (a captured graph's step counter)
};

struct GoalArgs {
    const float* info7; uint32_t S; HeightDev h; StoneGridDev grid;
    const int64_t* env_ids; int64_t id_offset;
    uint32_t n_host; const int32_t* n_dev;
    const float* initial_pos3; float* target3; float radius;
    const float* draws; int32_t max_draws; uint64_t seed;
    const uint64_t* seed_dev;    // optional [1]: added to seed on the device
    int32_t* t_acc;              // [n] scratch: iteration at which entry i was accepted (-1: id 0 from the start)
    int32_t* n_draws_used;
};

struct PrePhysicsArgs {
    uint32_t E;
    const float *actions, *quat;
    float *lin_hist, *ang_hist, *euler_pre, *pos_targets13, *vel_targets13;
    float* actions_nn;           // optional [E,2,3]: self.actions_nn (rover.py:366), newest first
};

struct LinearArgs {
    const float* x; int64_t x_stride;      // [M, K] rows at x_stride floats
    const float* w; const float* b;        // nn.Linear: weight [N][K], bias [N] (optional)
    float* y; int64_t y_stride;            // [M, N] rows at y_stride floats
    int32_t M, K, N, act;                  // act: 0 none, 1 leakyrelu(0.01), 2 tanh, 3 relu, 4 elu
};
// the instantiation a layer runs (rover_mlp.hip): linear_act_kernel<nt, nw> on ny column tiles (grid.y); nw = 0: refused
struct LinearRoute { int nw, nt, ny; };
LinearRoute linear_route(int M, int N);
const char* linear_route_name(const LinearRoute& r);      // "linear_act<3,4>x2", or NULL
hipError_t launch_linear_act(const LinearArgs& a, hipStream_t s);
// Launches what a LinearRoute names, for the forward and for dgrad alike: launch(nt, nw, grid) with nt and nw as integral constants
// — <1..5, 4> or <1, 1> — on a grid of 32 nw-row slabs x r.ny; any other route is refused.
template <class Launch>
hipError_t launch_linear_route(int M, const LinearRoute& r, Launch&& launch) {
    if ((r.nw != 4 && r.nw != 1) || (r.nw == 1 && r.nt != 1)) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((M + 32 * r.nw - 1) / (32 * r.nw)), (uint32_t)r.ny);
    const std::integral_constant<int, 1> one{};
    const std::integral_constant<int, 4> four{};
    switch (r.nw == 1 ? 0 : r.nt) {
        case 0: launch(one, one, grid); break;
        case 1: launch(one, four, grid); break;
        case 2: launch(std::integral_constant<int, 2>{}, four, grid); break;
        case 3: launch(std::integral_constant<int, 3>{}, four, grid); break;
        case 4: launch(four, four, grid); break;
        case 5: launch(std::integral_constant<int, 5>{}, four, grid); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
// the same layer with bf16 operands (rover_bf16_tile.hip): one instantiation, linear_route's refusals; the name, or NULL
const char* linear_route_bf16_name(int M, int N);        // "linear_bf16<128,128>"
hipError_t launch_linear_bf16(const LinearArgs& a, hipStream_t s);

// One GRU layer for one time step (rover_gru_cell of the C ABI, validated; rover_gru.hip): torch.nn.GRU's cell, gates r, z, n
struct GruArgs {
    const float* x; int64_t x_stride;          // [M, K] rows at x_stride floats (unread when K = 0)
    const float* h_in; int64_t h_in_stride;    // [M, H]
    const float* w_ih; const float* w_hh;      // [3H][K], [3H][H]
    const float* b_ih; const float* b_hh;      // [3H] each, or NULL (zeros)
    const uint8_t* reset_mask;                 // [M] or NULL: a non-zero byte reads the row's h_in as zero
    float* h_out; int64_t h_out_stride;        // [M, H]; overlaps nothing the call reads
    int32_t M, K, H;
    float* gates; int64_t gates_stride;        // rover_gru_cell_train only: [M, 4H] = r | z | n | q (q = s_hn + b_hn); else NULL, unread
};
// the instantiation a cell runs: gru_cell_kernel<nw> on a grid of row slabs x 32-column tiles of the hidden state; nw = 0: refused
struct GruRoute { int nw; };
GruRoute gru_cell_route(int M, int K, int H);
const char* gru_cell_route_name(const GruRoute& r);       // "gru_cell<4>", or NULL
hipError_t launch_gru_cell(const GruArgs& a, hipStream_t s);                 // a.gates set: the training instantiation of the same route
// the same cell with bf16 operands and an f32 state (rover_bf16_tile.hip): one instantiation, gru_cell_route's refusals; no gates
const char* gru_cell_route_bf16_name(int M, int K, int H);       // "gru_cell_bf16<128,64>", or NULL
hipError_t launch_gru_cell_bf16(const GruArgs& a, hipStream_t s);

// The backward of one cell (rover_gru_cell_backward of the C ABI, validated; rover_gru.hip): dgi, dgh [M, 3H] and dh_in [M, H] from the
// gradient at h' (dh_above + dh_next), the gates the training forward stored and w_hh
struct GruBwdArgs {
    const float* dh_above; int64_t dh_above_stride;    // [M, H]
    const float* dh_next; int64_t dh_next_stride;      // [M, H] or NULL (zeros)
    const float* gates; int64_t gates_stride;          // [M, 4H] r | z | n | q
    const float* h_in; int64_t h_in_stride;            // [M, H]
    const uint8_t* reset_mask;                         // [M] or NULL
    const float* w_hh;                                 // [3H][H]
    float* dgi; int64_t dgi_stride;                    // [M, 3H]
    float* dgh; int64_t dgh_stride;                    // [M, 3H]
    float* dh_in; int64_t dh_in_stride;                // [M, H]
    int32_t M, H;
};
GruRoute gru_cell_backward_route(int M, int H);
const char* gru_cell_backward_route_name(const GruRoute& r);     // "gru_bwd<4>", or NULL
hipError_t launch_gru_cell_backward(const GruBwdArgs& a, hipStream_t s);

// out = add + mul * sigmoid(pre) over [M, N] (rover_gated_sum; rover_gru.hip); an input's row stride may be 0 (one row for all)
struct GatedSumArgs {
    const float* add; int64_t add_stride; const float* mul; int64_t mul_stride; const float* pre; int64_t pre_stride;
    float* out; int64_t out_stride;
    int32_t M, N;
};
hipError_t launch_gated_sum(const GatedSumArgs& a, hipStream_t s);
// its backward: d_mul = d_out s, d_pre = (d_out mul) (s (1 - s)), s = sigmoid(pre); each output optional, per row
struct GatedSumBwdArgs {
    const float* d_out; int64_t d_out_stride; const float* mul; int64_t mul_stride; const float* pre; int64_t pre_stride;
    float* d_mul; int64_t d_mul_stride; float* d_pre; int64_t d_pre_stride;
    int32_t M, N;
};
hipError_t launch_gated_sum_backward(const GatedSumBwdArgs& a, hipStream_t s);

// a chain of 2 or 4 layers in one kernel (rover_mlp.hip): y = L_n(... L_1(x)), L_i(v) = act_i(W_i v + b_i)
struct ChainArgs {
    const float* x; int64_t x_stride;      // [M, K0] rows at x_stride floats
    int32_t M, K0, n_layers;
    int32_t n[4];                          // output widths
    const float* w[4]; const float* b[4];  // nn.Linear: weight [n_i][n_{i-1}] (row-major, K0 for the first), bias [n_i] or NULL
    int32_t act[4];
    float* y; int64_t y_stride;            // [M, n_last] rows at y_stride floats
};
// which kernel runs a chain, decided once from M, K0, the widths and the activations (no pointer is read): split-k (a 2-layer chain
// at small batches, first layer split along k through a scratch buffer; tn output tiles, rt row tiles per wave), mlp_small (a 4-layer
// net at small batches) or chain16 with the tile shape the widths need; None: outside the built tile shapes
enum class ChainKernel { None, SplitK, MlpSmall, Chain16_5, Chain16_6, Chain16Long, Bf16_5, Bf16_6, Bf16Long };
struct ChainRoute { ChainKernel kernel; int tn, rt; };
ChainRoute chain_route(const ChainArgs& a);
// the same fit rule for precision = "bf16" (bf16 operands, f32 accumulation): chain_bf16<...> at every batch size, never split-k
// (the rounding its kernels apply to every operand: bf16_rne() of rover_bf16.h)
ChainRoute chain_route_bf16(const ChainArgs& a);
// "splitk<6,2>", "chain16<16,10,8,1>", ..., or NULL.  This and chain_act_route_name() read one table (rover_mlp.hip: kChainKernels) and
// compose the name in one buffer per thread: valid until the calling thread's next call of either
const char* chain_route_name(const ChainRoute& r);
// split-k: scratch holds chain_splitk_scratch_floats() floats
size_t chain_splitk_scratch_floats(int M, int K0, int n0);
hipError_t launch_chain(const ChainArgs& a, const ChainRoute& r, float* split_k_scratch, hipStream_t s);
// two split-k chains over the same rows in one launch per stage (+ an optional column copy), when chain_pair_side_by_side()
bool chain_pair_side_by_side(const ChainRoute& ra, const ChainRoute& rb);
hipError_t launch_chain_splitk_pair(const ChainArgs& a, const ChainArgs& b, const ChainRoute& r, float* scratch_a, float* scratch_b,
                                    const float* copy_src, int64_t copy_src_stride, float* copy_dst, int64_t copy_dst_stride, int copy_cols,
                                    hipStream_t s);

// The Gaussian policy head (rover_gauss_head of the C ABI, validated): actions = mean + exp(log_std') eps with counter-based noise,
// and the log-probability of the returned (or the taken) actions — one row per thread, in the last kernel of the actor's forward
// (chain16 / mlp_small "+gauss", A <= 4) or as a kernel of its own on a given mean.
#define GAUSS_MAX_A 16
enum GaussReduction { GAUSS_SUM = 0, GAUSS_MEAN = 1, GAUSS_PROD = 2, GAUSS_MAX = 3, GAUSS_MIN = 4, GAUSS_NONE = 5 };
struct GaussHead {
    const float* log_std;                  // [A]
    int32_t A, clip_log_std, clip_actions, reduction, deterministic;
    float min_log_std, max_log_std, low, high;
    uint64_t seed, step;
    const uint64_t* step_dev;              // optional [1]: added to step on the device (a captured graph's call counter)
    int64_t row_offset;                    // global row of local row 0 (a shard's env_offset)
    const float* taken; int64_t taken_stride;      // optional [M, A]: log_prob is evaluated at these instead of the returned actions
    float* actions; int64_t actions_stride;        // [M, A]
    float* log_prob; int64_t log_prob_stride;      // [M, 1], or [M, A] with GAUSS_NONE
};
// fused: the chain's last kernel carries the head (A <= 4 on mlp_small / chain16<16,10,8,1>); else forward, then the head's own launch
bool chain_head_fused(const ChainRoute& r, int A);
const char* chain_act_route_name(const ChainRoute& r, int A);     // "mlp_small+gauss", "chain16<16,10,8,1>;gauss", ..., or NULL
hipError_t launch_chain_head(const ChainArgs& a, const ChainRoute& r, const GaussHead& h, hipStream_t s);       // chain_head_fused() routes only
hipError_t launch_gaussian_head(const float* mean, int64_t mean_stride, int M, const GaussHead& h, hipStream_t s);
hipError_t launch_policy_noise(uint64_t seed, uint64_t step, const uint64_t* step_dev, int64_t row_offset, int M, int A, float* eps,
                               int64_t eps_stride, hipStream_t s);

// The exteroception noise on an observation matrix (rover_obs_noise of the C ABI, validated; rover_noise.hip): columns [0, first) are
// copied, every heightmap column c = col - first gets v = (in + (sigma_offset s) eo) + (sigma_point s) eps_c, or drop_value where the
// column's 24-bit word is below thr.  A sigma of 0 switches its term (and its draw) off; thr = 0 switches the dropout off.
struct ObsNoiseArgs {
    const float* in; int64_t in_stride;    // [M, F] rows at in_stride floats
    float* out; int64_t out_stride;        // [M, F]; out == in (and the same stride): in place, the first columns are then left alone
    int32_t M, F, first;
    float sigma_point, sigma_offset, drop_value;
    uint32_t thr;                          // llrint(dropout 2^24): 0 .. 2^24
    const float* row_scale;                // optional [M]
    const int64_t* episode;                // optional [M]
    uint64_t seed, step;
    const uint64_t* step_dev;              // optional [1]: added to step on the device
    int64_t row_offset;                    // global row of local row 0
};
hipError_t launch_obs_noise(const ObsNoiseArgs& a, hipStream_t s);

// The line-of-sight occlusion of the heightmap columns (rover_obs_occlusion of the C ABI, validated; rover_occlusion.hip): the definition
// is in include/rover_step.h.  body3, order and tilemax are rover_set_occlusion's tables.
#define OCC_TILE 8                         // nodes per side of a tile of the tile-max table
struct OcclusionArgs {
    HeightDev h;
    const float* tilemax;                  // [TN0][TN1]: max of hm * vscale over the tile's nodes, NaN ignored; -inf for a tile of NaNs
    int32_t TN0, TN1;                      // ceil(N0 / OCC_TILE), ceil(N1 / OCC_TILE)
    const float* body3;                    // [C][3] the columns' body points, f32
    const int32_t* order;                  // [C] a permutation of the columns (route 1)
    const float *pos3, *quat4;             // [M, 3], [M, 4]
    const float* clean; int64_t clean_stride;
    const float* in; int64_t in_stride;
    float* out; int64_t out_stride;        // out == in (and the same stride): in place, the first columns are then left alone
    uint8_t* hidden; int64_t hidden_stride;   // optional [M, C]
    float* target3;                        // optional [M, C, 3]
    int32_t M, F, first;
    float camera[3], step, clearance, miss, drop_value;
    int32_t max_steps;
    int32_t route;                         // 0 plain march, 1 ordered columns + tile table
};
hipError_t launch_obs_occlusion(const OcclusionArgs& a, hipStream_t s);
hipError_t launch_occlusion_tiles(const HeightDev& h, float* tilemax, int32_t TN0, int32_t TN1, hipStream_t s);

// skrl's RunningStandardScaler (rover_scaler_update / rover_scaler_apply of the C ABI, validated; rover_scaler.hip).  The plan's numbers
// come from rover_scaler_plan; `partials` points one double past the scratch's start (the header double keeps the count the call
// started from): three planes [n_chunks][N] of count, mean, M2.
#define SCALER_ROUTE_WIDE 0
#define SCALER_ROUTE_NARROW 1
#define SCALER_NARROW_MAX_N 8u             // narrow route (rows split over a workgroup's lanes) for N <= 8
struct ScalerUpdateArgs {
    const float* x; int64_t x_stride;      // [M, N] rows at x_stride floats
    uint32_t M, N, rows_per_chunk, n_chunks;
    double* partials;
    double *mean, *var, *count;            // [N], [N], [1]: the caller's state
    const int32_t* skip_if;                // optional [1]: nonzero when the kernel runs = the state stays unchanged
};
hipError_t launch_scaler_update(const ScalerUpdateArgs& a, int route, hipStream_t s);      // two launches: moments, fold
struct ScalerApplyArgs {
    const float* x; int64_t x_stride;
    float* y; int64_t y_stride;            // y == x (and the same stride): in place
    uint32_t M, N;
    const double *mean, *var;
    float epsilon, clip;
};
hipError_t launch_scaler_apply(const ScalerApplyArgs& a, bool inverse, hipStream_t s);

// The terrain-following motion model (rover_motion_step of the C ABI, validated; rover_motion.hip): `substeps` sub-steps of length dt on
// the poses in place, one thread per env, then the optional copy of the joint targets into the joint state.
#define MOTION_WHEELS 6
struct MotionArgs {
    HeightDev h;
    float *pos3, *quat4;                   // [E, 3], [E, 4] (w, x, y, z): read and written in place
    const float *lin, *ang;                // the env's commands at [e * cmd_stride]
    int32_t cmd_stride;
    uint32_t E;
    int32_t substeps;
    float dt, max_lin, max_ang, ride_height;
    float fit[3][MOTION_WHEELS];           // motion_plane_fit(): (z_c, p, q) = fit . z
    const float *joint_pos_targets13, *joint_vel_targets13;      // all four given, or all four NULL
    float *joint_pos13, *joint_vel13;
};
void motion_plane_fit(float out[3][MOTION_WHEELS]);       // host, double arithmetic rounded to f32 once: pinv([1, a_i, b_i])
hipError_t launch_motion(const MotionArgs& a, hipStream_t s);
// The rocker-bogie posture mode (rover_motion_step_bogie, validated): the same arguments (fit is not read), `iters` chord iterations with
// the constant inverse of the Jacobian at rest, the joint angles clamped to +-max_bogie into columns 0-2 of joint_pos13.
void motion_bogie_fit(float out[MOTION_WHEELS][MOTION_WHEELS]);      // host, double arithmetic rounded to f32 once: inv(dF/du at u = 0)
hipError_t launch_motion_bogie(const MotionArgs& a, int32_t iters, float max_bogie, hipStream_t s);
// The wheel-level drive mode (rover_motion_step_drive, validated): the same arguments — the commands and their scales are not read, the
// joint quadruple is always given —, rate-limited actuators on the joint state, the body twist fitted to the six wheel velocity vectors,
// and the posture of the plane (bogie = false: fit is read) or of the bogie solve (iters, max_bogie as above).
struct DriveArgs {
    float wheel_radius, steer_rate, wheel_accel;
    float* slip;                           // [E] or NULL
    bool bogie;
    int32_t iters;
    float max_bogie;
};
void motion_drive_fit(float out[3][2 * MOTION_WHEELS]);   // host, double arithmetic rounded to f32 once: pinv of the rigid-motion matrix
hipError_t launch_motion_drive(const MotionArgs& a, const DriveArgs& d, hipStream_t s);

// Episode statistics (rover_episode_track of the C ABI, validated; rover_track.hip): one env step's rewards, done flags and component
// columns folded into the per-env state, the window ring and the interval record; the definition is in include/rover_step.h.
#define TRACK_BLOCK 256
#define TRACK_MAX_COMP 16
struct TrackArgs {
    const float* rewards;                  // [E]
    const void* done;                      // [E] of 1 or 8 bytes
    int32_t done8;                         // 1: int64 flags
    uint32_t E, W, K;
    const void* comp[TRACK_MAX_COMP];      // K columns [E]
    uint32_t comp_i64;                     // bit k: column k is int64 (else f32)
    float* cum_reward;
    int32_t* cum_steps;
    float* ring_ret;
    int32_t* ring_len;
    int64_t* ring_count;
    void* record;                          // rover_track_record
    void* scratch;                         // track_scratch_bytes(E), 8-byte aligned: the partials, then the finished returns, then the lengths
};
uint32_t track_partial_bytes();
static inline uint32_t track_partials(uint32_t E) { return (uint32_t)(((uint64_t)E + TRACK_BLOCK - 1) / TRACK_BLOCK); }
static inline uint64_t track_scratch_bytes(uint32_t E) { return (uint64_t)track_partials(E) * ((uint64_t)track_partial_bytes() + 8ull * TRACK_BLOCK); }
hipError_t launch_track(const TrackArgs& a, hipStream_t s);

// The heightfield of a triangle mesh (rover_build_heightfield of the C ABI, validated; rover_raster.hip): snap the vertices, scatter every
// triangle into the nodes of its box (small boxes by a lane group, large ones listed and rasterised per tile by a second launch), decode.
#define RASTER_SUB 256                     // sub-units per node spacing
#define RASTER_MAX_SNAP (1 << 25)          // largest |X|, |Y| of a snapped vertex: every edge function stays within 2^53
#define RASTER_MAX_NODES 131072            // largest N0, N1: 256 (N - 1) < 2^25
#define RASTER_GROUP 16                    // lanes per triangle on the small route
#define RASTER_SMALL_NODES 512             // largest box (nodes) of the small route
#define RASTER_TILE_I 32                   // the large route's tile: rows (4 waves x 8) ...
#define RASTER_TILE_J 64                   // ... x consecutive j (one per lane)
struct RasterArgs {
    const void* snap;                      // [V] 16-byte snapped vertices (launch_raster_snap)
    const int32_t* tris;                   // [T, 3]
    int32_t V, T, N0, N1;
    uint32_t* keys;                        // [N0][N1]: hm_out while it holds keys (all 0 before the first triangle)
    uint32_t* n_large;                     // [1] length of the list
    uint32_t* large_tri;                   // [T] the listed triangles ...
    uint32_t* large_tiles;                 // [T] ... and how many tiles each one's box touches
    unsigned long long* stats;             // [2] {uncovered nodes, skipped triangles}
};
hipError_t launch_raster_snap(const float* vertices, uint32_t V, float hs, float shift_x, float shift_y, void* snap, hipStream_t s);
hipError_t launch_raster_small(const RasterArgs& a, hipStream_t s);
hipError_t launch_raster_large(const RasterArgs& a, const uint64_t* tile_start, uint32_t n_large, uint64_t total, hipStream_t s);
hipError_t launch_raster_decode(uint32_t* keys, uint64_t n, float fill, unsigned long long* stats, hipStream_t s);

// The Mars terrain generator's heightfield (rover_mars_heightfield of the C ABI, validated; rover_mars.hip): one workgroup per
// MARS_TILE^2 nodes adds the hills, then walks the tile's stamp list (built on the host) in ascending order through LDS.
#define MARS_TILE 16                       // = ROVER_MARS_TILE
#define MARS_CHUNK 128                     // stamp records staged in LDS at a time (4 KiB)
struct MarsHill { int32_t r0, r1, c0, c1, a0, b0; double amp; };       // rows r0 .. r1 - 1, columns c0 .. c1 - 1; g from a0 / b0
struct MarsStamp { int32_t row, col; uint32_t side, table; double factor, pad; };      // table: the class table's first element
static_assert(sizeof(MarsHill) == 32 && sizeof(MarsStamp) == 32, "Mars records must be 32 bytes");
struct MarsArgs {
    double* hf; uint8_t* mask;             // [rows][cols]; mask may be null
    int32_t rows, cols;
    uint32_t tiles_r, tiles_c;
    const MarsHill* hills; int32_t n_hills;
    const double* g;
    const double* tables;
    const MarsStamp* stamps;               // [n_stamps], indexed by stamp id (dropped stamps hold zeros and are in no list)
    const int32_t* tile_start;             // [tiles_r tiles_c + 1]
    const int32_t* tile_items;
};
hipError_t launch_mars_heightfield(const MarsArgs& a, hipStream_t s);

// Generalised advantage estimation over a stored rollout (rover_gae of the C ABI, validated; rover_rollout.hip): rows are time steps at
// a stride in elements, the env stride is 1.
enum GaeNormalize { GAE_RAW = 0, GAE_NORMALIZE = 1, GAE_NORMALIZE_GIVEN = 2 };
constexpr uint32_t GAE_MAX_BLOCKS = 2048;  // most blocks of the scan = most (count, mean, M2) partials: the ctx holds 3 doubles for each
struct GaeArgs {
    int32_t T; uint32_t E;
    float gamma, lam;
    const float* rewards; int64_t rewards_stride;
    const float* values; int64_t values_stride;
    const uint8_t* dones; int64_t dones_stride;
    const float* last_values;              // [E]
    float* returns; int64_t returns_stride;            // may alias values
    float* advantages; int64_t advantages_stride;
    int32_t normalize;                     // GaeNormalize
    double* stats_out;                     // optional [3]: (count, mean, M2) of this call's raw A
    const double* stats_in;                // [3], GAE_NORMALIZE_GIVEN
    double* partials;                      // [GAE_MAX_BLOCKS][3], the ctx's
};
int gae_launches(const GaeArgs& a);        // 0 (E = 0), 1 (the scan) or 2 (+ the finishing kernel: own moments needed)
hipError_t launch_gae(const GaeArgs& a, hipStream_t s);
void gae_combine_moments(const double* a, const double* b, double* out);   // host: Chan's update, the one the kernels run

// The backward of one Layer (rover_linear_backward of the C ABI, validated; rover_train.hip): dz = dy act'(y), dx = dz W, dW = dz^T x,
// db = column sums of dz; every output optional (null).
struct LinearBwdArgs {
    const float* x; int64_t x_stride;      // [M, K]
    const float* y; int64_t y_stride;      // [M, N] the layer's output as the forward wrote it (unused with act 0)
    const float* dy; int64_t dy_stride;    // [M, N]
    const float* w;                        // [N][K]
    float* dx; int64_t dx_stride;          // [M, K]
    float* dw; float* db;                  // [N][K], [N]
    int32_t M, K, N, act;
};
// what a backward launches: linear_wgrad_kernel<nt, nw> over `splits` cuts of M of rows_per_split rows each (+ the merge when
// splits > 1), and for dx linear_dgrad_kernel on the forward's route of an M x K output (dx.nw = 0: no dx); ok = false: refused
struct LinearBwdRoute { bool ok; int nt, nw, splits, rows_per_split; LinearRoute dx; };
LinearBwdRoute linear_backward_route(int M, int K, int N, bool want_dx);
const char* linear_backward_route_name(const LinearBwdRoute& r);      // "wgrad<3,4>/64;dgrad<1,4>", or NULL; valid until the thread's next call
size_t linear_backward_scratch_floats(const LinearBwdRoute& r, int K, int N);
hipError_t launch_linear_backward(const LinearBwdArgs& a, const LinearBwdRoute& r, float* scratch, hipStream_t s);
// dx alone for any N >= 1 and K >= 1 (rover_linear_dgrad): linear_dgrad_kernel<nt, nw> on ny column tiles of dx; nw = 0: refused
LinearRoute linear_dgrad_route(int M, int N, int K);
const char* linear_dgrad_route_name(const LinearRoute& r);      // "dgrad<2,4>x5", or NULL; valid until the thread's next call
hipError_t launch_linear_dgrad(const LinearBwdArgs& a, const LinearRoute& r, hipStream_t s);

// The PPO minibatch loss and its gradients at the nets' outputs (rover_ppo_loss of the C ABI, validated; rover_train.hip)
constexpr uint32_t PPO_MAX_BLOCKS = 1024;  // most blocks = most partials of 3 + GAUSS_MAX_A doubles: the ctx holds them since rover_create
struct PpoArgs {
    int32_t M, A;
    const float* mean; int64_t mean_stride;
    const float* log_std;
    const float* actions; int64_t actions_stride;
    const float *old_log_prob, *advantages, *value, *old_values, *returns;
    int32_t clip_log_std; float min_log_std, max_log_std;
    float ratio_clip, value_clip; int32_t clip_predicted_values;
    float entropy_loss_scale, value_loss_scale;
    float* d_mean; int64_t d_mean_stride;
    float *d_value, *d_log_std;
    double* stats;                         // [4] policy_loss, value_loss, entropy_loss, kl
    double* partials;                      // [PPO_MAX_BLOCKS][3 + GAUSS_MAX_A], the ctx's
};
hipError_t launch_ppo_loss(const PpoArgs& a, hipStream_t s);

// Gradient-norm clip + Adam over a list of tensors (rover_optim_* of the C ABI, validated; rover_optim.hip)
constexpr uint32_t OPTIM_CHUNK = 1024;     // elements of one chunk = of one workgroup: THE chunk length (optim_plan, both kernels)
struct OptimChunkHost { int32_t tensor, first, length; };
// the chunks of tensors of numel[i] elements in tensor order, then element order; a tensor of 0 elements yields none.  -> the count;
// writes at most `capacity` records (out may be NULL with capacity 0).  Host only, no device.
int64_t optim_plan(int32_t n_tensors, const int64_t* numel, OptimChunkHost* out, int64_t capacity);
enum OptimChunkFlags { OPTIM_PG_ALIGNED = 1, OPTIM_STATE_ALIGNED = 2 };      // 16-byte loads / stores of (p, g) and of (m, v)
struct OptimChunk {                        // the device table's record (32 B)
    float* p; const float* g;              // the chunk's first parameter and gradient element
    uint32_t state;                        // its first element in exp_avg / exp_avg_sq
    uint32_t len, flags, pad;
};
static_assert(sizeof(OptimChunk) == 32, "OptimChunk must be 32 bytes");
struct OptimRecord { int64_t step; int32_t stopped, pad; };      // what prepare leaves for apply: the step in force, the decision
struct OptimArgs {
    const OptimChunk* chunks; uint32_t n_chunks;
    double* partials;                      // [n_chunks] sums of g*g
    OptimRecord* record;
    float *exp_avg, *exp_avg_sq;
    int64_t* step; int32_t* stopped;
    double lr, beta1, beta2, eps, clip;
    const double* gate; double gate_threshold;
    double* norm_out;
};
hipError_t launch_optim_step(const OptimArgs& a, hipStream_t s);          // two launches: prepare, apply

// blocks of bs threads (or items) that cover n: the launchers' grid sizes
static inline uint32_t blocks_for(uint64_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }

// rover_rays.hip
hipError_t launch_repack(const int32_t* map_idx, const int32_t* tris, const uint16_t* verts, uint64_t n_cells, uint32_t K,
                         uint32_t K8, uint32_t T, uint32_t V, uint16_t* table, hipStream_t s);
hipError_t launch_prep(const PrepArgs& a, hipStream_t s);
hipError_t launch_raycast(const RayRec* rays, uint32_t n_rays, const uint16_t* tab0, const uint16_t* tab1, uint32_t kp0,
                          uint32_t kp1, float* out, hipStream_t s);
hipError_t launch_raycast_binned(const RayRec* rays, const uint32_t* sorted, uint32_t n_sorted, const uint16_t* tab0,
                                 const uint16_t* tab1, uint32_t kp0, uint32_t kp1, uint32_t run, bool fp16_math, uint32_t early_out, float* out,
                                 hipStream_t s);
hipError_t launch_export_dist(const float* dist, const RayRec* rays, uint32_t E, uint32_t R8, uint32_t P, int precision, float* ray_dist,
                              float* wheel, float* body, float* ray_src, float* hit_pt, hipStream_t s);
hipError_t launch_export_rays(const RayRec* rays, const float* dist, uint32_t E, uint32_t R8, uint32_t P, float* src, float* dir, int32_t* cell,
                              float* out_dist, hipStream_t s);
hipError_t launch_import_rays(const float* src, const float* dir, uint32_t E, uint32_t R8, uint32_t P, const KnnDev& terrain, const KnnDev& rocks,
                              uint32_t rocks_bin_offset, int precision, int cell_rcp, RayRec* rays, uint32_t* bin_out, hipStream_t s,
                              uint32_t* not_unit = nullptr /* optional: counts the finite directions whose length is not 1 */);
// rover_sort.hip
// packed: one-dword sort entries (bin_entries_packed(n_slots, low_bits): the plan's sort_entry_dwords == 1)
hipError_t launch_bin_rays(const uint32_t* bins, uint32_t n_slots, uint32_t n_valid, uint32_t n_bins, uint32_t low_bits, bool packed,
                           uint32_t* table, uint2* pairs, uint32_t* block_sums, uint32_t* sorted, bool hist_done, hipStream_t s);
hipError_t launch_scan_exclusive(uint32_t* data, uint32_t n, uint32_t* block_sums, hipStream_t s);
// rover_obs.hip
hipError_t launch_assemble_obs(const ObsArgs& a, hipStream_t s);
hipError_t launch_obs_metrics(const ObsArgs& o, const MetricsArgs& m, hipStream_t s);     // both in one launch (rover_step)
hipError_t launch_metrics_done(const MetricsArgs& a, hipStream_t s);
hipError_t launch_compact(const int64_t* reset, uint32_t n, int64_t offset, uint32_t* block_cnt, bool counted, int64_t* ids,
                          int32_t* count, hipStream_t s);
hipError_t launch_eval_summary(const int64_t* eval_res, const int64_t* eval_step, uint32_t E, int64_t* summary8, hipStream_t s);
hipError_t launch_eval_clear(int64_t* eval_res, int64_t* eval_step, uint32_t E, const int64_t* ids, uint32_t n, hipStream_t s);
// rover_reset.hip
hipError_t launch_quat_to_euler(const float* q, float* eul, uint32_t n, hipStream_t s);
hipError_t launch_clearance(const float* info7, uint32_t S, const float* xy, uint32_t n, float* out, hipStream_t s);
hipError_t launch_shift_spawns(const StoneGridDev& g, const float* info7, float* pos3, uint32_t n, int32_t max_iter, hipStream_t s);
hipError_t launch_sample_height(const HeightDev& h, const float* xy, uint32_t n, float* out, hipStream_t s);
hipError_t launch_generate_goals(const GoalArgs& a, uint32_t n_max, hipStream_t s);
hipError_t launch_reset_envs(const ResetArgs& a, uint32_t n_max, hipStream_t s);
hipError_t launch_pre_physics(const PrePhysicsArgs& a, hipStream_t s);
hipError_t launch_ackermann(const float* lin, const float* ang, uint32_t n, float* steer, float* vel, hipStream_t s);
// rover_knn.hip
hipError_t launch_knn_centroids(const float* verts, const int32_t* tris, uint32_t T, uint32_t V, int ref, float* cx, float* cy,
                                hipStream_t s);
hipError_t launch_knn_bucket(const float* cx, const float* cy, uint32_t T, float ox, float oy, float inv_g, uint32_t nbx, uint32_t nby,
                             uint32_t* cursor, uint32_t* items, int count, hipStream_t s);
hipError_t launch_knn_select(const float* cx, const float* cy, const uint32_t* bucket_start, const uint32_t* items, float ox, float oy,
                             float g, float span, uint32_t nbx, uint32_t nby, uint32_t X, uint32_t Y, float res, uint32_t K,
                             const float* cell_x, const float* cell_y, int32_t* out, int32_t* overflow, hipStream_t s);
// rover_cull.hip
hipError_t launch_tri_centroids(const int32_t* tris, const uint16_t* verts, uint32_t T, uint32_t V, float2* out, hipStream_t s);
// the tables of the culled and staged ray casts for one map (launch_cull_build, rover_cull.hip)
struct CullBuildArgs {
    const int32_t* map_idx;      // [cell][K] the caller's triangle ids
    const int32_t* tris;         // [T][3]
    const uint16_t* verts;       // [V][3] fp16
    uint64_t n_cells;
    uint32_t K, K8;
    uint32_t T, T_int, V;        // T: the caller's triangle count (ids in map_idx); T_int: slots of the internal numbering
    const uint32_t *order, *newid;   // [T_int] internal id -> caller's (0xffffffff = hole), [T] caller's id -> internal
    int32_t* idx4;               // [cell][K8/4][4] internal triangle ids (both proofs)
    uint16_t* rtab;              // [T_int] 20 B: nine fp16 vertex components (both proofs)
    uint4 *ctab, *ctab_h;        // [T_int] per proof: f32 / as-shipped fp16 (CullK<1>)
    uint32_t *qrow, *qrow_h;     // [cell] per proof, read only by the build kernels
    float4 *far, *far_h;         // [cell][2] far-pair bounds, then [cell] near-pair bounds, per proof
    float* nz_scratch;           // [T_int]
    uint32_t* counts;            // [8], zeroed: [7] the largest union of a shared row, in pairs (launch_lane_union); [0..6] always-candidate triangles, cells without a cone; the same for fp16; cells with a useful far bound; non-empty and well-filled pairs (f32 staged tables)
    CullProofH ph;
    uint32_t Y;
    float cell_size, shift_x, shift_y;
    LaneTables lane, lane_h;     // the staged kernel's tables per proof (null: not built)
};
hipError_t launch_cull_build(const CullBuildArgs& a, hipStream_t s);
// The form of test (A)'s records in the f32 proof's staged tables: launch_cull_build builds spheres and leaves the map's non-empty and
// well-filled pairs in counts[5], counts[6]; where lane_box_share_met, launch_lane_box builds the same tables again as boxes.
bool lane_box_share_met(uint64_t pairs, uint64_t well_filled);
hipError_t launch_lane_box(const CullBuildArgs& a, hipStream_t s);
// Shared-row form of a map's staged tables, both proofs: one row per two cells that neighbour in iy.  launch_lane_union leaves
// the rows' unions in upair [lane_pair_rows_count][128] and the largest one in counts[7]; lane_pair_rows_pp gives the pairs per row for it,
// or 0 where a union does not fit a row (the map then keeps its per-cell tables); launch_lane_pair_rows builds the tables.
uint64_t lane_pair_rows_count(uint64_t n_cells, uint32_t Y);
uint32_t lane_pair_rows_pp(uint32_t max_union_pairs);
hipError_t launch_lane_union(const CullBuildArgs& a, uint2* upair, hipStream_t s);
hipError_t launch_lane_pair_rows(const CullBuildArgs& a, const uint2* upair, uint32_t pp, int box, hipStream_t s);
float cull_far_k2(int half, CullProofH ph);
hipError_t launch_raycast_culled(CullArgs a, hipStream_t s);

}  // namespace rover
