// rover_ctx.h — what the units of the C-ABI layer (rover_capi*.cpp) share: the ctx and the owners of its device tables, the device guard,
// the error helpers.  Private and host only: the kernel files do not include it.
#pragma once
#include "../../include/rover_step.h"
#include "rover_internal.h"
#include "rover_operands.h"
#include "rover_plan.h"

#include <string>
#include <vector>

using namespace rover;

// One hipMalloc allocation, owned: freed when the owner is reset, replaced or destroyed (on the ctx's device: every entry point that can
// free holds a DeviceGuard).  Move-only.
template <typename T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    // n elements in place of what the buffer held; on failure it holds nothing and the runtime's sticky error is cleared
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) { (void)hipGetLastError(); p_ = nullptr; return e; }
        n_ = n;
        return e;
    }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    T* get() const { return p_; }
    uint64_t bytes() const { return (uint64_t)n_ * sizeof(T); }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// The tables of one map for one rejection proof: proof 0 is the f32 one (ray_precision 0 / 1), proof 1 the as-shipped fp16 arithmetic's
// (ray_precision 2).  The culled ray cast (variant 3) reads ctab and far; the staged one (variant 4) lvl / lrec / lid, which are optional.
struct ProofTables {
    DevBuf<uint4> ctab;                 // [T_int] bounding-sphere centre + scaled unit normal per triangle (16 B)
    DevBuf<float4> far;                 // [cell][2] far-pair bounds, then [cell] near-pair bounds
    DevBuf<float4> lvl;                 // staged: [cell][lane_lvl_stride()] header, suffix bounds, the suffixes' cones
    DevBuf<uint4> lrec;                 // staged: [cell][2][pp] pair records of tests (A) and (B) in group-bound order
    DevBuf<uint2> lid;                  // staged: [cell][pp] the pairs' triangle ids
    int64_t always = 0, nocone = 0;     // always-candidate triangles, cells without a cone (counted when the tables were built)
    LaneTables view() const { return LaneTables{lvl.get(), lrec.get(), lid.get()}; }
};

// Everything rover_set_knn_map builds for one map; built whole, then moved into the ctx in one assignment
struct MapTables {
    DevBuf<uint16_t> table;             // re-packed map, per-cell contiguous fp16 block [X*Y][9][K8]
    KnnDev knn{};                       // its geometry; knn.table = table.get()
    DevBuf<int32_t> cull_idx;           // culled / staged ray cast: [cell][K8] the cell's triangles in the internal numbering (null: not built)
    DevBuf<uint16_t> rtab;              // [T_int] the nine fp16 vertex components of a triangle (20 B)
    ProofTables proof[2];
    uint32_t lane_pp = 0;               // pairs per row of the staged kernel's records
    bool lane_box = false;              // the f32 proof's staged records are boxes (one per pair), not two spheres
    bool lane_pair_rows = false;        // the staged tables (both proofs) hold one row per two cells that neighbour in iy (lane_pp pairs: their union)
    int64_t tris = 0, farok = 0, cells = 0;   // triangles; cells whose far bound can hold for a usual ray (far_build_kernel); cells
    uint64_t bytes() const {
        uint64_t b = table.bytes() + cull_idx.bytes() + rtab.bytes();
        for (const ProofTables& p : proof) b += p.ctab.bytes() + p.far.bytes() + p.lvl.bytes() + p.lrec.bytes() + p.lid.bytes();
        return b;
    }
};

// The candidate queue of the culled / staged ray cast and its per-wave counters, with the two facts the steps check about them
struct CullQueue {
    DevBuf<uint2> entries;              // one region of 1 024 entries per wave of a launch
    DevBuf<uint4> stats;                // per-wave counters of the last culled launch (rover_get_cull_info)
    StepPlan sized_for{};               // the plan both were sized for (alloc_cull_queue)
    StepPlan counters_written_under{};  // the plan the counters were last written under (run_raycast)
};

// One rover_optim_create: the ctx owns the chunk table, the partials and the record; the tensors and the state are the caller's
struct OptimHandle {
    bool live = false;
    DevBuf<OptimChunk> chunks;          // [n_chunks] (optim_plan's chunks with their addresses)
    DevBuf<double> partials;            // [n_chunks] sums of g*g
    DevBuf<OptimRecord> record;         // [1] what the prepare launch leaves for the apply launch
    uint32_t n_chunks = 0;
    float *exp_avg = nullptr, *exp_avg_sq = nullptr;
    int64_t* step = nullptr;
    int32_t* stopped = nullptr;
    std::vector<Span> spans;            // everything the step reads or writes through the handle (norm_out must stay clear of it)
};

// Everything rover_set_occlusion derives, under one validity key: the counters of rover_set_distribution and rover_set_heightfield it was
// built under.  rover_obs_occlusion runs only while both still stand.
struct OcclusionTables {
    bool set = false;
    rover_occlusion_cfg cfg{};
    DevBuf<float> body3;                // [C][3] the columns' body points, f64 rounded to f32 once
    DevBuf<int32_t> order;              // [C] rover_occlusion_order
    DevBuf<float> tilemax;              // [TN0][TN1] maxima of the OCC_TILE x OCC_TILE-node tiles of the heightfield
    int32_t TN0 = 0, TN1 = 0;
    uint64_t dist_gen = 0, hf_gen = 0;  // the key
};

struct rover_ctx {
    rover_cfg cfg{};
    std::string err;
    MapTables maps[2];                  // terrain, rocks
    Knobs knobs{};                      // what rover_set_option / the ROVER_* environment set (the knob table below)
    StepPlan plan{};                    // the step in force (replan): what runs and what the plan-dependent buffers are sized for
    StepPlan ws_plan{};                 // the plan the ray workspace was produced with (cast_rays): the sorted list, rover_get_cull_info
    CullQueue queue;
    // distribution
    DevBuf<double> d_dist;          // [P][3]
    DevBuf<int32_t> d_obs_idx;      // [Ns+Nd]
    int32_t P = 0, Ns = 0, Nd = 0;
    bool have_dist = false;
    // heightfield / stones (hf and sgrid: the kernels' views of the owners beside them)
    DevBuf<float> d_hm;
    HeightDev hf{};
    bool have_hf = false;
    DevBuf<float> d_stones;         // [S][7]
    int32_t S = 0;
    DevBuf<uint32_t> d_grid_start;
    DevBuf<float4> d_grid_xyr;
    StoneGridDev sgrid{};
    bool have_stones = false;
    uint64_t dist_gen = 0, hf_gen = 0;  // advanced by rover_set_distribution / rover_set_heightfield: the validity key of derived tables
    OcclusionTables occ;                // rover_set_occlusion
    int32_t occlusion_route = 1;        // option "occlusion_route": 0 plain march, 1 ordered columns + tile-max table (results do not depend on it)
    // per-step workspace
    DevBuf<RayRec> d_rays;
    DevBuf<float> d_dist_out;       // [E*R8]
    DevBuf<float> d_euler;          // [E,3]
    DevBuf<float> d_heading;        // [E]
    DevBuf<int64_t> d_ids_work;     // [E]
    DevBuf<uint32_t> d_goal_work;   // [2][E] work lists of generate_goals
    DevBuf<uint32_t> d_block_cnt;   // [ceil(E/256)] + a spare word
    // ray binning (raycast variant 2)
    DevBuf<uint32_t> d_bins;            // [E*R8] bin key per slot
    DevBuf<uint32_t> d_bkt_table;       // [n_buckets * n_blocks] counts -> offsets
    bool bkt_table_dirty = true;        // not known to be all zero (what prep_rays_kernel's fused histogram starts from): a step failed half way
    DevBuf<uint2> d_pairs;              // [E*R8] (bin, slot) after the coarse partition
    int precision = 0;                  // option "ray_precision": 0 fp32 mode, 1 fp16 sources, 2 as shipped (fp16 maths)
    DevBuf<uint32_t> d_block_sums;      // [4096] bucket totals + [4097] bucket starts
    DevBuf<uint32_t> d_sorted;          // [E*R8] ray slots sorted by (map, cell)
    int32_t cell_rcp = 0;               // option "cell_index_mode": 0 cpu_div (x / 0.1), 1 cuda_rcp (x * (1 / 0.1))
    int32_t lane_rebase = 1;            // option "lane_rebase": the staged kernel's level loop measures a ray from the point where its line crosses the row's height (bit 4 of LaneArgs::forms; results do not depend on it)
    // all the learning entry points (rover_capi_learn.cpp) keep in the ctx; they touch no member but this one
    struct {
        DevBuf<float> mlp_scratch;          // partial sums of the split-k small-batch encoder path (rover_mlp_chain_forward)
        DevBuf<double> gae_partials;        // [GAE_MAX_BLOCKS][3] per-block (count, mean, M2) of rover_gae, sized once at rover_create
        DevBuf<double> ppo_partials;        // [PPO_MAX_BLOCKS][3 + GAUSS_MAX_A] per-block sums of rover_ppo_loss, sized once at rover_create
        std::vector<OptimHandle> optims;    // rover_optim_create's handles, by number (a destroyed one's slot is given out again)
    } learn;
    uint64_t workspace_bytes = 0;
    bool ws_ok = false, bins_ok = false;   // false after a failed (re)allocation: the step entry points refuse to run
    bool rays_valid = false;            // the ray workspace holds a finished ray cast (rover_replay_raycast)
    bool obs_valid = false;             // ... and euler / heading hold the state of a rover_get_observations (rover_calculate_metrics reads them)
    // evaluation mode (rover_set_evaluation): per-env outcome code and the progress at which it latched
    DevBuf<int64_t> d_eval_res;         // [E] 0 pending, 1 collided / out of area, 2 reached goal, 3 timed out
    DevBuf<int64_t> d_eval_step;        // [E]
    bool eval_on = false;
    // in-situ ray-cast timing (rover_set_profiling)
    bool profiling = false;
    int32_t prof_every = 1;             // time every prof_every-th ray-cast launch (an event pair costs ~12 us of stream time)
    int32_t prof_seen = 0;              // launches since profiling was switched on
    std::vector<hipEvent_t> ev0, ev1;
    int32_t prof_launches = 0;
    double prof_ms = 0.0;
    int32_t prof_pending = 0;
};

// Defined once, in rover_capi.cpp: records the message with c, or for rover_last_error(NULL) when c is null, and returns code.
int fail(rover_ctx* c, int code, const char* fmt, ...);

// Each learning entry point lists its arrays as an operand table (rover_operands.h), which applies the operand rules of rover_step.h; the ctx is looked at last
// (`need_ctx`: here), so every refusal is reached with a NULL ctx too and reports through rover_last_error(NULL).
// (inline: it is on the path of every call, rover_gru_cell's thousands per BPTT pass among them)
static inline int check_operands(rover_ctx* c, Operands& ops, bool need_ctx = true) {
    char why[512];
    if (ops.refused(why, sizeof why)) return fail(c, ROVER_E_INVALID, "%s", why);
    return need_ctx && !c ? fail(nullptr, ROVER_E_INVALID, "%s: null ctx", ops.entry()) : ROVER_OK;
}

#define HIP_TRY(c, expr)                                                                         \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) return fail((c), ROVER_E_HIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// Makes the ctx's device current for the duration of one entry point and restores the caller's device afterwards
// (the reference's task pins everything to one device, rover.py:90; a library must not change the caller's).
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t err;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            changed = err == hipSuccess;
        }
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define USE_DEVICE(c)                                                                                          \
    DeviceGuard device_guard__((c)->cfg.device);                                                               \
    if (device_guard__.err != hipSuccess)                                                                      \
        return fail((c), ROVER_E_HIP, "hipSetDevice(%d): %s", (c)->cfg.device, hipGetErrorString(device_guard__.err))
