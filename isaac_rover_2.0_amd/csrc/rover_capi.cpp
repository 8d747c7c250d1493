// rover_capi.cpp — C-ABI layer of librover_step.so (include/rover_step.h): context, library-owned device
// tables, argument checks, kernel sequencing.  No torch, no exceptions across the boundary.
#include "../../include/rover_step.h"
#include "rover_internal.h"
#include "rover_bf16.h"
#include "rover_philox.h"
#include "rover_operands.h"
#include "rover_plan.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
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
    DevBuf<float> d_mlp_scratch;        // partial sums of the split-k small-batch encoder path (rover_mlp_chain_forward)
    DevBuf<double> d_gae_partials;      // [GAE_MAX_BLOCKS][3] per-block (count, mean, M2) of rover_gae, sized once at rover_create
    DevBuf<double> d_ppo_partials;      // [PPO_MAX_BLOCKS][3 + GAUSS_MAX_A] per-block sums of rover_ppo_loss, sized once at rover_create
    std::vector<OptimHandle> optims;    // rover_optim_create's handles, by number (a destroyed one's slot is given out again)
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

static const int kProfRing = 256;

static int prof_drain(rover_ctx* c) {
    for (int i = 0; i < c->prof_pending; ++i) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(c->ev1[i]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0[i], c->ev1[i]);
        if (e != hipSuccess) { c->prof_pending = 0; return ROVER_E_HIP; }
        c->prof_ms += ms;
    }
    c->prof_pending = 0;
    return ROVER_OK;
}

static thread_local std::string g_create_err;

static int fail(rover_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
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

static bool have_maps(const rover_ctx* c) { return c->maps[0].table.get() && c->maps[1].table.get(); }

// What plan_step reads, from the ctx: the only place that reads it for planning
static PlanInputs plan_inputs(const rover_ctx* c) {
    PlanInputs in;
    in.num_envs = c->cfg.num_envs; in.P = c->P; in.have_dist = c->have_dist; in.precision = c->precision; in.knobs = c->knobs;
    for (int w = 0; w < 2; ++w) {
        const MapTables& m = c->maps[w];
        MapShape& s = in.map[w];
        s.present = m.table.get() != nullptr;
        s.X = m.knn.X; s.Y = m.knn.Y; s.K8 = m.knn.K8; s.cells = m.cells; s.farok = m.farok;
        s.has_cull_tables = m.cull_idx.get() != nullptr;
        for (int k = 0; k < 2; ++k) s.has_staged_tables[k] = m.proof[k].lrec.get() != nullptr;
    }
    return in;
}

static uint32_t bucket_count(const StepPlan& p) { return (uint32_t)((p.n_bins + (1u << p.low_bits) - 1u) >> p.low_bits); }

// the sort's tables, for the bins and the digit the plan says
static int alloc_bins(rover_ctx* c) {
    const StepPlan& p = c->plan;
    c->bins_ok = false;
    if (!have_maps(c)) return ROVER_OK;
    if (p.n_bins > 0xfffffffeull) return fail(c, ROVER_E_INVALID, "too many map cells for ray binning");
    if (!c->d_block_sums.get()) HIP_TRY(c, c->d_block_sums.alloc(2 * 4096 + 8));   // bucket totals + bucket starts
    if (c->have_dist) {                                   // table size depends on E*R8 too
        const uint64_t n_blocks = ((uint64_t)c->cfg.num_envs * p.R8 + 4095) / 4096;
        HIP_TRY(c, c->d_bkt_table.alloc((uint64_t)bucket_count(p) * n_blocks + 1));
        // zero from the start, here and not in the first step: a first step that is only CAPTURED (hipGraph) would record the clearing
        // without running it, and an eager step after it would count into whatever the allocation held
        HIP_TRY(c, hipMemset(c->d_bkt_table.get(), 0, c->d_bkt_table.bytes()));
        c->bkt_table_dirty = false;
        c->bins_ok = true;
    }
    return ROVER_OK;
}

// the candidate queue and its per-wave counters, as large as the plan says (nothing to do for a plan without a queue)
static int alloc_cull_queue(rover_ctx* c) {
    const StepPlan& p = c->plan;
    CullQueue& q = c->queue;
    if (!c->ws_ok || !p.queue_entries) return ROVER_OK;
    // (the counters are sized by the ray count, the queue — once capped by the budget — is not: a second rover_set_distribution with more
    //  rays must grow the counters even when the queue keeps its size)
    const bool fits = q.entries.get() && q.stats.get() && p.queue_entries == q.sized_for.queue_entries && p.stat_slots == q.sized_for.stat_slots;
    q.sized_for = p;
    if (fits) return ROVER_OK;
    q.entries.reset(); q.stats.reset();
    // no fallback to another kernel: a queue that cannot be allocated is an error the caller sees
    if (hipError_t e = q.entries.alloc(p.queue_entries))
        return fail(c, ROVER_E_NOMEM, "culled ray cast: candidate queue of %llu bytes: %s", (unsigned long long)(p.queue_entries * sizeof(uint2)), hipGetErrorString(e));
    HIP_TRY(c, q.stats.alloc(p.stat_slots));
    q.counters_written_under = StepPlan{};
    HIP_TRY(c, hipMemset(q.stats.get(), 0, q.stats.bytes()));
    return ROVER_OK;
}

static int alloc_workspace(rover_ctx* c);

// Every change of a plan input ends here: the plan, then the buffers it sizes — `what` names those beyond the queue that the change can
// resize — here, never in a step (hipMalloc is not allowed while a stream is capturing).  r: the caller's own result; after an error the
// plan is still brought up to date (rover_get_info reports it), and the buffers are left as they are.
enum Realloc { REALLOC_QUEUE, REALLOC_BINS, REALLOC_WORKSPACE };
static int replan(rover_ctx* c, Realloc what = REALLOC_QUEUE, int r = ROVER_OK) {
    c->plan = plan_step(plan_inputs(c));
    if (!r && what == REALLOC_WORKSPACE) r = alloc_workspace(c);
    if (!r && what == REALLOC_BINS) r = alloc_bins(c);
    return r ? r : alloc_cull_queue(c);
}

static int alloc_workspace(rover_ctx* c) {
    c->ws_ok = false;
    c->d_rays.reset(); c->d_dist_out.reset(); c->d_euler.reset(); c->d_heading.reset(); c->d_sorted.reset();
    c->d_bins.reset(); c->d_pairs.reset();
    const uint64_t E = (uint64_t)c->cfg.num_envs;
    const uint64_t n = E * c->plan.R8;
    if (n > 0xffffffffull) return fail(c, ROVER_E_INVALID, "num_envs * rays_per_env = %llu exceeds 2^32", (unsigned long long)n);
    HIP_TRY(c, c->d_rays.alloc(n));
    HIP_TRY(c, c->d_dist_out.alloc(n));
    HIP_TRY(c, c->d_euler.alloc(E * 3));
    HIP_TRY(c, c->d_heading.alloc(E));
    HIP_TRY(c, c->d_sorted.alloc(n));
    HIP_TRY(c, c->d_bins.alloc(n));
    HIP_TRY(c, c->d_pairs.alloc(n));
    HIP_TRY(c, hipMemset(c->d_euler.get(), 0, c->d_euler.bytes()));
    HIP_TRY(c, hipMemset(c->d_heading.get(), 0, c->d_heading.bytes()));
    c->workspace_bytes = n * (sizeof(RayRec) + sizeof(float) + 2 * sizeof(uint32_t) + sizeof(uint2)) + E * (4 * sizeof(float) + sizeof(int64_t));
    c->rays_valid = false;
    c->obs_valid = false;
    c->ws_ok = true;
    return alloc_bins(c);
}


// ---- internal triangle numbering of the culled ray cast's tables (rover_set_knn_map) -----------------------------------------
// The caller's triangle order means nothing (a decimated .ply lists triangles in no spatial order), but the kernel gains from
// two properties of the ids it works with: (i) consecutive ids are neighbours in space (one gather instruction of a wave then
// touches few cache lines, and bins that follow each other re-use each other's records in L2), (ii) a lane's packed pair holds two
// triangles that are candidates for the same rays (a queue entry then carries two candidates: fewer entries, fewer exact-phase
// lanes).  So: triangles are matched into spatial partners — mutual nearest centroids first (on a grid mesh exactly the two
// halves of every mesh cell), then greedily the nearest unmatched neighbour — and a pair gets the ids 2p, 2p + 1, pairs in
// Morton order of their first member; an unmatched triangle gets 2p and leaves 2p + 1 a hole.  order[new] = old (0xffffffff =
// hole), newid[old] = new.  A min over the same set of triangles does not depend on the numbering: results are unchanged.
static void cull_numbering(const std::vector<float2>& cen, std::vector<uint32_t>& order, std::vector<uint32_t>& newid) {
    const uint32_t T = (uint32_t)cen.size(), NONE = 0xffffffffu;
    auto finite = [](const float2& p) { return std::fabs(p.x) < 1e30f && std::fabs(p.y) < 1e30f; };
    float bx0 = 0.f, bx1 = 0.f, by0 = 0.f, by1 = 0.f;
    bool any = false;
    uint32_t n_fin = 0;
    for (const float2& p : cen) {
        if (!finite(p)) continue;
        ++n_fin;
        if (!any) { bx0 = bx1 = p.x; by0 = by1 = p.y; any = true; }
        bx0 = p.x < bx0 ? p.x : bx0; bx1 = p.x > bx1 ? p.x : bx1; by0 = p.y < by0 ? p.y : by0; by1 = p.y > by1 ? p.y : by1;
    }
    // Morton rank (16 bits per axis of the bounding box; broken triangles last)
    const double sx = bx1 > bx0 ? 65535.0 / ((double)bx1 - bx0) : 0.0, sy = by1 > by0 ? 65535.0 / ((double)by1 - by0) : 0.0;
    auto spread = [](uint32_t v) {                     // 16 bits -> every second bit of 32
        v = (v | (v << 8)) & 0x00ff00ffu; v = (v | (v << 4)) & 0x0f0f0f0fu;
        v = (v | (v << 2)) & 0x33333333u; v = (v | (v << 1)) & 0x55555555u;
        return v;
    };
    std::vector<uint64_t> key((size_t)T);
    for (uint32_t t = 0; t < T; ++t) {
        uint32_t m = 0xffffffffu;
        if (finite(cen[t])) m = (spread((uint32_t)(((double)cen[t].x - bx0) * sx)) << 1) | spread((uint32_t)(((double)cen[t].y - by0) * sy));
        key[t] = ((uint64_t)m << 32) | t;
    }
    std::sort(key.begin(), key.end());
    // uniform hash grid over the centroids, ~4 per bucket at mean density
    const double area = ((double)bx1 - bx0 + 1e-6) * ((double)by1 - by0 + 1e-6);
    double h = std::sqrt(area * 4.0 / (double)(n_fin ? n_fin : 1));
    uint32_t gx = (uint32_t)(((double)bx1 - bx0) / h) + 1, gy = (uint32_t)(((double)by1 - by0) / h) + 1;
    while ((uint64_t)gx * gy > (1u << 24)) { h *= 2.0; gx = (uint32_t)(((double)bx1 - bx0) / h) + 1; gy = (uint32_t)(((double)by1 - by0) / h) + 1; }
    auto bucket = [&](const float2& p, uint32_t& ix, uint32_t& iy) {
        ix = (uint32_t)(((double)p.x - bx0) / h); iy = (uint32_t)(((double)p.y - by0) / h);
        ix = ix >= gx ? gx - 1 : ix; iy = iy >= gy ? gy - 1 : iy;
    };
    std::vector<uint32_t> start((size_t)gx * gy + 1, 0), items((size_t)n_fin);
    for (uint32_t t = 0; t < T; ++t) if (finite(cen[t])) { uint32_t ix, iy; bucket(cen[t], ix, iy); ++start[(size_t)ix * gy + iy + 1]; }
    for (size_t b = 0; b < (size_t)gx * gy; ++b) start[b + 1] += start[b];
    {
        std::vector<uint32_t> cur(start.begin(), start.end() - 1);
        for (uint32_t t = 0; t < T; ++t) if (finite(cen[t])) { uint32_t ix, iy; bucket(cen[t], ix, iy); items[cur[(size_t)ix * gy + iy]++] = t; }
    }
    std::vector<uint32_t> partner((size_t)T, NONE);
    // nearest other centroid in the 3 x 3 buckets around t among those for which ok(u); ties by id
    auto nearest = [&](uint32_t t, auto&& ok) {
        uint32_t ix, iy, best = NONE;
        bucket(cen[t], ix, iy);
        double bd = 1e300;
        for (uint32_t a = ix ? ix - 1 : 0; a <= (ix + 1 < gx ? ix + 1 : gx - 1); ++a)
            for (uint32_t b = iy ? iy - 1 : 0; b <= (iy + 1 < gy ? iy + 1 : gy - 1); ++b)
                for (uint32_t k = start[(size_t)a * gy + b]; k < start[(size_t)a * gy + b + 1]; ++k) {
                    const uint32_t u = items[k];
                    if (u == t || !ok(u)) continue;
                    const double dx = (double)cen[u].x - cen[t].x, dy = (double)cen[u].y - cen[t].y, d = dx * dx + dy * dy;
                    if (d < bd || (d == bd && u < best)) { bd = d; best = u; }
                }
        return best;
    };
    {   // pass 1: mutual nearest neighbours
        std::vector<uint32_t> nn((size_t)T, NONE);
        for (uint32_t t = 0; t < T; ++t) if (finite(cen[t])) nn[t] = nearest(t, [](uint32_t) { return true; });
        for (uint32_t t = 0; t < T; ++t) if (nn[t] != NONE && nn[t] > t && nn[nn[t]] == t) { partner[t] = nn[t]; partner[nn[t]] = t; }
    }
    // pass 2, in Morton order: the nearest still unmatched neighbour
    for (uint32_t r = 0; r < T; ++r) {
        const uint32_t t = (uint32_t)key[r];
        if (partner[t] != NONE || !finite(cen[t])) continue;
        const uint32_t u = nearest(t, [&](uint32_t v) { return partner[v] == NONE; });
        if (u != NONE) { partner[t] = u; partner[u] = t; }
    }
    order.clear();
    order.reserve((size_t)T + T / 8);
    std::vector<uint8_t> done((size_t)T, 0);
    for (uint32_t r = 0; r < T; ++r) {
        const uint32_t t = (uint32_t)key[r];
        if (done[t]) continue;
        const uint32_t u = partner[t];
        done[t] = 1;
        newid[t] = (uint32_t)order.size(); order.push_back(t);
        if (u != NONE) { done[u] = 1; newid[u] = (uint32_t)order.size(); order.push_back(u); }
        else order.push_back(NONE);
    }
}

// rover_set_knn_map's work, into `m` alone: the re-packed map, then — where the culled ray cast can serve the map (64 lanes x 4 triangles;
// triangle ids and the map bit share 32 bits of a queue entry) — its tables, then the staged kernel's.  The build's own buffers go on return.
static int build_map_tables(rover_ctx* c, MapTables& m, int which, const int32_t* map_idx, int32_t X, int32_t Y, int32_t K, const int32_t* tris,
                            int32_t T, const uint16_t* verts, int32_t V, float cell, float shift_x, float shift_y) {
    const uint64_t n_cells = (uint64_t)X * Y;
    const uint32_t K8 = (uint32_t)((K + 7) / 8 * 8);
    DevBuf<int32_t> d_idx, d_tris;
    DevBuf<uint16_t> d_verts;
    hipError_t e;
    if ((e = d_idx.alloc(n_cells * K)) != hipSuccess || (e = d_tris.alloc((uint64_t)T * 3)) != hipSuccess ||
        (e = d_verts.alloc((uint64_t)V * 3)) != hipSuccess || (e = m.table.alloc(n_cells * 9ull * K8)) != hipSuccess)
        return fail(c, ROVER_E_NOMEM, "set_knn_map: hipMalloc (%llu B table): %s", (unsigned long long)(n_cells * 9ull * K8 * sizeof(uint16_t)),
                    hipGetErrorString(e));
    if ((e = hipMemcpy(d_idx.get(), map_idx, d_idx.bytes(), hipMemcpyDefault)) != hipSuccess ||
        (e = hipMemcpy(d_tris.get(), tris, d_tris.bytes(), hipMemcpyDefault)) != hipSuccess ||
        (e = hipMemcpy(d_verts.get(), verts, d_verts.bytes(), hipMemcpyDefault)) != hipSuccess ||
        (e = launch_repack(d_idx.get(), d_tris.get(), d_verts.get(), n_cells, (uint32_t)K, K8, (uint32_t)T, (uint32_t)V, m.table.get(), nullptr)) != hipSuccess ||
        (e = hipDeviceSynchronize()) != hipSuccess)
        return fail(c, ROVER_E_HIP, "set_knn_map: %s", hipGetErrorString(e));
    m.knn = KnnDev{m.table.get(), X, Y, K, (int32_t)K8, cell, shift_x, shift_y, 1.0f / cell};
    m.lane_pp = lane_pairs_per_row(K8);
    m.tris = T; m.cells = (int64_t)n_cells;
    if (K8 > 256 || (uint32_t)T >= 0x1ffffffu) return ROVER_OK;
    // internal triangle numbering (spatial partners get ids 2p, 2p + 1, pairs ordered along a Morton curve): cull_numbering()
    std::vector<uint32_t> order, newid((size_t)T);
    {
        DevBuf<float2> d_cen;
        std::vector<float2> cen((size_t)T);
        if ((e = d_cen.alloc(T)) != hipSuccess ||
            (e = launch_tri_centroids(d_tris.get(), d_verts.get(), (uint32_t)T, (uint32_t)V, d_cen.get(), nullptr)) != hipSuccess ||
            (e = hipMemcpy(cen.data(), d_cen.get(), d_cen.bytes(), hipMemcpyDeviceToHost)) != hipSuccess)
            return fail(c, ROVER_E_HIP, "set_knn_map: triangle centroids: %s", hipGetErrorString(e));
        cull_numbering(cen, order, newid);
    }
    const uint32_t T_int = (uint32_t)order.size();
    if (T_int >= 0x3ffffffu) return fail(c, ROVER_E_INVALID, "set_knn_map: too many triangles for the culled ray cast's 26-bit ids");
    // the culled ray cast's tables and the build's buffers (qrow: per cell and proof, read only by the build kernels)
    DevBuf<uint32_t> d_qrow[2], d_order, d_newid, d_cnt;
    DevBuf<float> d_nz;
    if ((e = m.cull_idx.alloc(n_cells * K8)) != hipSuccess || (e = m.rtab.alloc((uint64_t)T_int * 10u)) != hipSuccess ||
        (e = m.proof[0].ctab.alloc(T_int)) != hipSuccess || (e = m.proof[1].ctab.alloc(T_int)) != hipSuccess ||
        (e = m.proof[0].far.alloc(3 * n_cells)) != hipSuccess || (e = m.proof[1].far.alloc(3 * n_cells)) != hipSuccess ||
        (e = d_qrow[0].alloc(n_cells)) != hipSuccess || (e = d_qrow[1].alloc(n_cells)) != hipSuccess || (e = d_nz.alloc(T_int)) != hipSuccess ||
        (e = d_cnt.alloc(8)) != hipSuccess || (e = d_order.alloc(T_int)) != hipSuccess || (e = d_newid.alloc(T)) != hipSuccess)
        return fail(c, ROVER_E_HIP, "set_knn_map: cull tables: %s", hipGetErrorString(e));
    // The staged kernel's tables are optional, each proof's on its own: which proofs get them is the "staged_tables" option, and an allocation
    // that fails drops that proof's (the culled kernel then runs for it, plan_step) — unless variant 4 was asked for by name.
    for (int k = 0; k < 2; ++k) {
        if (!((c->knobs.staged_tables >> k) & 1)) continue;
        ProofTables& p = m.proof[k];
        if ((e = p.lvl.alloc(n_cells * lane_lvl_stride())) != hipSuccess || (e = p.lrec.alloc(n_cells * 2ull * m.lane_pp)) != hipSuccess ||
            (e = p.lid.alloc(n_cells * m.lane_pp)) != hipSuccess) {
            p.lvl.reset(); p.lrec.reset(); p.lid.reset();
            if (c->knobs.variant == 4)
                return fail(c, ROVER_E_NOMEM, "set_knn_map: the staged ray cast's tables (%llu B per proof) do not fit and raycast_variant 4 was requested: %s",
                            (unsigned long long)(n_cells * ((uint64_t)lane_lvl_stride() * sizeof(float4) + (uint64_t)m.lane_pp * (2 * sizeof(uint4) + sizeof(uint2)))),
                            hipGetErrorString(e));
        }
    }
    CullBuildArgs a{};
    a.map_idx = d_idx.get(); a.tris = d_tris.get(); a.verts = d_verts.get();
    a.n_cells = n_cells; a.K = (uint32_t)K; a.K8 = K8; a.T = (uint32_t)T; a.T_int = T_int; a.V = (uint32_t)V;
    a.order = d_order.get(); a.newid = d_newid.get(); a.idx4 = m.cull_idx.get(); a.rtab = m.rtab.get();
    a.ctab = m.proof[0].ctab.get(); a.ctab_h = m.proof[1].ctab.get(); a.qrow = d_qrow[0].get(); a.qrow_h = d_qrow[1].get();
    a.far = m.proof[0].far.get(); a.far_h = m.proof[1].far.get(); a.nz_scratch = d_nz.get(); a.counts = d_cnt.get();
    a.ph = cull_proof_h(c->knobs.cull_eta_h, c->knobs.cull_split_h); a.Y = (uint32_t)Y; a.cell_size = cell; a.shift_x = shift_x; a.shift_y = shift_y;
    a.lane = m.proof[0].view(); a.lane_h = m.proof[1].view();
    uint32_t h_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((e = hipMemcpy(d_order.get(), order.data(), d_order.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_newid.get(), newid.data(), d_newid.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemset(d_cnt.get(), 0, d_cnt.bytes())) != hipSuccess || (e = launch_cull_build(a, nullptr)) != hipSuccess ||
        (e = hipDeviceSynchronize()) != hipSuccess || (e = hipMemcpy(h_cnt, d_cnt.get(), sizeof h_cnt, hipMemcpyDeviceToHost)) != hipSuccess)
        return fail(c, ROVER_E_HIP, "set_knn_map: cull tables (%llu B): %s", (unsigned long long)m.bytes(), hipGetErrorString(e));
    m.proof[0].always = h_cnt[0]; m.proof[0].nocone = h_cnt[1];
    m.proof[1].always = h_cnt[2]; m.proof[1].nocone = h_cnt[3];
    m.farok = h_cnt[4];
    const bool box = a.lane.lrec && (c->knobs.lane_box > 0 || (c->knobs.lane_box < 0 && lane_box_share_met(h_cnt[5], h_cnt[6])));
    // One row per two cells (option "lane_pair_rows": auto = the terrain map, whose cells nearly all hold rays, so that a row is read once for
    // the rays of both): taken where every row's union fits a row — else the map keeps the per-cell tables built above.  The tables are
    // allocated again for the form (rows of the largest union: about 0.6 of the per-cell size); as before, a proof whose tables do not fit goes without.
    if ((a.lane.lrec || a.lane_h.lrec) && n_cells < (1ull << 24) && (uint32_t)T < (1u << 30) &&
        (c->knobs.lane_pair_rows > 0 || (c->knobs.lane_pair_rows < 0 && which == ROVER_MAP_TERRAIN))) {
        const uint64_t n_rows = lane_pair_rows_count(n_cells, (uint32_t)Y);
        DevBuf<uint2> d_upair;
        if (d_upair.alloc(n_rows * 128ull) == hipSuccess) {
            if ((e = launch_lane_union(a, d_upair.get(), nullptr)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
                (e = hipMemcpy(h_cnt + 7, d_cnt.get() + 7, sizeof(uint32_t), hipMemcpyDeviceToHost)) != hipSuccess)
                return fail(c, ROVER_E_HIP, "set_knn_map: staged tables, the rows' unions: %s", hipGetErrorString(e));
            const uint32_t pp = lane_pair_rows_pp(h_cnt[7]);
            if (pp) {
                for (int k = 0; k < 2; ++k) {
                    ProofTables& p = m.proof[k];
                    if (!p.lrec.get()) continue;
                    p.lvl.reset(); p.lrec.reset(); p.lid.reset();
                    if (p.lvl.alloc(n_rows * lane_lvl_stride()) != hipSuccess || p.lrec.alloc(n_rows * 2ull * pp) != hipSuccess ||
                        p.lid.alloc(n_rows * pp) != hipSuccess) { p.lvl.reset(); p.lrec.reset(); p.lid.reset(); }
                }
                a.lane = m.proof[0].view(); a.lane_h = m.proof[1].view();
                if ((e = launch_lane_pair_rows(a, d_upair.get(), pp, box ? 1 : 0, nullptr)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
                    return fail(c, ROVER_E_HIP, "set_knn_map: staged tables in shared-row form: %s", hipGetErrorString(e));
                m.lane_pp = pp; m.lane_pair_rows = true; m.lane_box = box && a.lane.lrec;
                return ROVER_OK;
            }
        }
    }
    // the form of test (A)'s records in the f32 proof's staged tables (option "lane_box"): boxes where most pairs fill theirs
    if (box) {
        if ((e = launch_lane_box(a, nullptr)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
            return fail(c, ROVER_E_HIP, "set_knn_map: staged tables in box form: %s", hipGetErrorString(e));
        m.lane_box = true;
    }
    return ROVER_OK;
}

// ---- knobs: one table for the ROVER_* environment (rover_create) and rover_set_option -------------------------------------------------
// What a change invalidates, and how the two sides differ where they do, are data of the row.
enum : unsigned { KNOB_REPLAN = 1, KNOB_BINS = 2, KNOB_RAYS_OBS = 4 };      // the plan; the sort's tables too; the ray workspace and the obs state
enum : unsigned {
    KNOB_OPT_ALSO_ZERO = 1,     // the option accepts 0 (the library's choice) beside its range; the environment only the range
    KNOB_ENV_AS_BOOL = 2,       // the environment's value is read as v != 0
    KNOB_REAL = 4,              // a real number (atof), else an integer (atol)
    KNOB_MUST_RUN = 8,          // the option names a kernel: a variant that cannot run is refused (staged_tables_missing)
};
struct KnobRow {
    const char* option;         // rover_set_option name, or NULL
    const char* env;            // read at rover_create, or NULL
    double opt_lo, opt_hi;      // accepted by the option; anything else is ROVER_E_INVALID
    double env_lo, env_hi;      // accepted from the environment; anything else is ignored
    unsigned flags;
    void (*set)(rover_ctx*, double);
    unsigned invalidates;
    const char* values;         // the option's accepted values in words (its error message)
};
#define KNOB_SET(field, expr) [](rover_ctx* c, double v) { c->field = (expr); }
static const double kIntMin = -2147483648.0, kIntMax = 2147483647.0, kLongMax = 9223372036854775807.0;
static const KnobRow kKnobs[] = {
    {"raycast_variant", "ROVER_RAYCAST_VARIANT", 0, 4, 1, 4, KNOB_MUST_RUN, KNOB_SET(knobs.variant, (int)v), KNOB_REPLAN,
     "0 (auto), 1 (env order), 2 (binned), 3 (culled) or 4 (staged)"},
    {"raycast_run", "ROVER_RAYCAST_RUN", 0, 4096, 1, 4096, 0, KNOB_SET(knobs.run, (uint32_t)v), KNOB_REPLAN, "0 (auto) or in [1, 4096]"},
    {"lane_env_order", "ROVER_LANE_ENV_ORDER", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_env_order, (int)v), KNOB_REPLAN,
     "-1 (auto), 0 or 1"},
    {"lane_rocks", "ROVER_LANE_ROCKS", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_rocks, (int)v), KNOB_REPLAN, "-1 (auto), 0 or 1"},
    {"lane_box", "ROVER_LANE_BOX", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_box, (int)v), 0,      // takes effect at the next rover_set_knn_map
     "-1 (auto), 0 or 1"},
    {"lane_pair_rows", "ROVER_LANE_PAIR_ROWS", -1, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(knobs.lane_pair_rows, (int)v), 0,      // (the same)
     "-1 (auto), 0 or 1"},
    {"lane_rebase", "ROVER_LANE_REBASE", 0, 1, kIntMin, kIntMax, KNOB_ENV_AS_BOOL, KNOB_SET(lane_rebase, (int32_t)v), 0,      // read at every launch: no plan, no table depends on it
     "0 or 1"},
    {nullptr, "ROVER_CULL_LAZY", 1, 0, kIntMin, kIntMax, 0, KNOB_SET(knobs.cull_lazy, (int)v), KNOB_REPLAN, nullptr},
    {"bin_low_bits", "ROVER_BIN_LOW_BITS", 8, 12, 8, 12, KNOB_OPT_ALSO_ZERO, KNOB_SET(knobs.low_bits_opt, (uint32_t)v), KNOB_REPLAN | KNOB_BINS,
     "0 (chosen by the library) or in [8, 12]"},
    {"cull_queue_mb", "ROVER_CULL_QUEUE_MB", 1, 1 << 20, 1, kLongMax, 0, KNOB_SET(knobs.cull_budget, (uint64_t)v << 20), KNOB_REPLAN, "in [1, 1048576]"},
    {nullptr, "ROVER_CULLH_ETA", 1, 0, 0.02, 0.5, KNOB_REAL, KNOB_SET(knobs.cull_eta_h, v), 0, nullptr},
    {nullptr, "ROVER_CULLH_SPLIT", 1, 0, 0.5, 64.0, KNOB_REAL, KNOB_SET(knobs.cull_split_h, v), 0, nullptr},
    {"staged_tables", nullptr, 0, 3, 1, 0, 0, KNOB_SET(knobs.staged_tables, (int)v), 0,      // takes effect at the next rover_set_knn_map
     "0 (none), 1 (f32 proof), 2 (as-shipped fp16 proof) or 3 (both)"},
    {"raycast_early_out", nullptr, 0, 1, 1, 0, 0, KNOB_SET(knobs.early_out, (uint32_t)v), 0, "0 or 1"},
    // (what an observation means changes with these two: rover_calculate_metrics wants a fresh rover_get_observations)
    {"ray_precision", nullptr, 0, 2, 1, 0, 0, KNOB_SET(precision, (int)v), KNOB_REPLAN | KNOB_RAYS_OBS, "0 (fp32), 1 (fp16 sources) or 2 (as shipped)"},
    {"cell_index_mode", nullptr, 0, 1, 1, 0, 0, KNOB_SET(cell_rcp, (int32_t)v), KNOB_RAYS_OBS, "0 (cpu_div) or 1 (cuda_rcp)"},
    {"occlusion_route", nullptr, 0, 1, 1, 0, 0, KNOB_SET(occlusion_route, (int32_t)v), 0,      // read at every call: no table depends on it
     "0 (plain march) or 1 (ordered columns and the tile-max table)"},
};
#undef KNOB_SET

static const KnobRow* knob_by_option(const char* name) {
    for (const KnobRow& k : kKnobs)
        if (k.option && !strcmp(k.option, name)) return &k;
    return nullptr;
}
static bool knob_option_accepts(const KnobRow& k, double v) {
    return (v >= k.opt_lo && v <= k.opt_hi) || ((k.flags & KNOB_OPT_ALSO_ZERO) && v == 0);
}

static void plan_to_c(const StepPlan& p, rover_raycast_plan* out) {
    out->variant = p.variant; out->proof = p.proof; out->sorted = p.sorted ? 1 : 0; out->env_order = p.env_order ? 1 : 0;
    out->rocks_staged = p.rocks_staged ? 1 : 0; out->run = (int32_t)p.run; out->env_run = (int32_t)p.env_run;
    out->lazy_far = p.lazy_far ? 1 : 0; out->skip_clear = p.skip_clear ? 1 : 0;
    out->cull_launches = (int32_t)p.cull_launches; out->low_bits = (int32_t)p.low_bits;
    out->sort_entry_dwords = (int32_t)p.sort_entry_dwords; out->hist_fused = p.hist_fused ? 1 : 0;
}

extern "C" {

#ifndef ROVER_SRC_HASH
#define ROVER_SRC_HASH "unknown"
#endif
const char* rover_version(void) { return "rover_step 0.3 (gfx950) src-" ROVER_SRC_HASH; }

const char* rover_last_error(const rover_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int rover_create(const rover_cfg* cfg, rover_ctx** out) {
    if (!cfg || !out) return fail(nullptr, ROVER_E_INVALID, "rover_create: null argument");
    if (cfg->num_envs <= 0) return fail(nullptr, ROVER_E_INVALID, "rover_create: num_envs must be > 0 (got %d)", cfg->num_envs);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, ROVER_E_HIP, "rover_create: no HIP device available (%s)", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, ROVER_E_INVALID, "rover_create: device %d out of range (have %d)", cfg->device, ndev);
    rover_ctx* c = new (std::nothrow) rover_ctx();
    if (!c) return fail(nullptr, ROVER_E_NOMEM, "rover_create: out of host memory");
    c->cfg = *cfg;
    if (c->cfg.num_envs_global <= 0) c->cfg.num_envs_global = c->cfg.num_envs;
    if (c->cfg.max_episode_length <= 0) c->cfg.max_episode_length = 3000;
    for (const KnobRow& k : kKnobs) {
        const char* text = k.env ? getenv(k.env) : nullptr;
        if (!text) continue;
        double v = (k.flags & KNOB_REAL) ? atof(text) : (double)atol(text);
        if (v < k.env_lo || v > k.env_hi) continue;
        if (k.flags & KNOB_ENV_AS_BOOL) v = v != 0 ? 1 : 0;
        k.set(c, v);
    }
    (void)replan(c);                 // (no maps, no distribution yet: nothing to size)
    DeviceGuard guard(cfg->device);
    e = guard.err;
    if (e == hipSuccess) e = c->d_block_cnt.alloc((size_t)cfg->num_envs / 256 + 2);
    if (e == hipSuccess) e = c->d_goal_work.alloc(2 * (size_t)cfg->num_envs);
    if (e == hipSuccess) e = c->d_ids_work.alloc((size_t)cfg->num_envs);
    if (e == hipSuccess) e = c->d_gae_partials.alloc(3 * (size_t)GAE_MAX_BLOCKS);
    if (e == hipSuccess) e = c->d_ppo_partials.alloc((3 + (size_t)GAUSS_MAX_A) * PPO_MAX_BLOCKS);
    if (e != hipSuccess) { delete c; return fail(nullptr, ROVER_E_HIP, "rover_create: %s", hipGetErrorString(e)); }
    *out = c;
    return ROVER_OK;
}

void rover_destroy(rover_ctx* c) {
    if (!c) return;
    DeviceGuard guard(c->cfg.device);         // the owners free their device memory on the ctx's device
    for (auto& e : c->ev0) (void)hipEventDestroy(e);
    for (auto& e : c->ev1) (void)hipEventDestroy(e);
    delete c;
}

int rover_set_knn_map(rover_ctx* c, int which, const int32_t* map_idx, int32_t X, int32_t Y, int32_t K, const int32_t* tris,
                      int32_t T, const uint16_t* verts, int32_t V, float cell, float shift_x, float shift_y) {
    if (!c) return ROVER_E_INVALID;
    if (which != ROVER_MAP_TERRAIN && which != ROVER_MAP_ROCKS) return fail(c, ROVER_E_INVALID, "set_knn_map: which=%d", which);
    if (!map_idx || !tris || !verts) return fail(c, ROVER_E_INVALID, "set_knn_map: null table pointer");
    if (X <= 0 || Y <= 0 || K <= 0 || T <= 0 || V <= 0 || !(cell > 0.0f))
        return fail(c, ROVER_E_INVALID, "set_knn_map: bad shape X=%d Y=%d K=%d T=%d V=%d cell=%g", X, Y, K, T, V, (double)cell);
    if ((uint64_t)X * (uint64_t)Y > 0xffffffffull) return fail(c, ROVER_E_INVALID, "set_knn_map: X*Y exceeds 2^32 cells");
    USE_DEVICE(c);
    MapTables m;
    if (int r = build_map_tables(c, m, which, map_idx, X, Y, K, tris, T, verts, V, cell, shift_x, shift_y)) return r;      // (the previous map stays)
    c->maps[which] = std::move(m);
    c->rays_valid = false;
    return replan(c, REALLOC_BINS);
}

int rover_set_distribution(rover_ctx* c, const double* pts, int32_t P, const int64_t* sparse_idx, int32_t Ns,
                           const int64_t* dense_idx, int32_t Nd) {
    if (!c) return ROVER_E_INVALID;
    if (!pts || P <= 0 || Ns < 0 || Nd < 0 || (Ns > 0 && !sparse_idx) || (Nd > 0 && !dense_idx))
        return fail(c, ROVER_E_INVALID, "set_distribution: bad arguments (P=%d Ns=%d Nd=%d)", P, Ns, Nd);
    USE_DEVICE(c);
    std::vector<double> hp((size_t)P * 3);
    std::vector<int64_t> hs((size_t)Ns), hd((size_t)Nd);
    HIP_TRY(c, hipMemcpy(hp.data(), pts, hp.size() * sizeof(double), hipMemcpyDefault));
    if (Ns) HIP_TRY(c, hipMemcpy(hs.data(), sparse_idx, hs.size() * sizeof(int64_t), hipMemcpyDefault));
    if (Nd) HIP_TRY(c, hipMemcpy(hd.data(), dense_idx, hd.size() * sizeof(int64_t), hipMemcpyDefault));
    std::vector<int32_t> idx;
    idx.reserve((size_t)Ns + Nd);
    for (int64_t v : hs) idx.push_back((int32_t)v);
    for (int64_t v : hd) idx.push_back((int32_t)v);
    for (int32_t v : idx)
        if (v < 0 || v >= P) return fail(c, ROVER_E_INVALID, "set_distribution: index %d outside [0,%d)", v, P);
    c->have_dist = false;
    ++c->dist_gen;
    c->d_dist.reset(); c->d_obs_idx.reset();
    const int r = [&]() -> int {
        HIP_TRY(c, c->d_dist.alloc(hp.size()));
        HIP_TRY(c, hipMemcpy(c->d_dist.get(), hp.data(), c->d_dist.bytes(), hipMemcpyHostToDevice));
        HIP_TRY(c, c->d_obs_idx.alloc(idx.size() + 1));
        HIP_TRY(c, hipMemset(c->d_obs_idx.get(), 0, c->d_obs_idx.bytes()));      // assemble_obs_kernel reads entry 0 from every lane
        if (!idx.empty()) HIP_TRY(c, hipMemcpy(c->d_obs_idx.get(), idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        c->P = P; c->Ns = Ns; c->Nd = Nd;
        c->have_dist = true;
        return ROVER_OK;
    }();
    return replan(c, REALLOC_WORKSPACE, r);         // (a failure half way leaves no distribution: the plan says so too)
}

int rover_set_heightfield(rover_ctx* c, const float* hm, int32_t N0, int32_t N1, float hscale, float vscale, float sx, float sy) {
    if (!c) return ROVER_E_INVALID;
    if (!hm || N0 <= 0 || N1 <= 0 || !(hscale > 0.0f)) return fail(c, ROVER_E_INVALID, "set_heightfield: bad arguments");
    USE_DEVICE(c);
    DevBuf<float> d;
    HIP_TRY(c, d.alloc((uint64_t)N0 * N1));
    HIP_TRY(c, hipMemcpy(d.get(), hm, d.bytes(), hipMemcpyDefault));       // (the previous heightfield stays in place)
    c->d_hm = std::move(d);
    ++c->hf_gen;
    c->hf = HeightDev{c->d_hm.get(), N0, N1, hscale, vscale, sx, sy, 1.0f / hscale, c->cell_rcp};
    c->have_hf = true;
    return ROVER_OK;
}

int rover_set_stones(rover_ctx* c, const float* info7, int32_t S) {
    if (!c) return ROVER_E_INVALID;
    if (S < 0 || (S > 0 && !info7)) return fail(c, ROVER_E_INVALID, "set_stones: bad arguments");
    USE_DEVICE(c);
    std::vector<float> h((size_t)S * 7);
    if (S) HIP_TRY(c, hipMemcpy(h.data(), info7, h.size() * sizeof(float), hipMemcpyDefault));
    // stone-occupancy grid: 2 m cells over the stones' bounding box padded by r_max + 1.4 m (the largest threshold the
    // task uses, rover.py:660) + margin; a cell lists the stones whose inflated disc reaches it.
    const float cell = 2.0f, reach = 1.4f + 0.05f;
    float x0 = 0.f, y0 = 0.f, x1 = 1.f, y1 = 1.f, rmax = 0.f;
    bool any = false, poisoned = false;
    for (int s = 0; s < S; ++s) {
        float x = h[7 * s], y = h[7 * s + 1], r = h[7 * s + 6];
        // torch.min propagates NaN (rover.py:538): one NaN stone makes nearest_rock NaN for every query, and
        // NaN <= thr is False -> nothing ever collides.  Reproduced by leaving every cell list empty.
        if (!(x == x) || !(y == y) || !(r == r)) { poisoned = true; continue; }
        if (!any) { x0 = x1 = x; y0 = y1 = y; any = true; }
        x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        rmax = r > rmax ? r : rmax;
    }
    const float pad = rmax + reach;
    x0 -= pad; y0 -= pad; x1 += pad; y1 += pad;
    int nx = (int)((x1 - x0) / cell) + 1, ny = (int)((y1 - y0) / cell) + 1;
    if (nx < 1) nx = 1; if (ny < 1) ny = 1;
    if ((int64_t)nx * ny > (int64_t)1 << 24) return fail(c, ROVER_E_INVALID, "set_stones: stone extent too large for the 2 m grid");
    std::vector<std::vector<uint32_t>> lists((size_t)nx * ny);
    for (int s = 0; s < S && any && !poisoned; ++s) {
        float x = h[7 * s], y = h[7 * s + 1], r = h[7 * s + 6];
        if (!(x == x) || !(y == y) || !(r == r)) continue;
        float rr = r + reach;
        int cx0 = (int)((x - rr - x0) / cell), cx1 = (int)((x + rr - x0) / cell);
        int cy0 = (int)((y - rr - y0) / cell), cy1 = (int)((y + rr - y0) / cell);
        cx0 = cx0 < 0 ? 0 : cx0; cy0 = cy0 < 0 ? 0 : cy0; cx1 = cx1 >= nx ? nx - 1 : cx1; cy1 = cy1 >= ny ? ny - 1 : cy1;
        for (int cx = cx0; cx <= cx1; ++cx)
            for (int cy = cy0; cy <= cy1; ++cy) lists[(size_t)cx * ny + cy].push_back((uint32_t)s);   // stone order kept
    }
    std::vector<uint32_t> start((size_t)nx * ny + 1, 0), idx;
    for (size_t k = 0; k < lists.size(); ++k) { start[k + 1] = start[k] + (uint32_t)lists[k].size(); idx.insert(idx.end(), lists[k].begin(), lists[k].end()); }
    std::vector<float4> xyr(idx.size() + 1);
    for (size_t k = 0; k < idx.size(); ++k) {
        const uint32_t sidx = idx[k];
        float fid; memcpy(&fid, &sidx, sizeof fid);
        xyr[k] = float4{h[7 * (size_t)sidx], h[7 * (size_t)sidx + 1], h[7 * (size_t)sidx + 6], fid};
    }
    DevBuf<uint32_t> d_start;
    DevBuf<float4> d_xyr;
    DevBuf<float> d_info;
    hipError_t e;
    if ((e = d_start.alloc(start.size())) != hipSuccess || (e = d_xyr.alloc(xyr.size())) != hipSuccess ||
        (e = d_info.alloc((uint64_t)S * 7 + 1)) != hipSuccess ||
        (e = hipMemcpy(d_start.get(), start.data(), d_start.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(d_xyr.get(), xyr.data(), d_xyr.bytes(), hipMemcpyHostToDevice)) != hipSuccess ||
        (S && (e = hipMemcpy(d_info.get(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess))
        return fail(c, ROVER_E_HIP, "set_stones: %s", hipGetErrorString(e));        // the previous stone tables stay in place
    c->d_stones = std::move(d_info); c->d_grid_start = std::move(d_start); c->d_grid_xyr = std::move(d_xyr);
    c->sgrid = StoneGridDev{c->d_grid_start.get(), c->d_grid_xyr.get(), x0, y0, 1.0f / cell, nx, ny};
    c->S = S;
    c->have_stones = true;
    return ROVER_OK;
}

int rover_set_curriculum_level(rover_ctx* c, int32_t level) {
    if (!c) return ROVER_E_INVALID;
    c->cfg.curriculum_level = level;
    return ROVER_OK;
}

// ---- step ------------------------------------------------------------------------------------------
static int check_precision(rover_ctx* c) {
    if (c->precision == 2 && c->plan.variant < 2)
        return fail(c, ROVER_E_STATE, "ray_precision 2 (as shipped, fp16 maths) needs ray-cast variant 2 or 3 (K <= 256 on both maps)");
    // a variant asked for by name is the one that runs, or the call fails: the staged kernel needs the tables of the arithmetic in force
    if (c->knobs.variant == 4 && staged_tables_missing(plan_inputs(c)))
        return fail(c, ROVER_E_STATE, "raycast_variant 4 (staged) was requested but its tables for ray_precision %d are not there (option "
                                      "staged_tables, or they did not fit when the maps were set)", c->precision);
    return ROVER_OK;
}

static int check_ready(rover_ctx* c) {
    if (!have_maps(c)) return fail(c, ROVER_E_STATE, "terrain and rocks maps must be set (rover_set_knn_map)");
    if (!c->have_dist) return fail(c, ROVER_E_STATE, "ray distribution must be set (rover_set_distribution)");
    if (!c->ws_ok || !c->bins_ok) return fail(c, ROVER_E_STATE, "the step workspace is not allocated (an earlier rover_set_* call failed)");
    return check_precision(c);
}

static CullArgs cull_args(const rover_ctx* c, const StepPlan& p, uint32_t n_valid) {
    CullArgs a{};
    a.rays = c->d_rays.get(); a.sorted = c->d_sorted.get(); a.n_sorted = n_valid;
    a.n_terrain = (uint32_t)c->cfg.num_envs * (uint32_t)c->P;
    const MapTables &m0 = c->maps[0], &m1 = c->maps[1];
    const int k = p.proof;                // the as-shipped fp16 arithmetic: its own proof tables, the fp16 exact phase
    a.idx0 = m0.cull_idx.get(); a.idx1 = m1.cull_idx.get();
    a.ctab0 = m0.proof[k].ctab.get(); a.ctab1 = m1.proof[k].ctab.get();
    a.rtab0 = m0.rtab.get(); a.rtab1 = m1.rtab.get();
    a.half = k;
    const CullProofH ph = cull_proof_h(c->knobs.cull_eta_h, c->knobs.cull_split_h);
    a.c_a_h = ph.c_a; a.tau2_h = ph.tau2;
    a.far0 = m0.proof[k].far.get(); a.far1 = m1.proof[k].far.get();
    a.near0 = a.far0 + 2ull * (uint64_t)m0.cells; a.near1 = a.far1 + 2ull * (uint64_t)m1.cells;
    a.k2_far = cull_far_k2(a.half, ph);
    a.lazy_far = p.lazy_far ? 1 : 0;
    a.skip_clear = p.skip_clear ? 1 : 0;
    a.kp0 = (uint32_t)c->maps[0].knn.K8; a.kp1 = (uint32_t)c->maps[1].knn.K8;
    a.run = p.run;
    a.out = c->d_dist_out.get();
    a.queue = c->queue.entries.get();
    a.stats = c->queue.stats.get();
    a.queue_entries = p.queue_entries;          // (check_queue: the queue was sized for p)
    return a;
}

// the culled / staged ray cast's candidate queue and counters were sized for plan p (replan; never in a step: no hipMalloc inside a stream capture)
static int check_queue(rover_ctx* c, const StepPlan& p) {
    const CullQueue& q = c->queue;
    if (p.variant >= 3 && (!q.entries.get() || !q.stats.get() || q.sized_for != p))
        return fail(c, ROVER_E_STATE, "the culled ray cast's candidate queue is not allocated for the options in force");
    return ROVER_OK;
}

// the ray-cast launch(es) of plan p, on the ray records / sorted list in the workspace
static int run_raycast(rover_ctx* c, const StepPlan& p, uint32_t n_valid, hipStream_t s) {
    const uint32_t E = (uint32_t)c->cfg.num_envs;
    CullQueue& q = c->queue;
    if (p.variant >= 3 && q.stats.get() && p != q.counters_written_under) {
        // the per-wave counters of rover_get_cull_info: a launch writes the slots of its own waves; when the way the rays are cast changed
        // since the last launch (another kernel, order or run length: another number of waves) the slots are cleared first
        HIP_TRY(c, hipMemsetAsync(q.stats.get(), 0, q.stats.bytes(), s));
        q.counters_written_under = p;
    }
    if (p.variant == 4) {
        LaneArgs l{};
        l.rays = c->d_rays.get(); l.sorted = c->d_sorted.get(); l.n_sorted = n_valid; l.n_terrain = E * (uint32_t)c->P;
        for (int w = 0; w < 2; ++w) {
            const LaneTables t = c->maps[w].proof[p.proof].view();
            l.lvl[w] = t.lvl; l.lrec[w] = t.lrec; l.lid[w] = t.lid; l.rtab[w] = c->maps[w].rtab.get(); l.pp[w] = c->maps[w].lane_pp;
        }
        {
            const CullProofH ph = cull_proof_h(c->knobs.cull_eta_h, c->knobs.cull_split_h);
            l.half = p.proof; l.c_a_h = ph.c_a; l.k2_far = cull_far_k2(l.half, ph);
            l.forms = p.proof ? 0u : (c->maps[0].lane_box ? 1u : 0u) | (c->maps[1].lane_box ? 2u : 0u);
            for (int w = 0; w < 2; ++w) { l.forms |= c->maps[w].lane_pair_rows ? 4u << w : 0u; l.y[w] = (uint32_t)c->maps[w].knn.Y; }
            l.forms |= c->lane_rebase ? 16u : 0u;
        }
        l.run = p.run; l.out = c->d_dist_out.get(); l.stats = q.stats.get();
        if (p.env_order) {      // every slot (padding included), in env order, one launch
            l.sorted = nullptr; l.n_sorted = E * p.R8; l.n_terrain = l.n_sorted; l.run = p.env_run;
            HIP_TRY(c, launch_raycast_lane(l, s));
            return ROVER_OK;
        }
        if (p.rocks_staged) {
            HIP_TRY(c, launch_raycast_lane(l, s));
        } else {
            // the terrain rays (the first E x P of the sorted list: terrain bins sort first) through the staged kernel, the rock rays — few per
            // bin, a tenth of them off every cone (the horizontal body rays) — through the culled one, which reads 800 bytes of ids per bin
            // where the staged kernel reads the 3.5 KB of a cell's whole row for one such ray
            CullArgs a = cull_args(c, p, n_valid);
            l.n_sorted = l.n_terrain < n_valid ? l.n_terrain : n_valid;
            a.sorted += l.n_sorted; a.n_sorted -= l.n_sorted; a.n_terrain = 0;
            a.stats += lane_waves(l.n_sorted, l.run);
            // (the two launches touch disjoint rays, results and counters; side by side on a second stream they measured slower: 125 against
            //  127 M env-steps/s)
            HIP_TRY(c, launch_raycast_lane(l, s));
            if (a.n_sorted) HIP_TRY(c, launch_raycast_culled(a, s));
        }
    } else if (p.variant == 3)
        HIP_TRY(c, launch_raycast_culled(cull_args(c, p, n_valid), s));
    else if (p.variant == 2)
        HIP_TRY(c, launch_raycast_binned(c->d_rays.get(), c->d_sorted.get(), n_valid, c->maps[0].knn.table, c->maps[1].knn.table,
                                         (uint32_t)c->maps[0].knn.K8, (uint32_t)c->maps[1].knn.K8, p.run, p.proof != 0, c->knobs.early_out, c->d_dist_out.get(), s));
    else
        HIP_TRY(c, launch_raycast(c->d_rays.get(), E * p.R8, c->maps[0].knn.table, c->maps[1].knn.table, (uint32_t)c->maps[0].knn.K8,
                                  (uint32_t)c->maps[1].knn.K8, c->d_dist_out.get(), s));
    return ROVER_OK;
}

// The ray pipeline of a step: env records + ray records, the bucket sort by (map, cell), the ray cast -> d_dist_out [E][R8].
// euler_in != NULL (rover_get_depths): the poses come as euler angles, quat / joints / target may be NULL, and the ctx's euler / heading
// state of the last observation is left alone.
static int cast_rays(rover_ctx* c, const float* pos, const float* quat, const float* joints, const float* target, const float* euler_in,
                     hipStream_t s, const float* import_src = nullptr, const float* import_dir = nullptr) {
    const uint32_t E = (uint32_t)c->cfg.num_envs;
    PrepArgs p{};
    const StepPlan& plan = c->plan;
    p.E = E; p.P = (uint32_t)c->P; p.R8 = plan.R8;
    p.pos = pos; p.quat = quat; p.joints = joints; p.target = target; p.euler_in = euler_in;
    p.dist = c->d_dist.get(); p.terrain = c->maps[0].knn; p.rocks = c->maps[1].knn;
    p.rays = c->d_rays.get(); p.euler = euler_in ? nullptr : c->d_euler.get(); p.heading = euler_in ? nullptr : c->d_heading.get();
    if (int r = check_queue(c, plan)) return r;
    const uint32_t n_valid = E * (26u + (uint32_t)c->P);
    p.rocks_bin_offset = (uint32_t)((uint64_t)c->maps[0].knn.X * c->maps[0].knn.Y);
    const bool sorts = plan.sorted;
    if (sorts) p.bin_out = c->d_bins.get();
    p.precision = c->precision;
    p.cell_rcp = c->cell_rcp;
    // the sort's first pass (keys per coarse bucket and tile) inside prep_rays_kernel where a 64-env block's keys lie in one tile: the
    // table is zero between steps (allocation, then the sort's last kernel) — unless a step failed half way
    // (caller-supplied rays, rover_cast_rays: import_rays_kernel writes the records and keys, the sort counts its keys itself)
    const bool hist_fused = !import_src && plan.hist_fused;
    if (hist_fused) {
        if (c->bkt_table_dirty) HIP_TRY(c, hipMemsetAsync(c->d_bkt_table.get(), 0, c->d_bkt_table.bytes(), s));
        c->bkt_table_dirty = true;
        p.hist = c->d_bkt_table.get(); p.hist_low_bits = plan.low_bits; p.hist_buckets = bucket_count(plan); p.hist_blocks_per_tile = plan.hist_blocks_per_tile;
    }
    if (import_src) {
        // caller-supplied directions: the culled / staged ray cast's proofs need them of unit length (what -normalize() gives)
        uint32_t* const not_unit = plan.variant >= 3 ? c->d_block_cnt.get() + (size_t)c->cfg.num_envs / 256 + 1 : nullptr;      // (the spare word behind the block counts)
        if (not_unit) HIP_TRY(c, hipMemsetAsync(not_unit, 0, sizeof(uint32_t), s));
        HIP_TRY(c, launch_import_rays(import_src, import_dir, E, plan.R8, (uint32_t)c->P, c->maps[0].knn, c->maps[1].knn, p.rocks_bin_offset, c->precision,
                                      c->cell_rcp, c->d_rays.get(), sorts ? c->d_bins.get() : nullptr, s, not_unit));
        if (not_unit) {
            uint32_t bad = 0;
            HIP_TRY(c, hipMemcpyAsync(&bad, not_unit, sizeof bad, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            if (bad) {
                c->rays_valid = false;
                return fail(c, ROVER_E_INVALID, "cast_rays: %u directions are not of unit length (|d|^2 within %g of 1: pass -normalize(direction) as "
                            "rover_export_rays returns it, or use raycast_variant 1 / 2, which evaluate every triangle)", bad, c->precision == 2 ? 4.0e-3 : 1.0e-5);
            }
        }
    } else {
        HIP_TRY(c, launch_prep(p, s));
    }
    if (sorts)
        HIP_TRY(c, launch_bin_rays(c->d_bins.get(), E * plan.R8, n_valid, (uint32_t)plan.n_bins, plan.low_bits, plan.sort_entry_dwords == 1,
                                   c->d_bkt_table.get(), c->d_pairs.get(), c->d_block_sums.get(), c->d_sorted.get(), hist_fused, s));
    // fused histogram: bucket_sort_kernel has cleared the table again; otherwise the table (if the sort ran) holds this step's offsets
    if (sorts) c->bkt_table_dirty = !hist_fused;        // (variant 1 does not touch the table)
    const bool timed = c->profiling && (c->prof_seen++ % c->prof_every) == 0;
    if (timed) {
        if (c->prof_pending == kProfRing && prof_drain(c)) return fail(c, ROVER_E_HIP, "profiling: event drain failed");
        HIP_TRY(c, hipEventRecord(c->ev0[c->prof_pending], s));
    }
    if (int r = run_raycast(c, plan, n_valid, s)) return r;
    if (timed) {
        HIP_TRY(c, hipEventRecord(c->ev1[c->prof_pending], s));
        ++c->prof_pending;
        ++c->prof_launches;
    }
    c->ws_plan = plan;
    c->rays_valid = true;
    return ROVER_OK;
}

// launch_obs false (rover_step): the obs pass is left to the caller, which hands *obs_args to do_metrics — one grid for both passes
static int do_observations(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, hipStream_t s, bool launch_obs, ObsArgs* obs_args) {
    if (!in->pos || !in->quat || !in->joints || !in->target || !in->lin_hist || !in->ang_hist)
        return fail(c, ROVER_E_INVALID, "get_observations: null input pointer");
    if (!out->obs) return fail(c, ROVER_E_INVALID, "get_observations: obs is required");
    const uint32_t E = (uint32_t)c->cfg.num_envs, W = (uint32_t)(4 + c->Ns + c->Nd);
    const int64_t stride = out->obs_stride ? out->obs_stride : (int64_t)W;
    if (stride < (int64_t)W) return fail(c, ROVER_E_INVALID, "obs_stride %lld < row width %u", (long long)stride, W);
    if (int r = cast_rays(c, in->pos, in->quat, in->joints, in->target, nullptr, s)) return r;
    c->obs_valid = true;
    ObsArgs o{};
    o.E = E; o.W = W; o.R8 = c->plan.R8; o.obs_stride = stride;
    o.pos = in->pos; o.target = in->target; o.heading = c->d_heading.get(); o.lin_hist = in->lin_hist; o.ang_hist = in->ang_hist;
    o.dist = c->d_dist_out.get(); o.obs_idx = c->d_obs_idx.get(); o.obs = out->obs; o.fp16_div = c->precision == 2;
    if (launch_obs) HIP_TRY(c, launch_assemble_obs(o, s));
    *obs_args = o;
    if (out->ray_dist || out->wheel_dist || out->body_dist || out->ray_src || out->hit_pt)
        HIP_TRY(c, launch_export_dist(c->d_dist_out.get(), c->d_rays.get(), E, c->plan.R8, (uint32_t)c->P, c->precision, out->ray_dist, out->wheel_dist,
                                      out->body_dist, out->ray_src, out->hit_pt, s));
    if (out->euler) HIP_TRY(c, hipMemcpyAsync(out->euler, c->d_euler.get(), (uint64_t)E * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (out->heading_diff) HIP_TRY(c, hipMemcpyAsync(out->heading_diff, c->d_heading.get(), (uint64_t)E * sizeof(float), hipMemcpyDeviceToDevice, s));
    return ROVER_OK;
}

// with_obs != NULL: the obs pass of a do_observations(launch_obs = false) runs in the same launch
static int do_metrics(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, int inc, int coll, int met, int done,
                      hipStream_t s, bool count_done = false, const ObsArgs* with_obs = nullptr) {
    if (!in->pos || !in->target) return fail(c, ROVER_E_INVALID, "metrics/done: null input pointer");
    if ((inc || met || done) && !in->progress) return fail(c, ROVER_E_INVALID, "metrics/done: progress is required");
    if (!out->rock_collision) return fail(c, ROVER_E_INVALID, "metrics/done: rock_collision is required");
    if (met && (!in->joints || !in->lin_hist || !in->ang_hist || !out->rew))
        return fail(c, ROVER_E_INVALID, "calculate_metrics: joints, lin_hist, ang_hist and rew are required");
    if (done && (!in->euler_pre || !out->reset)) return fail(c, ROVER_E_INVALID, "is_done: euler_pre and reset are required");
    if (coll && out->stone_collision) {
        if (!c->have_stones) return fail(c, ROVER_E_STATE, "stone_collision: rover_set_stones first");
        if (!(out->stone_margin <= 1.4f)) return fail(c, ROVER_E_INVALID, "stone_margin %g exceeds the 1.4 m reach of the stone grid", (double)out->stone_margin);
    }
    MetricsArgs m{};
    m.E = (uint32_t)c->cfg.num_envs; m.R8 = c->plan.R8;
    m.curriculum_level = c->cfg.curriculum_level; m.max_episode_length = c->cfg.max_episode_length;
    m.num_envs_global = c->cfg.num_envs_global;
    m.do_increment = inc; m.do_collision = coll; m.do_metrics = met; m.do_done = done;
    m.pos_reward = c->cfg.pos_reward; m.heading_contraint_reward = c->cfg.heading_contraint_reward;
    m.motion_contraint_reward = c->cfg.motion_contraint_reward; m.goal_angle_reward = c->cfg.goal_angle_reward;
    m.boogie_contraint_reward = c->cfg.boogie_contraint_reward;
    m.wheel_thr = c->precision == 2 ? 0.7998046875f : 0.8f;                // fp16(0.8), fp16(0.45): Python scalars compared
    m.body_thr = c->precision == 2 ? 0.449951171875f : 0.45f;              // against fp16 tensors (rover.py:667-668)
    m.pos = in->pos; m.target = in->target; m.joints = in->joints; m.lin_hist = in->lin_hist; m.ang_hist = in->ang_hist;
    m.euler_pre = in->euler_pre; m.heading = c->d_heading.get(); m.dist = c->d_dist_out.get();
    m.progress = in->progress; m.rock_collision = out->rock_collision; m.rew = out->rew; m.reset = out->reset;
    m.ex_pos_reward = out->ex_pos_reward; m.ex_collision = out->ex_collision_penalty; m.ex_upright = out->ex_uprightness_penalty;
    m.ex_heading = out->ex_heading_contraint_penalty; m.ex_motion = out->ex_motion_contraint_penalty;
    m.block_cnt = count_done ? c->d_block_cnt.get() : nullptr;
    m.stone_collision = coll ? out->stone_collision : nullptr; m.stone_margin = out->stone_margin;
    m.done_u8 = done ? out->done_u8 : nullptr;
    m.sgrid = c->sgrid; m.info7 = c->d_stones.get();
    m.ex_goal_angle = out->ex_goal_angle_penalty; m.ex_lin = out->ex_torque_penalty_driving; m.ex_ang = out->ex_torque_penalty_steering;
    // the evaluation latch: check_collision's update (rover.py:670-672, level >= 2 only) and is_done's (:620-631); never metrics alone
    if (c->eval_on && ((coll && c->cfg.curriculum_level >= 2) || done)) {
        if (!in->progress) return fail(c, ROVER_E_INVALID, "evaluation: progress is required (the latch records it)");
        m.eval_res = c->d_eval_res.get(); m.eval_step = c->d_eval_step.get();
    }
    if (with_obs) HIP_TRY(c, launch_obs_metrics(*with_obs, m, s));
    else HIP_TRY(c, launch_metrics_done(m, s));
    return ROVER_OK;
}

int rover_get_observations(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "get_observations: null struct");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    ObsArgs o{};
    if (int r = do_observations(c, in, out, s, true, &o)) return r;
    if (!out->rock_collision) return ROVER_OK;
    // check_collision (rover.py:292-293) is part of get_observations: run only the collision stage
    return do_metrics(c, in, out, 0, 1, 0, 0, s);
}

int rover_calculate_metrics(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "calculate_metrics: null struct");
    if (int r = check_ready(c)) return r;
    if (!c->obs_valid) return fail(c, ROVER_E_STATE, "calculate_metrics: call rover_get_observations first (rover.py:479 reads self.heading_diff)");
    USE_DEVICE(c);
    return do_metrics(c, in, out, 0, 0, 1, 0, (hipStream_t)stream);
}

int rover_is_done(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "is_done: null struct");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    return do_metrics(c, in, out, 0, 0, 0, 1, (hipStream_t)stream);
}

int rover_get_depths(rover_ctx* c, const float* positions, const float* rotations_euler, float* distances, float* points,
                     float* sources, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!positions || !rotations_euler) return fail(c, ROVER_E_INVALID, "get_depths: positions and rotations are required");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (int r = cast_rays(c, positions, nullptr, nullptr, nullptr, rotations_euler, s)) return r;
    if (distances || points || sources)
        HIP_TRY(c, launch_export_dist(c->d_dist_out.get(), c->d_rays.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, c->precision, distances,
                                      nullptr, nullptr, sources, points, s));
    return ROVER_OK;
}

int rover_get_collisions(rover_ctx* c, const float* positions, const float* rotations_euler, const float* joints, float* wheel_dist,
                         float* body_dist, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!positions || !rotations_euler) return fail(c, ROVER_E_INVALID, "get_collisions: positions and rotations are required");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (int r = cast_rays(c, positions, nullptr, joints, nullptr, rotations_euler, s)) return r;
    if (wheel_dist || body_dist)
        HIP_TRY(c, launch_export_dist(c->d_dist_out.get(), c->d_rays.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, c->precision, nullptr,
                                      wheel_dist, body_dist, nullptr, nullptr, s));
    return ROVER_OK;
}

int rover_export_rays(rover_ctx* c, float* src, float* dir, int32_t* cell, float* dist, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (int r = check_ready(c)) return r;
    if (!c->rays_valid) return fail(c, ROVER_E_STATE, "export_rays: no ray records yet (run a step first)");
    USE_DEVICE(c);
    HIP_TRY(c, launch_export_rays(c->d_rays.get(), c->d_dist_out.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, src, dir, cell, dist,
                                  (hipStream_t)stream));
    return ROVER_OK;
}

int rover_cast_rays(rover_ctx* c, const float* src, const float* dir, float* dist, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!src || !dir || !dist) return fail(c, ROVER_E_INVALID, "cast_rays: src, dir and dist are required");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (int r = cast_rays(c, nullptr, nullptr, nullptr, nullptr, nullptr, s, src, dir)) return r;
    HIP_TRY(c, launch_export_rays(c->d_rays.get(), c->d_dist_out.get(), (uint32_t)c->cfg.num_envs, c->plan.R8, (uint32_t)c->P, nullptr, nullptr, nullptr, dist, s));
    return ROVER_OK;
}

int rover_compact_resets(rover_ctx* c, const int64_t* reset, int64_t* ids, int32_t* n_reset, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!reset || !ids || !n_reset) return fail(c, ROVER_E_INVALID, "compact_resets: null pointer");
    USE_DEVICE(c);
    HIP_TRY(c, launch_compact(reset, (uint32_t)c->cfg.num_envs, (int64_t)c->cfg.env_offset, c->d_block_cnt.get(), false, ids, n_reset,
                              (hipStream_t)stream));
    return ROVER_OK;
}

int rover_step(rover_ctx* c, const rover_step_in* in, const rover_step_out* out, uint32_t flags, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!in || !out) return fail(c, ROVER_E_INVALID, "step: null struct");
    if (int r = check_ready(c)) return r;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if ((flags & ROVER_STEP_COMPACT) && (!out->reset_ids || !out->n_reset))
        return fail(c, ROVER_E_INVALID, "step: ROVER_STEP_COMPACT needs reset_ids and n_reset");
    ObsArgs o{};                      // the obs pass is launched by do_metrics, in one grid with the metrics pass
    if (int r = do_observations(c, in, out, s, false, &o)) return r;
    const bool compact = (flags & ROVER_STEP_COMPACT) != 0;
    if (int r = do_metrics(c, in, out, (flags & ROVER_STEP_INCREMENT_PROGRESS) ? 1 : 0, 1, 1, 1, s, compact, &o)) return r;
    if (compact)
        HIP_TRY(c, launch_compact(out->reset, (uint32_t)c->cfg.num_envs, (int64_t)c->cfg.env_offset, c->d_block_cnt.get(), true,
                                  out->reset_ids, out->n_reset, s));
    return ROVER_OK;
}

// ---- evaluation mode -------------------------------------------------------------------------------
int rover_set_evaluation(rover_ctx* c, int32_t enable) {
    if (!c) return ROVER_E_INVALID;
    USE_DEVICE(c);
    c->eval_on = false;
    c->d_eval_res.reset(); c->d_eval_step.reset();
    if (!enable) return ROVER_OK;
    const size_t E = (size_t)c->cfg.num_envs;
    HIP_TRY(c, c->d_eval_res.alloc(E));
    HIP_TRY(c, c->d_eval_step.alloc(E));
    HIP_TRY(c, hipMemset(c->d_eval_res.get(), 0, c->d_eval_res.bytes()));
    HIP_TRY(c, hipMemset(c->d_eval_step.get(), 0, c->d_eval_step.bytes()));
    HIP_TRY(c, hipDeviceSynchronize());
    c->eval_on = true;
    return ROVER_OK;
}

int rover_eval_clear(rover_ctx* c, const int64_t* env_ids, int32_t n, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->eval_on) return fail(c, ROVER_E_STATE, "eval_clear: evaluation is off (rover_set_evaluation(ctx, 1) first)");
    const int32_t E = c->cfg.num_envs;
    if (env_ids && (n < 0 || n > E)) return fail(c, ROVER_E_INVALID, "eval_clear: n = %d outside [0, %d]", n, E);
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (env_ids && n > 0) {                 // the ids are checked on the host: the call waits for the stream that wrote them
        std::vector<int64_t> h((size_t)n);
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipMemcpy(h.data(), env_ids, h.size() * sizeof(int64_t), hipMemcpyDefault));
        for (int32_t i = 0; i < n; ++i)
            if (h[i] < 0 || h[i] >= E) return fail(c, ROVER_E_INVALID, "eval_clear: env id %lld outside [0, %d)", (long long)h[i], E);
    }
    HIP_TRY(c, launch_eval_clear(c->d_eval_res.get(), c->d_eval_step.get(), (uint32_t)E, env_ids, env_ids ? (uint32_t)n : (uint32_t)E, s));
    return ROVER_OK;
}

int rover_eval_read(rover_ctx* c, int64_t* eval_res, int64_t* eval_step, int64_t* summary8, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->eval_on) return fail(c, ROVER_E_STATE, "eval_read: evaluation is off (rover_set_evaluation(ctx, 1) first)");
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t bytes = (uint64_t)c->cfg.num_envs * sizeof(int64_t);
    if (eval_res) HIP_TRY(c, hipMemcpyAsync(eval_res, c->d_eval_res.get(), bytes, hipMemcpyDeviceToDevice, s));
    if (eval_step) HIP_TRY(c, hipMemcpyAsync(eval_step, c->d_eval_step.get(), bytes, hipMemcpyDeviceToDevice, s));
    if (summary8) HIP_TRY(c, launch_eval_summary(c->d_eval_res.get(), c->d_eval_step.get(), (uint32_t)c->cfg.num_envs, summary8, s));
    return ROVER_OK;
}

int rover_quat_to_euler(rover_ctx* c, const float* quat, float* euler, int32_t n, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!quat || !euler || n < 0) return fail(c, ROVER_E_INVALID, "quat_to_euler: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_quat_to_euler(quat, euler, (uint32_t)n, (hipStream_t)stream));
    return ROVER_OK;
}

// ---- reset path ------------------------------------------------------------------------------------
int rover_clearance(rover_ctx* c, const float* xy, int32_t n, float* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_stones) return fail(c, ROVER_E_STATE, "clearance: rover_set_stones first");
    if (n < 0 || (n > 0 && (!xy || !out))) return fail(c, ROVER_E_INVALID, "clearance: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_clearance(c->d_stones.get(), (uint32_t)c->S, xy, (uint32_t)n, out, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_shift_spawns(rover_ctx* c, float* pos3, int32_t n, int32_t max_iter, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_stones) return fail(c, ROVER_E_STATE, "shift_spawns: rover_set_stones first");
    if (n < 0 || (n > 0 && !pos3) || max_iter < 0) return fail(c, ROVER_E_INVALID, "shift_spawns: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_shift_spawns(c->sgrid, c->d_stones.get(), pos3, (uint32_t)n, max_iter, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_sample_height(rover_ctx* c, const float* xy, int32_t n, float* out, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "sample_height: rover_set_heightfield first");
    if (n < 0 || (n > 0 && (!xy || !out))) return fail(c, ROVER_E_INVALID, "sample_height: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_sample_height(c->hf, xy, (uint32_t)n, out, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_generate_goals(rover_ctx* c, const int64_t* env_ids, int32_t n, const float* initial_pos3, float* target3, float radius,
                         const float* draws, int32_t max_draws, uint64_t seed, int32_t* n_draws_used, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!c->have_stones || !c->have_hf) return fail(c, ROVER_E_STATE, "generate_goals: rover_set_stones and rover_set_heightfield first");
    if (n < 0 || n > c->cfg.num_envs || (n > 0 && (!env_ids || !initial_pos3 || !target3)) || max_draws <= 0)
        return fail(c, ROVER_E_INVALID, "generate_goals: bad arguments (n=%d, max_draws=%d)", n, max_draws);
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    GoalArgs g{c->d_stones.get(), (uint32_t)c->S, c->hf, c->sgrid, env_ids, 0, (uint32_t)n, nullptr, initial_pos3, target3, radius, draws,
               max_draws, seed, nullptr, (int32_t*)c->d_goal_work.get(), n_draws_used};
    HIP_TRY(c, launch_generate_goals(g, (uint32_t)n, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_reset_envs(rover_ctx* c, const rover_reset_io* io, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!io) return fail(c, ROVER_E_INVALID, "reset_envs: null struct");
    if (!io->reset_ids || !io->initial_pos3 || !io->pos3 || !io->quat4 || !io->reset || !io->progress)
        return fail(c, ROVER_E_INVALID, "reset_envs: reset_ids, initial_pos3, pos3, quat4, reset and progress are required");
    if (!io->n_reset_dev && (io->n_reset_host < 0 || io->n_reset_host > c->cfg.num_envs))
        return fail(c, ROVER_E_INVALID, "reset_envs: n_reset_host=%d out of range", io->n_reset_host);
    if (io->draws && io->n_reset_dev) return fail(c, ROVER_E_INVALID, "reset_envs: caller-supplied draws need n_reset_host");
    // yaw_deg[i] is read for every i < n: with the count on the device n can be any value up to num_envs
    if (io->yaw_deg && io->yaw_deg_len < (io->n_reset_dev ? c->cfg.num_envs : io->n_reset_host))
        return fail(c, ROVER_E_INVALID, "reset_envs: yaw_deg holds %d entries, %d may be read", io->yaw_deg_len,
                    io->n_reset_dev ? c->cfg.num_envs : io->n_reset_host);
    if (io->target3 && (!c->have_stones || !c->have_hf))
        return fail(c, ROVER_E_STATE, "reset_envs: goal validation needs rover_set_stones and rover_set_heightfield");
    if (!io->n_reset_dev && io->n_reset_host == 0) return ROVER_OK;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    ResetArgs a{};
    a.ids = io->reset_ids; a.id_offset = c->cfg.env_offset; a.n_host = (uint32_t)io->n_reset_host; a.n_dev = io->n_reset_dev;
    a.initial_pos3 = io->initial_pos3; a.pos3 = io->pos3; a.quat4 = io->quat4; a.joint_pos13 = io->joint_pos13;
    a.joint_vel13 = io->joint_vel13; a.base_pos3 = io->base_pos3; a.reset = io->reset; a.progress = io->progress;
    a.yaw_deg = io->yaw_deg; a.seed = io->seed; a.seed_dev = io->seed_dev;
    const uint32_t n_max = io->n_reset_dev ? (uint32_t)c->cfg.num_envs : (uint32_t)io->n_reset_host;
    HIP_TRY(c, launch_reset_envs(a, n_max, s));
    if (io->target3) {
        GoalArgs g{c->d_stones.get(), (uint32_t)c->S, c->hf, c->sgrid, io->reset_ids, (int64_t)c->cfg.env_offset, (uint32_t)io->n_reset_host,
                   io->n_reset_dev, io->initial_pos3, io->target3, io->radius > 0.f ? io->radius : 8.0f, io->draws,
                   io->max_draws > 0 ? io->max_draws : 256, io->seed, io->seed_dev, (int32_t*)c->d_goal_work.get(), io->n_draws_used};
        HIP_TRY(c, launch_generate_goals(g, n_max, s));
    }
    return ROVER_OK;
}

int rover_pre_physics_step(rover_ctx* c, const float* actions, const float* quat, float* lin_hist, float* ang_hist,
                           float* euler_pre, float* pos_targets13, float* vel_targets13, float* actions_nn, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!actions || !lin_hist || !ang_hist) return fail(c, ROVER_E_INVALID, "pre_physics_step: actions and both histories are required");
    if (euler_pre && !quat) return fail(c, ROVER_E_INVALID, "pre_physics_step: euler_pre needs quat");
    USE_DEVICE(c);
    PrePhysicsArgs a{(uint32_t)c->cfg.num_envs, actions, quat, lin_hist, ang_hist, euler_pre, pos_targets13, vel_targets13, actions_nn};
    HIP_TRY(c, launch_pre_physics(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_ackermann(rover_ctx* c, const float* lin, const float* ang, int32_t n, float* steering, float* velocities, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (n < 0 || (n > 0 && (!lin || !ang || !steering || !velocities))) return fail(c, ROVER_E_INVALID, "ackermann: bad arguments");
    if (n == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_ackermann(lin, ang, (uint32_t)n, steering, velocities, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_get_info(const rover_ctx* c, rover_info* info) {
    if (!c || !info) return ROVER_E_INVALID;
    memset(info, 0, sizeof *info);
    info->P = c->P; info->Ns = c->Ns; info->Nd = c->Nd; info->rays_per_env_padded = (int32_t)c->plan.R8;
    for (int w = 0; w < 2; ++w) {
        info->K[w] = c->maps[w].knn.K; info->K8[w] = c->maps[w].knn.K8; info->X[w] = c->maps[w].knn.X; info->Y[w] = c->maps[w].knn.Y;
        info->table_bytes[w] = c->maps[w].bytes();
    }
    // the per-step workspace: ray records, distances, sort buffers, env records, and the culled ray cast's queue + counters
    info->workspace_bytes = c->workspace_bytes + c->queue.entries.bytes() + c->queue.stats.bytes();
    info->raycast_variant = c->plan.variant;
    info->cell_index_mode = c->cell_rcp; info->ray_precision = c->precision;
    info->raycast_sorted = c->plan.sorted ? 1 : 0;
    info->raycast_rocks_staged = c->plan.rocks_staged ? 1 : 0;
    for (int w = 0; w < 2; ++w) { info->lane_box[w] = c->maps[w].lane_box ? 1 : 0; info->lane_pair_rows[w] = c->maps[w].lane_pair_rows ? 1 : 0; }
    return ROVER_OK;
}

int rover_get_raycast_plan(const rover_ctx* c, rover_raycast_plan* out) {
    if (!c || !out) return ROVER_E_INVALID;
    memset(out, 0, sizeof *out);
    plan_to_c(c->plan, out);
    return ROVER_OK;
}

int rover_get_cull_info(rover_ctx* c, rover_cull_info* out) {
    if (!c || !out) return ROVER_E_INVALID;
    memset(out, 0, sizeof *out);
    for (int w = 0; w < 2; ++w) {             // (of the proof tables the precision in force uses)
        const MapTables& m = c->maps[w];
        out->triangles[w] = m.tris;
        out->always_candidate_triangles[w] = m.proof[c->plan.proof].always;
        out->cells_without_cone[w] = m.proof[c->plan.proof].nocone;
        out->cells_with_far_bound[w] = m.farok;
    }
    out->far_records_on_demand = (c->have_dist && c->maps[0].table.get()) ? (uint64_t)c->plan.lazy_far : 0;
    const CullQueue& q = c->queue;
    out->queue_bytes = q.entries.bytes();
    out->launches_per_step = q.entries.get() ? q.sized_for.cull_launches : 0;
    if (!q.stats.get() || c->ws_plan.variant < 3) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, hipDeviceSynchronize());
    std::vector<uint4> h(q.stats.bytes() / sizeof(uint4));
    HIP_TRY(c, hipMemcpy(h.data(), q.stats.get(), q.stats.bytes(), hipMemcpyDeviceToHost));
    for (const uint4& v : h) {
        out->candidate_pairs += v.x; out->rays += v.y & 0xffu; out->rays_far_skipped += v.y >> 8; out->rays_both_tests += v.z & 0xffu; out->rays_not_scanned += v.z >> 8; out->bins += v.w & 0xffu;
        out->lane_items += (v.w >> 8) & 0x3ffffu; out->lane_flushes += v.w >> 26;      // (zero in the words the culled kernel's waves write)
        out->max_pairs_per_run = v.x > out->max_pairs_per_run ? v.x : out->max_pairs_per_run;
    }
    return ROVER_OK;
}

// IEEE binary16 <-> binary32 on the host (round to nearest even), for the reference-ranking coordinate tables
static float half_bits_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) u = sign;
        else { int e = -1; uint32_t m = man; do { ++e; m <<= 1; } while (!(m & 0x400u)); u = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3ffu) << 13); }
    } else if (exp == 31) u = sign | 0x7f800000u | (man << 13);
    else u = sign | ((exp + 112u) << 23) | (man << 13);
    float f; memcpy(&f, &u, sizeof f); return f;
}
static uint16_t float_to_half_bits(float f) {
    uint32_t u; memcpy(&u, &f, sizeof u);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (u > 0x7f800000u ? 0x200u : 0u));
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                        // rounds to infinity
    if (u < 0x38800000u) {                                                         // subnormal half or zero
        if (u < 0x33000000u) return (uint16_t)sign;
        const int shift = 126 - (int)(u >> 23);                                    // 14 .. 24
        const uint32_t m = (u & 0x7fffffu) | 0x800000u;
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (r & 1u))) ++r;
        return (uint16_t)(sign | r);
    }
    uint32_t r = (u - 0x38000000u) >> 13;
    const uint32_t rem = u & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
}

static int build_knn_map_impl(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                              float res, int32_t K, int ref, const uint16_t* cell_x_f16, const uint16_t* cell_y_f16,
                              int32_t* map_idx_out);

int rover_build_knn_map(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                        float res, int32_t K, int32_t* map_idx_out) {
    return build_knn_map_impl(c, vertices, V, triangles, T, X, Y, res, K, 0, nullptr, nullptr, map_idx_out);
}

int rover_build_knn_map_ref(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                            float res, int32_t K, const uint16_t* cell_x_f16, const uint16_t* cell_y_f16, int32_t* map_idx_out) {
    return build_knn_map_impl(c, vertices, V, triangles, T, X, Y, res, K, 1, cell_x_f16, cell_y_f16, map_idx_out);
}

static int build_knn_map_impl(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t X, int32_t Y,
                              float res, int32_t K, int ref, const uint16_t* cell_x_f16, const uint16_t* cell_y_f16,
                              int32_t* map_idx_out) {
    if (!c) return ROVER_E_INVALID;
    if (!vertices || !triangles || !map_idx_out || V <= 0 || T <= 0 || X <= 0 || Y <= 0 || K <= 0 || !(res > 0.0f))
        return fail(c, ROVER_E_INVALID, "build_knn_map: bad arguments");
    if (T < K) return fail(c, ROVER_E_INVALID, "build_knn_map: the mesh has %d triangles, fewer than K=%d", T, K);
    if (K > 4096) return fail(c, ROVER_E_INVALID, "build_knn_map: K=%d exceeds the builder's limit of 4096", K);
    USE_DEVICE(c);
    DevBuf<float> d_v, d_cx, d_cy, d_cell;
    DevBuf<int32_t> d_t, d_over;
    DevBuf<uint32_t> d_cur, d_items, d_bs, d_start;
#define KNN_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) return fail(c, ROVER_E_HIP, "build_knn_map: %s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)
    KNN_TRY(d_v.alloc((size_t)V * 3));
    KNN_TRY(d_t.alloc((size_t)T * 3));
    KNN_TRY(d_cx.alloc(T));
    KNN_TRY(d_cy.alloc(T));
    KNN_TRY(d_items.alloc(T));
    KNN_TRY(d_over.alloc(1));
    KNN_TRY(d_bs.alloc(8192));
    KNN_TRY(hipMemcpy(d_v.get(), vertices, d_v.bytes(), hipMemcpyDefault));
    KNN_TRY(hipMemcpy(d_t.get(), triangles, d_t.bytes(), hipMemcpyDefault));
    KNN_TRY(hipMemset(d_over.get(), 0, sizeof(int32_t)));
    KNN_TRY(launch_knn_centroids(d_v.get(), d_t.get(), (uint32_t)T, (uint32_t)V, ref, d_cx.get(), d_cy.get(), nullptr));
    if (ref) {
        // cell coordinates as fp16 values: the caller's tables (what the reference's torch.arange(0, X res, res, dtype=float16)
        // gave on the host that built the map), or fp16(float(i) * res) — ATen's CUDA arange kernel, the reference's own device
        std::vector<float> cell((size_t)X + (size_t)Y);
        std::vector<uint16_t> hx((size_t)X), hy((size_t)Y);
        if (cell_x_f16) KNN_TRY(hipMemcpy(hx.data(), cell_x_f16, hx.size() * sizeof(uint16_t), hipMemcpyDefault));
        if (cell_y_f16) KNN_TRY(hipMemcpy(hy.data(), cell_y_f16, hy.size() * sizeof(uint16_t), hipMemcpyDefault));
        for (int32_t i = 0; i < X; ++i) cell[(size_t)i] = half_bits_to_float(cell_x_f16 ? hx[(size_t)i] : float_to_half_bits((float)i * res));
        for (int32_t j = 0; j < Y; ++j) cell[(size_t)X + j] = half_bits_to_float(cell_y_f16 ? hy[(size_t)j] : float_to_half_bits((float)j * res));
        KNN_TRY(d_cell.alloc(cell.size()));
        KNN_TRY(hipMemcpy(d_cell.get(), cell.data(), d_cell.bytes(), hipMemcpyHostToDevice));
    }
    // bucket grid over the centroids' bounding box; bucket edge ~ the radius that holds K/4 centroids at mean density
    std::vector<float> hx((size_t)T), hy((size_t)T);
    KNN_TRY(hipMemcpy(hx.data(), d_cx.get(), d_cx.bytes(), hipMemcpyDeviceToHost));
    KNN_TRY(hipMemcpy(hy.data(), d_cy.get(), d_cy.bytes(), hipMemcpyDeviceToHost));
    // (NaN centroids are left out of the box, the first triangle's included: they all land in bucket 0 and rank last)
    float x0 = 0.0f, x1 = 0.0f, y0 = 0.0f, y1 = 0.0f;
    bool any_x = false, any_y = false;
    for (int32_t t = 0; t < T; ++t) {
        if (hx[t] == hx[t]) { x0 = (any_x && x0 < hx[t]) ? x0 : hx[t]; x1 = (any_x && x1 > hx[t]) ? x1 : hx[t]; any_x = true; }
        if (hy[t] == hy[t]) { y0 = (any_y && y0 < hy[t]) ? y0 : hy[t]; y1 = (any_y && y1 > hy[t]) ? y1 : hy[t]; any_y = true; }
    }
    // the largest |coordinate - origin| of any centroid or cell point: knn_select_kernel's stop slack is absolute in it
    const double cell_x1 = (double)((float)(X - 1) * res), cell_y1 = (double)((float)(Y - 1) * res);
    const float span = (float)std::max({(double)x1 - x0, (double)y1 - y0, std::fabs((double)x0), std::fabs(cell_x1 - x0), std::fabs((double)y0),
                                        std::fabs(cell_y1 - y0)});
    const double area = ((double)x1 - x0 + 1e-6) * ((double)y1 - y0 + 1e-6);
    // (an infinite centroid would make the bucket edge infinite or NaN, and the sizing below would never settle)
    if (!std::isfinite(area)) return fail(c, ROVER_E_INVALID, "build_knn_map: the centroids' bounding box is not finite");
    double gsz = std::sqrt(area * (double)K / (4.0 * (double)T));
    if (gsz < (double)res) gsz = (double)res;
    // A cell's search gathers whole rings of buckets into LDS (8192 candidates at most).  On a strongly non-uniform mesh (a
    // decimated terrain: millimetre triangles on the rocks, metre-sized ones between them) a ring sized for the MEAN density can
    // hold more than that next to a dense patch: the bucket edge is halved and the search repeated (same result: the ranking
    // does not depend on the bucket size).
    hipError_t e2 = hipSuccess;
    int32_t over = 0;
    for (int attempt = 0; attempt < 6; ++attempt, gsz *= 0.5) {
        uint32_t nbx = (uint32_t)(((double)x1 - x0) / gsz) + 1, nby = (uint32_t)(((double)y1 - y0) / gsz) + 1;
        while ((uint64_t)nbx * nby > (1u << 22)) { gsz *= 2.0; nbx = (uint32_t)(((double)x1 - x0) / gsz) + 1; nby = (uint32_t)(((double)y1 - y0) / gsz) + 1; attempt = 99; }
        const float g = (float)gsz, inv_g = 1.0f / g;
        const uint32_t nb = nbx * nby;
        d_start.reset();
        KNN_TRY(d_cur.alloc((size_t)nb + 1));
        KNN_TRY(hipMemset(d_cur.get(), 0, d_cur.bytes()));
        KNN_TRY(hipMemset(d_over.get(), 0, sizeof(int32_t)));
        KNN_TRY(launch_knn_bucket(d_cx.get(), d_cy.get(), (uint32_t)T, x0, y0, inv_g, nbx, nby, d_cur.get(), d_items.get(), 1, nullptr));
        KNN_TRY(launch_scan_exclusive(d_cur.get(), nb + 1, d_bs.get(), nullptr));
        e2 = d_start.alloc((size_t)nb + 1);
        if (e2 == hipSuccess) e2 = hipMemcpy(d_start.get(), d_cur.get(), d_cur.bytes(), hipMemcpyDeviceToDevice);
        if (e2 == hipSuccess) e2 = launch_knn_bucket(d_cx.get(), d_cy.get(), (uint32_t)T, x0, y0, inv_g, nbx, nby, d_cur.get(), d_items.get(), 0, nullptr);
        if (e2 == hipSuccess) e2 = launch_knn_select(d_cx.get(), d_cy.get(), d_start.get(), d_items.get(), x0, y0, g, span, nbx, nby, (uint32_t)X, (uint32_t)Y,
                                                     res, (uint32_t)K, d_cell.get(), d_cell.get() ? d_cell.get() + X : nullptr, map_idx_out, d_over.get(), nullptr);
        if (e2 == hipSuccess) e2 = hipDeviceSynchronize();
        over = 0;
        if (e2 == hipSuccess) e2 = hipMemcpy(&over, d_over.get(), sizeof over, hipMemcpyDeviceToHost);
        if (e2 != hipSuccess || !over) break;
    }
#undef KNN_TRY
    if (e2 != hipSuccess) return fail(c, ROVER_E_HIP, "build_knn_map: %s", hipGetErrorString(e2));
    if (over) return fail(c, ROVER_E_INVALID, "build_knn_map: a search ring held more than 8192 candidate triangles (mesh too dense for K=%d)", K);
    return ROVER_OK;
}

// Host only: the sizes that separate the rasteriser's routes
int rover_heightfield_limits(int32_t out[4]) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "heightfield_limits: null argument");
    out[0] = RASTER_SMALL_NODES; out[1] = RASTER_TILE_I; out[2] = RASTER_TILE_J; out[3] = RASTER_GROUP;
    return ROVER_OK;
}

// The arguments are validated before the ctx is looked at, as for rover_motion_step
int rover_build_heightfield(rover_ctx* c, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, int32_t N0, int32_t N1,
                            float horizontal_scale, float shift_x, float shift_y, float fill, float* hm_out, int64_t stats[2]) {
    if (N0 < 1 || N1 < 1 || N0 > RASTER_MAX_NODES || N1 > RASTER_MAX_NODES)
        return fail(c, ROVER_E_INVALID, "build_heightfield: N0 = %d or N1 = %d is outside 1 .. %d", N0, N1, RASTER_MAX_NODES);
    if (!std::isfinite(horizontal_scale) || !(horizontal_scale > 0.0f))
        return fail(c, ROVER_E_INVALID, "build_heightfield: horizontal_scale = %g is not finite or not > 0", (double)horizontal_scale);
    if (!std::isfinite(shift_x) || !std::isfinite(shift_y))
        return fail(c, ROVER_E_INVALID, "build_heightfield: shift = (%g, %g) is not finite", (double)shift_x, (double)shift_y);
    if (V < 0 || T < 0) return fail(c, ROVER_E_INVALID, "build_heightfield: V = %d or T = %d is negative", V, T);
    if ((V > 0 && !vertices) || (T > 0 && !triangles) || !hm_out)
        return fail(c, ROVER_E_INVALID, "build_heightfield: vertices, triangles and hm_out must be given");
    if (!c) return fail(nullptr, ROVER_E_INVALID, "build_heightfield: null ctx");
    USE_DEVICE(c);
#define HF_TRY(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e__ = (expr);                                                                              \
        if (e__ != hipSuccess) return fail(c, ROVER_E_HIP, "build_heightfield: %s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)
    DevBuf<float> d_v;
    DevBuf<int32_t> d_t;
    DevBuf<uint4> d_snap;
    DevBuf<uint32_t> d_large, d_tiles;
    DevBuf<unsigned long long> d_counts;            // {uncovered, skipped, length of the list}
    DevBuf<uint64_t> d_start;
    const size_t nv = V > 0 ? (size_t)V : 1, nt = T > 0 ? (size_t)T : 1;
    const uint64_t nodes = (uint64_t)N0 * (uint64_t)N1;
    HF_TRY(d_v.alloc(nv * 3));
    HF_TRY(d_t.alloc(nt * 3));
    HF_TRY(d_snap.alloc(nv));
    HF_TRY(d_large.alloc(nt));
    HF_TRY(d_tiles.alloc(nt));
    HF_TRY(d_counts.alloc(3));
    if (V > 0) HF_TRY(hipMemcpy(d_v.get(), vertices, (size_t)V * 3 * sizeof(float), hipMemcpyDefault));
    if (T > 0) HF_TRY(hipMemcpy(d_t.get(), triangles, (size_t)T * 3 * sizeof(int32_t), hipMemcpyDefault));
    HF_TRY(hipMemset(d_counts.get(), 0, d_counts.bytes()));
    HF_TRY(hipMemset(hm_out, 0, nodes * sizeof(float)));                                  // key 0: never covered
    RasterArgs a{};
    a.snap = d_snap.get(); a.tris = d_t.get(); a.V = V; a.T = T; a.N0 = N0; a.N1 = N1;
    a.keys = reinterpret_cast<uint32_t*>(hm_out);
    a.n_large = reinterpret_cast<uint32_t*>(d_counts.get() + 2);
    a.large_tri = d_large.get(); a.large_tiles = d_tiles.get(); a.stats = d_counts.get();
    HF_TRY(launch_raster_snap(d_v.get(), (uint32_t)V, horizontal_scale, shift_x, shift_y, d_snap.get(), nullptr));
    HF_TRY(launch_raster_small(a, nullptr));
    unsigned long long counts[3] = {0, 0, 0};
    HF_TRY(hipMemcpy(counts, d_counts.get(), sizeof counts, hipMemcpyDeviceToHost));      // (synchronises)
    const uint32_t n_large = (uint32_t)(counts[2] & 0xffffffffull);
    if (n_large > (uint32_t)T) return fail(c, ROVER_E_HIP, "build_heightfield: the list holds %u triangles of %d", n_large, T);
    if (n_large) {
        std::vector<uint32_t> tiles(n_large);
        std::vector<uint64_t> start((size_t)n_large + 1);
        HF_TRY(hipMemcpy(tiles.data(), d_tiles.get(), (size_t)n_large * sizeof(uint32_t), hipMemcpyDeviceToHost));
        start[0] = 0;
        for (uint32_t i = 0; i < n_large; ++i) start[(size_t)i + 1] = start[i] + tiles[i];
        HF_TRY(d_start.alloc(start.size()));
        HF_TRY(hipMemcpy(d_start.get(), start.data(), d_start.bytes(), hipMemcpyHostToDevice));
        HF_TRY(launch_raster_large(a, d_start.get(), n_large, start[n_large], nullptr));
    }
    HF_TRY(launch_raster_decode(a.keys, nodes, fill, d_counts.get(), nullptr));
    HF_TRY(hipDeviceSynchronize());
    HF_TRY(hipMemcpy(counts, d_counts.get(), sizeof counts, hipMemcpyDeviceToHost));
#undef HF_TRY
    if (stats) { stats[0] = (int64_t)counts[0]; stats[1] = (int64_t)counts[1]; }
    return ROVER_OK;
}

// ---- Mars terrain generator ----
static_assert(MARS_TILE == ROVER_MARS_TILE, "the kernel's tile is the ABI's");

// shared by rover_mars_heightfield and rover_mars_tiles: true when the descriptor is acceptable, else *why says what is wrong.  This is
// what keeps the kernel inside its buffers: a window or a kept stamp that fails here never reaches the device.
static bool mars_desc_ok(const rover_mars_desc* d, std::string* why) {
    char buf[256];
    buf[0] = 0;
#define MARS_REFUSE(...) do { snprintf(buf, sizeof buf, __VA_ARGS__); *why = buf; return false; } while (0)
    if (!d) MARS_REFUSE("desc is NULL");
    if (d->rows < 1 || d->cols < 1 || d->rows > ROVER_MARS_MAX_SIDE || d->cols > ROVER_MARS_MAX_SIDE)
        MARS_REFUSE("rows = %d or cols = %d is outside 1 .. %d", d->rows, d->cols, ROVER_MARS_MAX_SIDE);
    if (d->n_hills < 0) MARS_REFUSE("n_hills = %d is negative", d->n_hills);
    if (d->n_classes < 0 || d->n_classes > ROVER_MARS_MAX_CLASSES) MARS_REFUSE("n_classes = %d is outside 0 .. %d", d->n_classes, ROVER_MARS_MAX_CLASSES);
    if (d->n_stamps < 0) MARS_REFUSE("n_stamps = %d is negative", d->n_stamps);
    if (d->g_len < 1 || !d->g) MARS_REFUSE("g is NULL or g_len = %d is below 1", d->g_len);
    if (d->n_hills > 0 && (!d->hill_window || !d->hill_amp)) MARS_REFUSE("hill_window or hill_amp is NULL with n_hills = %d", d->n_hills);
    if (d->n_classes > 0 && (!d->class_side || !d->class_tables)) MARS_REFUSE("class_side or class_tables is NULL with n_classes = %d", d->n_classes);
    if (d->n_stamps > 0 && (!d->stamp_row || !d->stamp_col || !d->stamp_class || !d->stamp_factor || !d->stamp_kept))
        MARS_REFUSE("a stamp array is NULL with n_stamps = %d", d->n_stamps);
    for (int32_t k = 0; k < d->n_classes; ++k)
        if (d->class_side[k] < 1 || d->class_side[k] > ROVER_MARS_MAX_TABLE)
            MARS_REFUSE("class_side[%d] = %d is outside 1 .. %d", k, d->class_side[k], ROVER_MARS_MAX_TABLE);
    for (int32_t i = 0; i < d->n_hills; ++i) {
        const int32_t* w = d->hill_window + 6 * (size_t)i;
        const int64_t r0 = w[0], r1 = w[1], c0 = w[2], c1 = w[3], a0 = w[4], b0 = w[5];
        if (r0 < 0 || r1 < r0 || r1 > d->rows || c0 < 0 || c1 < c0 || c1 > d->cols)
            MARS_REFUSE("hill_window[%d] = rows %d:%d, columns %d:%d is not inside the %d x %d field", i, w[0], w[1], w[2], w[3], d->rows, d->cols);
        if (a0 < 0 || b0 < 0 || a0 + (r1 - r0) > d->g_len || b0 + (c1 - c0) > d->g_len)
            MARS_REFUSE("hill_window[%d] reads g from %d and %d: outside its %d entries", i, w[4], w[5], d->g_len);
        if (!std::isfinite(d->hill_amp[i])) MARS_REFUSE("hill_amp[%d] is not finite", i);
    }
    for (int32_t s = 0; s < d->n_stamps; ++s) {
        if (!d->stamp_kept[s]) continue;
        const int32_t k = d->stamp_class[s];
        if (k < 0 || k >= d->n_classes) MARS_REFUSE("stamp_class[%d] = %d is outside 0 .. %d", s, k, d->n_classes - 1);
        const int64_t side = d->class_side[k], r = d->stamp_row[s], c = d->stamp_col[s];
        if (r < 0 || c < 0 || r + side > d->rows || c + side > d->cols)
            MARS_REFUSE("stamp %d (stamp_row = %d, stamp_col = %d, side %d) is not inside the %d x %d field", s, d->stamp_row[s], d->stamp_col[s],
                        (int)side, d->rows, d->cols);
        if (!std::isfinite(d->stamp_factor[s])) MARS_REFUSE("stamp_factor[%d] is not finite", s);
    }
#undef MARS_REFUSE
    return true;
}

static inline uint32_t mars_tiles_of(int32_t n) { return ((uint32_t)n + MARS_TILE - 1) / MARS_TILE; }

// the total length of the tile lists of a descriptor that passed mars_desc_ok
static int64_t mars_count_items(const rover_mars_desc& d) {
    int64_t total = 0;
    for (int32_t s = 0; s < d.n_stamps; ++s) {
        if (!d.stamp_kept[s]) continue;
        const int32_t side = d.class_side[d.stamp_class[s]], r = d.stamp_row[s], c = d.stamp_col[s];
        total += (int64_t)((r + side - 1) / MARS_TILE - r / MARS_TILE + 1) * ((c + side - 1) / MARS_TILE - c / MARS_TILE + 1);
    }
    return total;
}

// start [tiles + 1], items [mars_count_items]: the stamps are visited in index order, so every tile's list is ascending
static void mars_fill_lists(const rover_mars_desc& d, int32_t* start, int32_t* items) {
    const uint32_t tiles_c = mars_tiles_of(d.cols);
    const size_t tiles = (size_t)mars_tiles_of(d.rows) * tiles_c;
    std::fill(start, start + tiles + 1, 0);
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int32_t> cursor;
        if (pass == 1) {                                  // counts -> exclusive sum
            int32_t sum = 0;
            for (size_t t = 0; t <= tiles; ++t) { const int32_t n = start[t]; start[t] = sum; sum += n; }
            cursor.assign(start, start + tiles);
        }
        for (int32_t s = 0; s < d.n_stamps; ++s) {
            if (!d.stamp_kept[s]) continue;
            const int32_t side = d.class_side[d.stamp_class[s]], r = d.stamp_row[s], c = d.stamp_col[s];
            for (int32_t ti = r / MARS_TILE; ti <= (r + side - 1) / MARS_TILE; ++ti)
                for (int32_t tj = c / MARS_TILE; tj <= (c + side - 1) / MARS_TILE; ++tj) {
                    const size_t t = (size_t)ti * tiles_c + (size_t)tj;
                    if (pass == 0) ++start[t]; else items[cursor[t]++] = s;
                }
        }
    }
}

int rover_mars_tiles(const rover_mars_desc* d, int32_t* tile_start, int32_t* tile_items, int64_t capacity, int64_t* n_items) {
    std::string why;
    if (!mars_desc_ok(d, &why)) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: %s", why.c_str());
    if (!n_items) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: n_items is NULL");
    const int64_t n = mars_count_items(*d);
    if (n > INT32_MAX) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: the tile lists hold %lld items, more than 2^31 - 1", (long long)n);
    const bool want = tile_start || tile_items;
    if (want && (!tile_start || (!tile_items && n > 0))) return fail(nullptr, ROVER_E_INVALID, "mars_tiles: tile_start and tile_items go together");
    if (capacity < 0 || (want && capacity < n))
        return fail(nullptr, ROVER_E_INVALID, "mars_tiles: capacity %lld < %lld items", (long long)capacity, (long long)n);
    if (want) mars_fill_lists(*d, tile_start, tile_items);
    *n_items = n;
    return ROVER_OK;
}

// The arguments are validated before the ctx is looked at, as for rover_build_heightfield
int rover_mars_heightfield(rover_ctx* c, const rover_mars_desc* d, double* hf, uint8_t* rock_mask, void* stream) {
    std::string why;
    if (!mars_desc_ok(d, &why)) return fail(c, ROVER_E_INVALID, "mars_heightfield: %s", why.c_str());
    if (!hf) return fail(c, ROVER_E_INVALID, "mars_heightfield: hf is NULL");
    const int64_t n_items = mars_count_items(*d);
    if (n_items > INT32_MAX) return fail(c, ROVER_E_INVALID, "mars_heightfield: the tile lists hold %lld items, more than 2^31 - 1", (long long)n_items);
    if (!c) return fail(nullptr, ROVER_E_INVALID, "mars_heightfield: null ctx");
    USE_DEVICE(c);
#define MARS_TRY(expr)                                                                                        \
    do {                                                                                                      \
        hipError_t e__ = (expr);                                                                              \
        if (e__ != hipSuccess) return fail(c, ROVER_E_HIP, "mars_heightfield: %s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)
    // host tables in the kernel's records
    const uint32_t tiles_r = mars_tiles_of(d->rows), tiles_c = mars_tiles_of(d->cols);
    const size_t tiles = (size_t)tiles_r * tiles_c;
    std::vector<MarsHill> hills((size_t)d->n_hills);
    for (int32_t i = 0; i < d->n_hills; ++i) {
        const int32_t* w = d->hill_window + 6 * (size_t)i;
        hills[i] = MarsHill{w[0], w[1], w[2], w[3], w[4], w[5], d->hill_amp[i]};
    }
    uint32_t table_at[ROVER_MARS_MAX_CLASSES + 1] = {0};
    for (int32_t k = 0; k < d->n_classes; ++k) table_at[k + 1] = table_at[k] + (uint32_t)(d->class_side[k] * d->class_side[k]);
    const size_t table_doubles = table_at[d->n_classes];
    std::vector<MarsStamp> stamps((size_t)d->n_stamps, MarsStamp{0, 0, 0u, 0u, 0.0, 0.0});
    for (int32_t s = 0; s < d->n_stamps; ++s)
        if (d->stamp_kept[s]) {
            const int32_t k = d->stamp_class[s];
            stamps[s] = MarsStamp{d->stamp_row[s], d->stamp_col[s], (uint32_t)d->class_side[k], table_at[k], d->stamp_factor[s], 0.0};
        }
    std::vector<int32_t> start(tiles + 1), items((size_t)n_items);
    mars_fill_lists(*d, start.data(), items.data());
    DevBuf<MarsHill> d_hills;
    DevBuf<MarsStamp> d_stamps;
    DevBuf<double> d_g, d_tables;
    DevBuf<int32_t> d_start, d_items;
    MARS_TRY(d_hills.alloc(std::max<size_t>(hills.size(), 1)));
    MARS_TRY(d_stamps.alloc(std::max<size_t>(stamps.size(), 1)));
    MARS_TRY(d_g.alloc((size_t)d->g_len));
    MARS_TRY(d_tables.alloc(std::max<size_t>(table_doubles, 1)));
    MARS_TRY(d_start.alloc(start.size()));
    MARS_TRY(d_items.alloc(std::max<size_t>(items.size(), 1)));
    if (!hills.empty()) MARS_TRY(hipMemcpy(d_hills.get(), hills.data(), hills.size() * sizeof(MarsHill), hipMemcpyHostToDevice));
    if (!stamps.empty()) MARS_TRY(hipMemcpy(d_stamps.get(), stamps.data(), stamps.size() * sizeof(MarsStamp), hipMemcpyHostToDevice));
    MARS_TRY(hipMemcpy(d_g.get(), d->g, (size_t)d->g_len * sizeof(double), hipMemcpyHostToDevice));
    if (table_doubles) MARS_TRY(hipMemcpy(d_tables.get(), d->class_tables, table_doubles * sizeof(double), hipMemcpyHostToDevice));
    MARS_TRY(hipMemcpy(d_start.get(), start.data(), start.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!items.empty()) MARS_TRY(hipMemcpy(d_items.get(), items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MarsArgs a{};
    a.hf = hf; a.mask = rock_mask; a.rows = d->rows; a.cols = d->cols; a.tiles_r = tiles_r; a.tiles_c = tiles_c;
    a.hills = d_hills.get(); a.n_hills = d->n_hills; a.g = d_g.get(); a.tables = d_tables.get(); a.stamps = d_stamps.get();
    a.tile_start = d_start.get(); a.tile_items = d_items.get();
    MARS_TRY(launch_mars_heightfield(a, (hipStream_t)stream));
    MARS_TRY(hipStreamSynchronize((hipStream_t)stream));          // the tables above are freed on return
#undef MARS_TRY
    return ROVER_OK;
}

// the f32 and the bf16 layer differ in the launch alone (launch_linear_act: rover_mlp.hip; launch_linear_bf16: rover_bf16_tile.hip)
static int linear_forward_run(rover_ctx* c, const char* what, hipError_t (*launch)(const LinearArgs&, hipStream_t), const float* x, int64_t x_stride,
                              int32_t M, int32_t K, const float* weight, const float* bias, int32_t N, int32_t activation, float* y, int64_t y_stride,
                              void* stream) {
    if (!c) return ROVER_E_INVALID;
    // K = 0: a layer over an empty obs slice (model.py builds Encoder(0, ...) when a heightmap part is absent) = act(bias)
    if ((K > 0 && (!x || !weight)) || !y || M < 0 || K < 0 || N <= 0 || N > 256 || x_stride < K || y_stride < N || activation < 0 || activation > 4)
        return fail(c, ROVER_E_INVALID, "%s: bad arguments (M=%d K=%d N=%d act=%d)", what, M, K, N, activation);
    if (M == 0) return ROVER_OK;
    USE_DEVICE(c);
    LinearArgs a{x, x_stride, weight, bias, y, y_stride, M, K, N, activation};
    HIP_TRY(c, launch(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_linear_forward(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K, const float* weight, const float* bias,
                         int32_t N, int32_t activation, float* y, int64_t y_stride, void* stream) {
    return linear_forward_run(c, "linear_forward", launch_linear_act, x, x_stride, M, K, weight, bias, N, activation, y, y_stride, stream);
}

int rover_linear_forward_bf16(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K, const float* weight, const float* bias,
                              int32_t N, int32_t activation, float* y, int64_t y_stride, void* stream) {
    return linear_forward_run(c, "linear_forward_bf16", launch_linear_bf16, x, x_stride, M, K, weight, bias, N, activation, y, y_stride, stream);
}

// One chain, validated in one place.  The shape half: M, K0, the depth, every width and activation — all chain_route() reads, so all a route query looks at (no pointer of
// the descriptor but widths / activations).  0 = fine, -1 = M / K0 / the depth / a null array, i + 1 = layer i's width or activation.
// min_k0: 1 for the f32 chains; 0 for the bf16 ones, which also run a chain over an EMPTY obs slice (model.py builds Encoder(0, ...) when
// a heightmap part is absent: its first layer is act(bias), as rover_linear_forward computes it for K = 0) — x is then not read.
static int chain_shape_of(const rover_chain_desc& d, int32_t M, ChainArgs* a, int32_t min_k0 = 1) {
    if (!d.widths || !d.activations || M < 0 || d.K0 < min_k0 || (d.n_layers != 2 && d.n_layers != 4)) return -1;
    *a = ChainArgs{};
    a->M = M; a->K0 = d.K0; a->n_layers = d.n_layers;
    for (int i = 0; i < d.n_layers; ++i) {
        if (d.widths[i] <= 0 || d.widths[i] > 256 || d.activations[i] < 0 || d.activations[i] > 4) return i + 1;
        a->n[i] = d.widths[i]; a->act[i] = d.activations[i];
    }
    return 0;
}
// The whole of it, for a call that launches: the shapes, then the pointers and the row strides (0 = ok, else the error is recorded
// under `what`, the entry point that was called)
static int chain_args_of(rover_ctx* c, const rover_chain_desc& d, int32_t M, const char* what, ChainArgs* out, int32_t min_k0 = 1) {
    ChainArgs a;
    const int bad = chain_shape_of(d, M, &a, min_k0);
    if (bad < 0 || (!d.x && d.K0 > 0) || !d.y || !d.weights || !d.biases || d.x_stride < d.K0)
        return fail(c, ROVER_E_INVALID, "%s: bad arguments (M=%d K0=%d layers=%d)", what, M, d.K0, d.n_layers);
    for (int i = 0; i < d.n_layers; ++i) {
        if ((!d.weights[i] && (i > 0 || d.K0 > 0)) || bad == i + 1)
            return fail(c, ROVER_E_INVALID, "%s: layer %d: width %d activation %d", what, i, d.widths[i], d.activations[i]);
        a.w[i] = d.weights[i]; a.b[i] = d.biases[i];
    }
    if (d.y_stride < a.n[d.n_layers - 1]) return fail(c, ROVER_E_INVALID, "%s: y_stride %lld < width %d", what, (long long)d.y_stride, a.n[d.n_layers - 1]);
    a.x = d.x; a.x_stride = d.x_stride; a.y = d.y; a.y_stride = d.y_stride;
    *out = a;
    return ROVER_OK;
}

// the split-k scratch buffer, grown when a larger batch comes (not inside a stream capture — size the first call before capturing)
static int mlp_scratch_reserve(rover_ctx* c, size_t need, hipStream_t s) {
    if (need * sizeof(float) <= c->d_mlp_scratch.bytes()) return ROVER_OK;
    HIP_TRY(c, hipStreamSynchronize(s));          // kernels still reading the old buffer
    HIP_TRY(c, c->d_mlp_scratch.alloc(need));
    return ROVER_OK;
}

static int chain_refused(rover_ctx* c, const char* what) {
    return fail(c, ROVER_E_INVALID, "%s: net outside the built tile shapes (<= 96 -> <= 64, or <= 256 -> <= 160 -> <= 128 -> <= 16 with hidden activations none / LeakyReLU / ReLU)", what);
}

// launches what chain_route() chose (never ChainKernel::None)
static int chain_run(rover_ctx* c, const ChainArgs& a, const ChainRoute& r, hipStream_t s) {
    if (r.kernel == ChainKernel::SplitK)
        if (int e = mlp_scratch_reserve(c, chain_splitk_scratch_floats(a.M, a.K0, a.n[0]), s)) return e;
    HIP_TRY(c, launch_chain(a, r, c->d_mlp_scratch.get(), s));
    return ROVER_OK;
}

// the f32 and the bf16 entry points differ in the route function alone (chain_route / chain_route_bf16: rover_mlp.hip)
typedef ChainRoute (*ChainRouteFn)(const ChainArgs&);
static int32_t chain_min_k0(ChainRouteFn route) { return route == chain_route_bf16 ? 0 : 1; }

static int chain_forward(rover_ctx* c, const rover_chain_desc& d, int32_t M, const char* what, ChainRouteFn route, void* stream) {
    if (!c) return ROVER_E_INVALID;
    ChainArgs a;
    if (int r = chain_args_of(c, d, M, what, &a, chain_min_k0(route))) return r;
    if (M == 0) return ROVER_OK;
    const ChainRoute r = route(a);
    if (r.kernel == ChainKernel::None) return chain_refused(c, what);
    USE_DEVICE(c);
    return chain_run(c, a, r, (hipStream_t)stream);
}

int rover_mlp_chain_forward(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                            const float* const* weights, const float* const* biases, const int32_t* widths, const int32_t* activations,
                            float* y, int64_t y_stride, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_forward(c, d, M, "mlp_chain_forward", chain_route, stream);
}

int rover_mlp_chain_forward_bf16(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers,
                                 const float* const* weights, const float* const* biases, const int32_t* widths, const int32_t* activations,
                                 float* y, int64_t y_stride, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_forward(c, d, M, "mlp_chain_forward_bf16", chain_route_bf16, stream);
}

int rover_bf16_round(const float* in, int64_t n, float* out) {
    if (n < 0 || (n > 0 && (!in || !out))) return fail(nullptr, ROVER_E_INVALID, "bf16_round: bad arguments (n=%lld)", (long long)n);
    for (int64_t i = 0; i < n; ++i) out[i] = (float)bf16_rne(in[i]);
    return ROVER_OK;
}

int rover_mlp_chain_pair_forward(rover_ctx* c, int32_t M, const rover_chain_desc* da, const rover_chain_desc* db, const float* copy_src,
                                 int64_t copy_src_stride, float* copy_dst, int64_t copy_dst_stride, int32_t copy_cols, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!da || !db || copy_cols < 0 || (copy_cols > 0 && (!copy_src || !copy_dst || copy_src_stride < copy_cols || copy_dst_stride < copy_cols)))
        return fail(c, ROVER_E_INVALID, "mlp_chain_pair_forward: bad arguments (copy_cols=%d)", copy_cols);
    ChainArgs a, b;
    if (int r = chain_args_of(c, *da, M, "mlp_chain_pair_forward", &a)) return r;
    if (int r = chain_args_of(c, *db, M, "mlp_chain_pair_forward", &b)) return r;
    if (M == 0) return ROVER_OK;
    const ChainRoute ra = chain_route(a), rb = chain_route(b);
    if (ra.kernel == ChainKernel::None || rb.kernel == ChainKernel::None) return chain_refused(c, "mlp_chain_pair_forward");
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (chain_pair_side_by_side(ra, rb)) {
        const size_t fa = chain_splitk_scratch_floats(a.M, a.K0, a.n[0]), fb = chain_splitk_scratch_floats(b.M, b.K0, b.n[0]);
        if (int r = mlp_scratch_reserve(c, fa + fb, s)) return r;
        HIP_TRY(c, launch_chain_splitk_pair(a, b, ra, c->d_mlp_scratch.get(), c->d_mlp_scratch.get() + fa, copy_src, copy_src_stride, copy_dst,
                                            copy_dst_stride, copy_cols, s));
        return ROVER_OK;
    }
    if (copy_cols > 0)
        HIP_TRY(c, hipMemcpy2DAsync(copy_dst, (size_t)copy_dst_stride * sizeof(float), copy_src, (size_t)copy_src_stride * sizeof(float),
                                    (size_t)copy_cols * sizeof(float), (size_t)M, hipMemcpyDeviceToDevice, s));
    if (int r = chain_run(c, a, ra, s)) return r;
    return chain_run(c, b, rb, s);
}

// ---- route queries: what the forward calls above would launch, from the shapes alone (host only) ----
const char* rover_linear_route(int32_t M, int32_t K, int32_t N) {
    const LinearRoute r = linear_route(M, N);
    if (K < 0 || !r.nw) return nullptr;
    return M == 0 ? "none" : linear_route_name(r);
}

const char* rover_linear_route_bf16(int32_t M, int32_t K, int32_t N) {
    const char* name = linear_route_bf16_name(M, N);
    if (K < 0 || !name) return nullptr;
    return M == 0 ? "none" : name;
}

static const char* chain_route_query(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations, ChainRouteFn route) {
    const rover_chain_desc d{nullptr, 0, K0, n_layers, nullptr, nullptr, widths, activations, nullptr, 0};      // a route query: shapes alone
    ChainArgs a;
    if (chain_shape_of(d, M, &a, chain_min_k0(route))) return nullptr;
    return M == 0 ? "none" : chain_route_name(route(a));
}
const char* rover_mlp_chain_route(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations) {
    return chain_route_query(M, K0, n_layers, widths, activations, chain_route);
}
const char* rover_mlp_chain_route_bf16(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations) {
    return chain_route_query(M, K0, n_layers, widths, activations, chain_route_bf16);
}

const char* rover_mlp_chain_pair_route(int32_t M, const rover_chain_desc* da, const rover_chain_desc* db) {
    ChainArgs a, b;
    if (!da || !db || chain_shape_of(*da, M, &a) || chain_shape_of(*db, M, &b)) return nullptr;
    if (M == 0) return "none";
    const ChainRoute ra = chain_route(a), rb = chain_route(b);
    if (ra.kernel == ChainKernel::None || rb.kernel == ChainKernel::None) return nullptr;
    static thread_local char name[96];
    char na[48];                                                     // (chain_route_name() may hand out one buffer twice)
    snprintf(na, sizeof na, "%s", chain_route_name(ra));
    if (chain_pair_side_by_side(ra, rb)) snprintf(name, sizeof name, "pair(%s)", na);
    else snprintf(name, sizeof name, "seq(%s;%s)", na, chain_route_name(rb));
    return name;
}

// ---- the Gaussian head ----
// the validated descriptor (0 = ok, else the error is recorded with c, or for rover_last_error(NULL) when c is null); no pointer is read
static int gauss_head_of(rover_ctx* c, const rover_gauss_head* g, int32_t M, bool given_mean, GaussHead* out) {
    if (!g) return fail(c, ROVER_E_INVALID, "gauss_head: null descriptor");
    if (g->A < 1 || g->A > GAUSS_MAX_A) return fail(c, ROVER_E_INVALID, "gauss_head: A = %d outside 1 .. %d", g->A, GAUSS_MAX_A);
    if (g->clip_log_std && !(g->min_log_std <= g->max_log_std))
        return fail(c, ROVER_E_INVALID, "gauss_head: min_log_std %g > max_log_std %g", (double)g->min_log_std, (double)g->max_log_std);
    if (g->clip_actions && !(g->low <= g->high)) return fail(c, ROVER_E_INVALID, "gauss_head: low %g > high %g", (double)g->low, (double)g->high);
    if (g->reduction < ROVER_REDUCE_SUM || g->reduction > ROVER_REDUCE_NONE) return fail(c, ROVER_E_INVALID, "gauss_head: unknown reduction %d", g->reduction);
    if (!g->log_std || !g->actions || !g->log_prob) return fail(c, ROVER_E_INVALID, "gauss_head: log_std, actions and log_prob must be given");
    const int lp_cols = g->reduction == ROVER_REDUCE_NONE ? g->A : 1;
    if (g->actions_stride < g->A || g->log_prob_stride < lp_cols || (g->taken_actions && g->taken_stride < g->A))
        return fail(c, ROVER_E_INVALID, "gauss_head: a row stride is shorter than its row (A = %d)", g->A);
    if (given_mean && (!g->mean || g->mean_stride < g->A)) return fail(c, ROVER_E_INVALID, "gauss_head: mean [M, A] must be given");
    if (M < 0 || g->row_offset < 0 || g->row_offset + (int64_t)M > (int64_t)1 << 32)
        return fail(c, ROVER_E_INVALID, "gauss_head: rows %lld .. + %d outside [0, 2^32)", (long long)g->row_offset, M);
    GaussHead h{};
    h.log_std = g->log_std; h.A = g->A; h.clip_log_std = g->clip_log_std != 0; h.clip_actions = g->clip_actions != 0;
    h.reduction = g->reduction; h.deterministic = g->deterministic != 0;
    h.min_log_std = g->min_log_std; h.max_log_std = g->max_log_std; h.low = g->low; h.high = g->high;
    h.seed = g->seed; h.step = g->step; h.step_dev = g->step_dev; h.row_offset = g->row_offset;
    h.taken = g->taken_actions; h.taken_stride = g->taken_stride;
    h.actions = g->actions; h.actions_stride = g->actions_stride; h.log_prob = g->log_prob; h.log_prob_stride = g->log_prob_stride;
    *out = h;
    return ROVER_OK;
}

static int chain_act(rover_ctx* c, const rover_chain_desc& d, int32_t M, const rover_gauss_head* head, const char* what, ChainRouteFn route,
                     void* stream) {
    if (!c) return ROVER_E_INVALID;
    ChainArgs a; GaussHead h{};
    if (int r = chain_args_of(c, d, M, what, &a, chain_min_k0(route))) return r;
    if (int r = gauss_head_of(c, head, M, false, &h)) return r;
    if (a.n[d.n_layers - 1] != h.A) return fail(c, ROVER_E_INVALID, "%s: the last layer is %d wide, the head has A = %d", what, a.n[d.n_layers - 1], h.A);
    if (M == 0) return ROVER_OK;
    const ChainRoute r = route(a);
    if (r.kernel == ChainKernel::None) return chain_refused(c, what);
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    if (chain_head_fused(r, h.A)) {
        HIP_TRY(c, launch_chain_head(a, r, h, s));
        return ROVER_OK;
    }
    if (int e = chain_run(c, a, r, s)) return e;
    HIP_TRY(c, launch_gaussian_head(a.y, a.y_stride, M, h, s));
    return ROVER_OK;
}

int rover_mlp_chain_act(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers, const float* const* weights,
                        const float* const* biases, const int32_t* widths, const int32_t* activations, float* y, int64_t y_stride,
                        const rover_gauss_head* head, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_act(c, d, M, head, "mlp_chain_act", chain_route, stream);
}

int rover_mlp_chain_act_bf16(rover_ctx* c, const float* x, int64_t x_stride, int32_t M, int32_t K0, int32_t n_layers, const float* const* weights,
                             const float* const* biases, const int32_t* widths, const int32_t* activations, float* y, int64_t y_stride,
                             const rover_gauss_head* head, void* stream) {
    const rover_chain_desc d{x, x_stride, K0, n_layers, weights, biases, widths, activations, y, y_stride};
    return chain_act(c, d, M, head, "mlp_chain_act_bf16", chain_route_bf16, stream);
}

int rover_gaussian_head(rover_ctx* c, int32_t M, const rover_gauss_head* head, void* stream) {
    if (!c) return ROVER_E_INVALID;
    GaussHead h{};
    if (int r = gauss_head_of(c, head, M, true, &h)) return r;
    if (M == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_gaussian_head(head->mean, head->mean_stride, M, h, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_policy_noise(rover_ctx* c, uint64_t seed, uint64_t step, const uint64_t* step_dev, int64_t row_offset, int32_t M, int32_t A, float* eps,
                       int64_t eps_stride, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (!eps || M < 0 || A < 1 || A > GAUSS_MAX_A || eps_stride < A || row_offset < 0 || row_offset + (int64_t)M > (int64_t)1 << 32)
        return fail(c, ROVER_E_INVALID, "policy_noise: bad arguments (M=%d A=%d row_offset=%lld)", M, A, (long long)row_offset);
    if (M == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_policy_noise(seed, step, step_dev, row_offset, M, A, eps, eps_stride, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_philox4x32(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
    if (!counter || !key || !out) return fail(nullptr, ROVER_E_INVALID, "philox4x32: null argument");
    uint32_t w[4] = {counter[0], counter[1], counter[2], counter[3]};
    philox4x32_10(w, key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = w[i];
    return ROVER_OK;
}

static const char* chain_act_route_query(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations,
                                         const rover_gauss_head* head, ChainRouteFn route) {
    const rover_chain_desc d{nullptr, 0, K0, n_layers, nullptr, nullptr, widths, activations, nullptr, 0};
    ChainArgs a; GaussHead h{};
    if (chain_shape_of(d, M, &a, chain_min_k0(route))) {
        fail(nullptr, ROVER_E_INVALID, "mlp_chain_act_route: bad shapes (M=%d K0=%d layers=%d)", M, K0, n_layers);
        return nullptr;
    }
    if (gauss_head_of(nullptr, head, M, false, &h)) return nullptr;
    if (a.n[n_layers - 1] != h.A) {
        fail(nullptr, ROVER_E_INVALID, "mlp_chain_act_route: the last layer is %d wide, the head has A = %d", a.n[n_layers - 1], h.A);
        return nullptr;
    }
    if (M == 0) return "none";
    const char* name = chain_act_route_name(route(a), h.A);
    if (!name) fail(nullptr, ROVER_E_INVALID, "mlp_chain_act_route: net outside the built tile shapes");
    return name;
}
const char* rover_mlp_chain_act_route(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations,
                                      const rover_gauss_head* head) {
    return chain_act_route_query(M, K0, n_layers, widths, activations, head, chain_route);
}
const char* rover_mlp_chain_act_route_bf16(int32_t M, int32_t K0, int32_t n_layers, const int32_t* widths, const int32_t* activations,
                                           const rover_gauss_head* head) {
    return chain_act_route_query(M, K0, n_layers, widths, activations, head, chain_route_bf16);
}

// ---- the learning entry points ----
// Each lists its arrays as an operand table (rover_operands.h), which applies the operand rules of rover_step.h; the ctx is looked at last
// (`need_ctx`: here), so every refusal is reached with a NULL ctx too and reports through rover_last_error(NULL).
static int check_operands(rover_ctx* c, Operands& ops, bool need_ctx = true) {
    char why[512];
    if (ops.refused(why, sizeof why)) return fail(c, ROVER_E_INVALID, "%s", why);
    return need_ctx && !c ? fail(nullptr, ROVER_E_INVALID, "%s: null ctx", ops.entry()) : ROVER_OK;
}

// ---- rollout: GAE ----
int rover_gae(rover_ctx* c, const rover_gae_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "gae: null descriptor");
    if (d->T < 1 || d->T > 4096 || d->E < 0 || (int64_t)d->T * d->E >= (int64_t)1 << 31)
        return fail(c, ROVER_E_INVALID, "gae: T = %d outside 1 .. 4096, E = %d < 0, or T E >= 2^31", d->T, d->E);
    if (d->normalize < ROVER_GAE_RAW || d->normalize > ROVER_GAE_NORMALIZE_GIVEN) return fail(c, ROVER_E_INVALID, "gae: unknown normalize %d", d->normalize);
    if (d->E == 0) return ROVER_OK;            // nothing to read or write: no pointer is required
    const int32_t T = d->T, E = d->E;
    if (d->normalize == ROVER_GAE_NORMALIZE && (int64_t)T * E < 2)
        return fail(c, ROVER_E_INVALID, "gae: ROVER_GAE_NORMALIZE needs T E >= 2 (the unbiased std of one element is NaN)");
    Operands ops("gae");
    ops.read("rewards", d->rewards, d->rewards_stride, T, E, 4).read("values", d->values, d->values_stride, T, E, 4)
        .read("dones", d->dones, d->dones_stride, T, E, 1).read("last_values", d->last_values, E, 1, E, 4)
        .written("returns", d->returns, d->returns_stride, T, E, 4).written("advantages", d->advantages, d->advantages_stride, T, E, 4)
        .written("stats_out", d->stats_out, 3, 1, 3, 8, OP_OPTIONAL)
        .same_array("returns", "values");
    if (d->normalize == ROVER_GAE_NORMALIZE_GIVEN) ops.state("stats_in", d->stats_in, 3, 1, 3, 8);     // only read, but clear of every array
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GaeArgs a{};
    a.T = d->T; a.E = (uint32_t)d->E; a.gamma = d->gamma; a.lam = d->lam;
    a.rewards = d->rewards; a.rewards_stride = d->rewards_stride; a.values = d->values; a.values_stride = d->values_stride;
    a.dones = d->dones; a.dones_stride = d->dones_stride; a.last_values = d->last_values;
    a.returns = d->returns; a.returns_stride = d->returns_stride; a.advantages = d->advantages; a.advantages_stride = d->advantages_stride;
    a.normalize = d->normalize; a.stats_out = d->stats_out; a.stats_in = d->normalize == ROVER_GAE_NORMALIZE_GIVEN ? d->stats_in : nullptr;
    a.partials = c->d_gae_partials.get();
    HIP_TRY(c, launch_gae(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_combine_moments(const double* a, const double* b, double* out) {
    if (!a || !b || !out) return fail(nullptr, ROVER_E_INVALID, "combine_moments: null argument");
    gae_combine_moments(a, b, out);
    return ROVER_OK;
}

// ---- training: the backward of one Layer, the PPO loss ----
int rover_linear_backward(rover_ctx* c, const float* x, int64_t x_stride, const float* y, int64_t y_stride, const float* dy, int64_t dy_stride,
                          int32_t M, int32_t K, const float* weight, int32_t N, int32_t activation, float* dx, int64_t dx_stride, float* dweight,
                          float* dbias, void* stream) {
    const LinearBwdRoute r = linear_backward_route(M, K, N, dx != nullptr);
    if (!r.ok || activation < 0 || activation > 4)
        return fail(c, ROVER_E_INVALID, "linear_backward: M=%d K=%d N=%d act=%d outside M >= 0, K >= 0 (<= 256 with dx), 1 <= N <= 256, act 0 .. 4", M, K, N, activation);
    const bool need_x = dweight && K > 0, need_w = dx && K > 0;
    Operands ops("linear_backward");        // M = 0: the [M, .] operands have no element and need no pointer, their strides are checked all the same
    ops.read("dy", dy, dy_stride, M, N, 4);
    if (activation) ops.read("y", y, y_stride, M, N, 4);
    if (need_x) ops.read("x", x, x_stride, M, K, 4);
    if (need_w) ops.read("weight", weight, K, M > 0 ? N : 0, K, 4).written("dx", dx, dx_stride, M, K, 4);
    if (need_x) ops.written("dweight", dweight, K, M > 0 ? N : 0, K, 4);
    ops.written("dbias", dbias, N, M > 0 ? 1 : 0, N, 4, OP_OPTIONAL);     // (M = 0 only zeroes dweight / dbias: they were never checked there)
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    LinearBwdArgs a{x, x_stride, y, y_stride, dy, dy_stride, weight, dx, dx_stride, dweight, dbias, M, K, N, activation};
    if (M > 0 && (dweight || dbias))
        if (int e = mlp_scratch_reserve(c, linear_backward_scratch_floats(r, K, N), s)) return e;
    HIP_TRY(c, launch_linear_backward(a, r, c->d_mlp_scratch.get(), s));
    return ROVER_OK;
}

const char* rover_linear_backward_route(int32_t M, int32_t K, int32_t N, int32_t want_dx) {
    const LinearBwdRoute r = linear_backward_route(M, K, N, want_dx != 0);
    if (!r.ok) return nullptr;
    return M == 0 ? "zero" : linear_backward_route_name(r);
}

int rover_linear_dgrad(rover_ctx* c, const float* y, int64_t y_stride, const float* dy, int64_t dy_stride, int32_t M, int32_t K, const float* weight,
                       int32_t N, int32_t activation, float* dx, int64_t dx_stride, void* stream) {
    const LinearRoute r = linear_dgrad_route(M, N, K);
    if (!r.nw || activation < 0 || activation > 4)
        return fail(c, ROVER_E_INVALID, "linear_dgrad: M=%d K=%d N=%d act=%d outside M >= 0, 1 <= K <= %d, N >= 1, act 0 .. 4", M, K, N, activation, 32 * 65535);
    if (M == 0) return ROVER_OK;
    Operands ops("linear_dgrad");
    ops.read("dy", dy, dy_stride, M, N, 4);
    if (activation) ops.read("y", y, y_stride, M, N, 4);
    ops.read("weight", weight, K, N, K, 4).written("dx", dx, dx_stride, M, K, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    LinearBwdArgs a{nullptr, 0, y, y_stride, dy, dy_stride, weight, dx, dx_stride, nullptr, nullptr, M, K, N, activation};
    HIP_TRY(c, launch_linear_dgrad(a, r, (hipStream_t)stream));
    return ROVER_OK;
}

const char* rover_linear_dgrad_route(int32_t M, int32_t K, int32_t N) {
    const LinearRoute r = linear_dgrad_route(M, N, K);
    if (!r.nw) return nullptr;
    return M == 0 ? "none" : linear_dgrad_route_name(r);
}

int rover_ppo_loss(rover_ctx* c, const rover_ppo_loss_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "ppo_loss: null descriptor");
    if (d->M < 0 || d->A < 1 || d->A > GAUSS_MAX_A) return fail(c, ROVER_E_INVALID, "ppo_loss: M = %d < 0 or A = %d outside 1 .. %d", d->M, d->A, GAUSS_MAX_A);
    if (d->reduction != ROVER_REDUCE_SUM) return fail(c, ROVER_E_INVALID, "ppo_loss: the log-prob reduction must be ROVER_REDUCE_SUM (got %d)", d->reduction);
    if (d->clip_log_std && !(d->min_log_std <= d->max_log_std))
        return fail(c, ROVER_E_INVALID, "ppo_loss: min_log_std %g > max_log_std %g", (double)d->min_log_std, (double)d->max_log_std);
    if (!(d->ratio_clip >= 0.0f) || (d->clip_predicted_values && !(d->value_clip >= 0.0f)))
        return fail(c, ROVER_E_INVALID, "ppo_loss: ratio_clip %g and value_clip %g must be >= 0", (double)d->ratio_clip, (double)d->value_clip);
    if (d->M == 0) return ROVER_OK;            // nothing to read or write: no pointer is required
    const int32_t M = d->M, A = d->A;
    Operands ops("ppo_loss");
    ops.read("mean", d->mean, d->mean_stride, M, A, 4).read("log_std", d->log_std, A, 1, A, 4).read("actions", d->actions, d->actions_stride, M, A, 4)
        .read("old_log_prob", d->old_log_prob, M, 1, M, 4).read("advantages", d->advantages, M, 1, M, 4).read("value", d->value, M, 1, M, 4)
        .read("old_values", d->old_values, M, 1, M, 4).read("returns", d->returns, M, 1, M, 4)
        .written("d_mean", d->d_mean, d->d_mean_stride, M, A, 4).written("d_value", d->d_value, M, 1, M, 4)
        .written("d_log_std", d->d_log_std, A, 1, A, 4).written("stats", d->stats, 4, 1, 4, 8);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    PpoArgs a{};
    a.M = M; a.A = A; a.mean = d->mean; a.mean_stride = d->mean_stride; a.log_std = d->log_std; a.actions = d->actions; a.actions_stride = d->actions_stride;
    a.old_log_prob = d->old_log_prob; a.advantages = d->advantages; a.value = d->value; a.old_values = d->old_values; a.returns = d->returns;
    a.clip_log_std = d->clip_log_std != 0; a.min_log_std = d->min_log_std; a.max_log_std = d->max_log_std;
    a.ratio_clip = d->ratio_clip; a.value_clip = d->value_clip; a.clip_predicted_values = d->clip_predicted_values != 0;
    a.entropy_loss_scale = d->entropy_loss_scale; a.value_loss_scale = d->value_loss_scale;
    a.d_mean = d->d_mean; a.d_mean_stride = d->d_mean_stride; a.d_value = d->d_value; a.d_log_std = d->d_log_std; a.stats = d->stats;
    a.partials = c->d_ppo_partials.get();
    HIP_TRY(c, launch_ppo_loss(a, (hipStream_t)stream));
    return ROVER_OK;
}

// ---- training: gradient-norm clip + Adam ----
// shared by rover_optim_plan and rover_optim_create: NULL when the sizes are acceptable, else what is wrong; *total = sum(numel)
static const char* optim_sizes_refused(int32_t n_tensors, const int64_t* numel, int64_t* total) {
    if (!numel) return "numel is NULL";
    if (n_tensors < 1 || n_tensors > 256) return "n_tensors outside 1 .. 256";
    int64_t sum = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0) return "a negative numel";
        if (numel[i] >= (int64_t)1 << 31 || (sum += numel[i]) >= (int64_t)1 << 31) return "total elements >= 2^31";
    }
    *total = sum;
    return nullptr;
}

int rover_optim_plan(int32_t n_tensors, const int64_t* numel, rover_optim_chunk* chunks, int64_t capacity, int64_t* n_chunks) {
    int64_t total = 0;
    if (const char* why = optim_sizes_refused(n_tensors, numel, &total)) return fail(nullptr, ROVER_E_INVALID, "optim_plan: %s", why);
    if (!n_chunks) return fail(nullptr, ROVER_E_INVALID, "optim_plan: n_chunks is NULL");
    const int64_t n = optim_plan(n_tensors, numel, nullptr, 0);
    if (capacity < 0 || (chunks && capacity < n)) return fail(nullptr, ROVER_E_INVALID, "optim_plan: capacity %lld < %lld chunks", (long long)capacity, (long long)n);
    static_assert(sizeof(rover_optim_chunk) == sizeof(OptimChunkHost), "rover_optim_chunk is OptimChunkHost");
    if (chunks) (void)optim_plan(n_tensors, numel, reinterpret_cast<OptimChunkHost*>(chunks), capacity);
    *n_chunks = n;
    return ROVER_OK;
}

int rover_optim_create(rover_ctx* c, const rover_optim_desc* d, int32_t* handle) {
    if (!d || !handle || !d->params || !d->grads) return fail(c, ROVER_E_INVALID, "optim_create: null descriptor, handle, params or grads");
    int64_t total = 0;
    if (const char* why = optim_sizes_refused(d->n_tensors, d->numel, &total)) return fail(c, ROVER_E_INVALID, "optim_create: %s", why);
    Operands st("optim_create");        // the state by the operand rules (total = 0: the moments have no element); the tensor lists by the loops below
    st.state("step", d->step, 1, 1, 1, 8, 0, 8).state("stopped", d->stopped, 1, 1, 1, 4, 0, 4)
        .state("exp_avg", d->exp_avg, total, 1, total, 4, 0, 4).state("exp_avg_sq", d->exp_avg_sq, total, 1, total, 4, 0, 4);
    if (int e = check_operands(c, st, false)) return e;
    const int32_t n = d->n_tensors;
    std::vector<Span> ps, gs, state = {st.span(0), st.span(1)};         // the tensors with elements; the state with elements
    if (total > 0) state.insert(state.end(), {st.span(2), st.span(3)});
    for (int32_t i = 0; i < n; ++i) {
        if (d->numel[i] == 0) continue;
        if (!d->params[i] || !d->grads[i] || (uintptr_t)d->params[i] % 4 || (uintptr_t)d->grads[i] % 4)
            return fail(c, ROVER_E_INVALID, "optim_create: params[%d] or grads[%d] is NULL or misaligned", i, i);
        Span p, g;
        if (!span_of(d->params[i], d->numel[i], 1, d->numel[i], 4, &p) || !span_of(d->grads[i], d->numel[i], 1, d->numel[i], 4, &g))
            return fail(c, ROVER_E_INVALID, "optim_create: params[%d] or grads[%d]: extent too large", i, i);
        ps.push_back(p);
        gs.push_back(g);
    }
    for (size_t i = 0; i < ps.size(); ++i) {
        for (const Span& s : state)
            if (overlap(ps[i], s) || overlap(gs[i], s)) return fail(c, ROVER_E_INVALID, "optim_create: a parameter or a gradient overlaps the state");
        for (size_t j = 0; j < ps.size(); ++j)
            if (overlap(ps[i], gs[j]) || (j > i && overlap(ps[i], ps[j])))
                return fail(c, ROVER_E_INVALID, "optim_create: a parameter overlaps a gradient or another parameter");
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "optim_create: null ctx");       // the ctx is only where the handle is kept
    USE_DEVICE(c);
    const int64_t n_chunks = optim_plan(n, d->numel, nullptr, 0);
    std::vector<OptimChunkHost> plan((size_t)n_chunks);
    (void)optim_plan(n, d->numel, plan.data(), n_chunks);
    std::vector<int64_t> offset((size_t)n, 0);                 // of tensor i in the flat state
    for (int32_t i = 1; i < n; ++i) offset[i] = offset[i - 1] + d->numel[i - 1];
    const bool state_al = ((uintptr_t)d->exp_avg | (uintptr_t)d->exp_avg_sq) % 16 == 0;
    std::vector<OptimChunk> table((size_t)n_chunks);
    for (int64_t k = 0; k < n_chunks; ++k) {
        const OptimChunkHost& h = plan[(size_t)k];
        OptimChunk& o = table[(size_t)k];
        o.p = d->params[h.tensor] + h.first;
        o.g = d->grads[h.tensor] + h.first;
        o.state = (uint32_t)(offset[h.tensor] + h.first);
        o.len = (uint32_t)h.length;
        o.flags = (((uintptr_t)d->params[h.tensor] | (uintptr_t)d->grads[h.tensor]) % 16 == 0 ? OPTIM_PG_ALIGNED : 0) |
                  (state_al && offset[h.tensor] % 4 == 0 ? OPTIM_STATE_ALIGNED : 0);
        o.pad = 0;
    }
    OptimHandle h;
    hipError_t e = h.record.alloc(1);
    if (e == hipSuccess && n_chunks > 0) e = h.chunks.alloc((size_t)n_chunks);
    if (e == hipSuccess && n_chunks > 0) e = h.partials.alloc((size_t)n_chunks);
    if (e == hipSuccess && n_chunks > 0) e = hipMemcpy(h.chunks.get(), table.data(), table.size() * sizeof(OptimChunk), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h.record.get(), 0, sizeof(OptimRecord));
    if (e != hipSuccess) return fail(c, ROVER_E_HIP, "optim_create: %s", hipGetErrorString(e));
    h.live = true;
    h.n_chunks = (uint32_t)n_chunks;
    h.exp_avg = d->exp_avg; h.exp_avg_sq = d->exp_avg_sq; h.step = d->step; h.stopped = d->stopped;
    h.spans = state;
    h.spans.insert(h.spans.end(), ps.begin(), ps.end());
    h.spans.insert(h.spans.end(), gs.begin(), gs.end());
    size_t slot = 0;
    while (slot < c->optims.size() && c->optims[slot].live) ++slot;
    if (slot == c->optims.size()) c->optims.emplace_back();
    c->optims[slot] = std::move(h);
    *handle = (int32_t)slot;
    return ROVER_OK;
}

static OptimHandle* optim_handle(rover_ctx* c, int32_t handle) {
    return handle >= 0 && (size_t)handle < c->optims.size() && c->optims[(size_t)handle].live ? &c->optims[(size_t)handle] : nullptr;
}

int rover_optim_destroy(rover_ctx* c, int32_t handle) {
    if (!c) return ROVER_E_INVALID;
    OptimHandle* h = optim_handle(c, handle);
    if (!h) return fail(c, ROVER_E_INVALID, "optim_destroy: handle %d is not live", handle);
    USE_DEVICE(c);
    *h = OptimHandle{};                 // (the owners free their device memory)
    return ROVER_OK;
}

int rover_optim_step(rover_ctx* c, int32_t handle, const rover_optim_step_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "optim_step: null descriptor");
    if (!(d->lr >= 0.0) || !std::isfinite(d->lr) || !(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0) ||
        !(d->eps >= 0.0) || !std::isfinite(d->eps))
        return fail(c, ROVER_E_INVALID, "optim_step: lr %g and eps %g must be finite and >= 0, beta1 %g and beta2 %g in [0, 1)", d->lr, d->eps, d->beta1, d->beta2);
    if (std::isnan(d->grad_norm_clip) || std::isnan(d->gate_threshold)) return fail(c, ROVER_E_INVALID, "optim_step: grad_norm_clip or gate_threshold is NaN");
    Operands ops("optim_step");
    ops.read("gate", d->gate, 1, 1, 1, 8, OP_OPTIONAL, 8).written("norm_out", d->norm_out, 1, 1, 1, 8, OP_OPTIONAL, 8);
    if (int e = check_operands(c, ops)) return e;
    const OptimHandle* h = optim_handle(c, handle);
    if (!h) return fail(c, ROVER_E_INVALID, "optim_step: handle %d is not live", handle);
    Span out;
    if (d->norm_out && span_of(d->norm_out, 1, 1, 1, 8, &out))
        for (const Span& s : h->spans)
            if (overlap(out, s)) return fail(c, ROVER_E_INVALID, "optim_step: norm_out overlaps a parameter, a gradient or the state");
    USE_DEVICE(c);
    OptimArgs a{};
    a.chunks = h->chunks.get(); a.n_chunks = h->n_chunks; a.partials = h->partials.get(); a.record = h->record.get();
    a.exp_avg = h->exp_avg; a.exp_avg_sq = h->exp_avg_sq; a.step = h->step; a.stopped = h->stopped;
    a.lr = d->lr; a.beta1 = d->beta1; a.beta2 = d->beta2; a.eps = d->eps; a.clip = d->grad_norm_clip;
    a.gate = d->gate; a.gate_threshold = d->gate_threshold; a.norm_out = d->norm_out;
    HIP_TRY(c, launch_optim_step(a, (hipStream_t)stream));
    return ROVER_OK;
}

// ---- the student policy's recurrent block (rover_gru.hip) ----
static int gru_cell_run(rover_ctx* c, const char* what, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K,
                        int32_t H, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                        int64_t h_out_stride, bool train, float* gates, int64_t gates_stride, void* stream,
                        hipError_t (*launch)(const GruArgs&, hipStream_t) = launch_gru_cell) {
    if (!gru_cell_route(M, K, H).nw) return fail(c, ROVER_E_INVALID, "%s: M=%d K=%d H=%d outside M >= 0, K >= 0, 1 <= H <= %d", what, M, K, H, 32 * 65535);
    if (M == 0) return ROVER_OK;                   // nothing is read or written: no pointer is required
    const int64_t G = (int64_t)3 * H;              // gate rows
    Operands ops(what);
    ops.read("h_in", h_in, h_in_stride, M, H, 4);  // (h_out may not even be h_in: a tile of h' needs whole rows of h that other workgroups still read)
    if (K > 0) ops.read("x", x, x_stride, M, K, 4).read("w_ih", w_ih, K, G, K, 4);
    ops.read("w_hh", w_hh, H, G, H, 4).read("b_ih", b_ih, G, 1, G, 4, OP_OPTIONAL).read("b_hh", b_hh, G, 1, G, 4, OP_OPTIONAL)
        .read("reset_mask", reset_mask, M, 1, M, 1, OP_OPTIONAL).written("h_out", h_out, h_out_stride, M, H, 4);
    if (train) ops.written("gates", gates, gates_stride, M, (int64_t)4 * H, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GruArgs a{x, x_stride, h_in, h_in_stride, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, M, K, H, train ? gates : nullptr, gates_stride};
    HIP_TRY(c, launch(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_gru_cell(rover_ctx* c, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K, int32_t H,
                   const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                   int64_t h_out_stride, void* stream) {
    return gru_cell_run(c, "gru_cell", x, x_stride, h_in, h_in_stride, M, K, H, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, false, nullptr, 0, stream);
}

int rover_gru_cell_bf16(rover_ctx* c, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K, int32_t H,
                        const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                        int64_t h_out_stride, void* stream) {
    return gru_cell_run(c, "gru_cell_bf16", x, x_stride, h_in, h_in_stride, M, K, H, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, false, nullptr, 0,
                        stream, launch_gru_cell_bf16);
}

int rover_gru_cell_train(rover_ctx* c, const float* x, int64_t x_stride, const float* h_in, int64_t h_in_stride, int32_t M, int32_t K, int32_t H,
                         const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const uint8_t* reset_mask, float* h_out,
                         int64_t h_out_stride, float* gates, int64_t gates_stride, void* stream) {
    return gru_cell_run(c, "gru_cell_train", x, x_stride, h_in, h_in_stride, M, K, H, w_ih, w_hh, b_ih, b_hh, reset_mask, h_out, h_out_stride, true, gates,
                        gates_stride, stream);
}

int rover_gru_cell_backward(rover_ctx* c, const float* dh_above, int64_t dh_above_stride, const float* dh_next, int64_t dh_next_stride, const float* gates,
                            int64_t gates_stride, const float* h_in, int64_t h_in_stride, const uint8_t* reset_mask, const float* w_hh, int32_t M, int32_t H,
                            float* dgi, int64_t dgi_stride, float* dgh, int64_t dgh_stride, float* dh_in, int64_t dh_in_stride, void* stream) {
    if (!gru_cell_backward_route(M, H).nw) return fail(c, ROVER_E_INVALID, "gru_cell_backward: M=%d H=%d outside M >= 0, 1 <= H <= %d", M, H, 32 * 65535);
    if (M == 0) return ROVER_OK;
    const int64_t G = (int64_t)3 * H;
    Operands ops("gru_cell_backward");
    ops.read("dh_above", dh_above, dh_above_stride, M, H, 4).read("dh_next", dh_next, dh_next_stride, M, H, 4, OP_OPTIONAL)
        .read("gates", gates, gates_stride, M, (int64_t)4 * H, 4).read("h_in", h_in, h_in_stride, M, H, 4)
        .read("reset_mask", reset_mask, M, 1, M, 1, OP_OPTIONAL).read("w_hh", w_hh, H, G, H, 4)
        .written("dgi", dgi, dgi_stride, M, G, 4).written("dgh", dgh, dgh_stride, M, G, 4).written("dh_in", dh_in, dh_in_stride, M, H, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GruBwdArgs a{dh_above, dh_above_stride, dh_next, dh_next_stride, gates, gates_stride, h_in, h_in_stride, reset_mask, w_hh,
                 dgi, dgi_stride, dgh, dgh_stride, dh_in, dh_in_stride, M, H};
    HIP_TRY(c, launch_gru_cell_backward(a, (hipStream_t)stream));
    return ROVER_OK;
}

const char* rover_gru_cell_backward_route(int32_t M, int32_t H) {
    const GruRoute r = gru_cell_backward_route(M, H);
    if (!r.nw) return nullptr;
    return M == 0 ? "none" : gru_cell_backward_route_name(r);
}

const char* rover_gru_cell_route(int32_t M, int32_t K, int32_t H) {
    const GruRoute r = gru_cell_route(M, K, H);
    if (!r.nw) return nullptr;
    return M == 0 ? "none" : gru_cell_route_name(r);
}

const char* rover_gru_cell_route_bf16(int32_t M, int32_t K, int32_t H) {
    const char* name = gru_cell_route_bf16_name(M, K, H);
    if (!name) return nullptr;
    return M == 0 ? "none" : name;
}

int rover_gated_sum(rover_ctx* c, const float* add, int64_t add_stride, const float* mul, int64_t mul_stride, const float* pre, int64_t pre_stride,
                    int32_t M, int32_t N, float* out, int64_t out_stride, void* stream) {
    if (M < 0 || N < 1 || (int64_t)M * N >= (int64_t)1 << 38) return fail(c, ROVER_E_INVALID, "gated_sum: M=%d N=%d outside M >= 0, N >= 1, M N < 2^38", M, N);
    if (M == 0) return ROVER_OK;
    Operands ops("gated_sum");
    ops.read("add", add, add_stride, M, N, 4, OP_STRIDE0).read("mul", mul, mul_stride, M, N, 4, OP_STRIDE0).read("pre", pre, pre_stride, M, N, 4, OP_STRIDE0)
        .written("out", out, out_stride, M, N, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GatedSumArgs a{add, add_stride, mul, mul_stride, pre, pre_stride, out, out_stride, M, N};
    HIP_TRY(c, launch_gated_sum(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_gated_sum_backward(rover_ctx* c, const float* d_out, int64_t d_out_stride, const float* mul, int64_t mul_stride, const float* pre,
                             int64_t pre_stride, int32_t M, int32_t N, float* d_mul, int64_t d_mul_stride, float* d_pre, int64_t d_pre_stride, void* stream) {
    if (M < 0 || N < 1 || (int64_t)M * N >= (int64_t)1 << 38)
        return fail(c, ROVER_E_INVALID, "gated_sum_backward: M=%d N=%d outside M >= 0, N >= 1, M N < 2^38", M, N);
    if (M == 0 || (!d_mul && !d_pre)) return ROVER_OK;
    Operands ops("gated_sum_backward");
    ops.read("d_out", d_out, d_out_stride, M, N, 4);
    if (d_pre) ops.read("mul", mul, mul_stride, M, N, 4, OP_STRIDE0);
    ops.read("pre", pre, pre_stride, M, N, 4, OP_STRIDE0).written("d_mul", d_mul, d_mul_stride, M, N, 4, OP_OPTIONAL)
        .written("d_pre", d_pre, d_pre_stride, M, N, 4, OP_OPTIONAL);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    GatedSumBwdArgs a{d_out, d_out_stride, mul, mul_stride, pre, pre_stride, d_mul, d_mul_stride, d_pre, d_pre_stride, M, N};
    HIP_TRY(c, launch_gated_sum_backward(a, (hipStream_t)stream));
    return ROVER_OK;
}

// Validates the whole descriptor before the ctx is looked at (a NULL ctx reports through rover_last_error(NULL)): the refusals can be
// checked without a device.
int rover_obs_noise(rover_ctx* c, const rover_obs_noise_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "obs_noise: null descriptor");
    if (d->M < 0 || d->F < 0) return fail(c, ROVER_E_INVALID, "obs_noise: M = %d or F = %d is negative", d->M, d->F);
    if (d->first < 0 || d->first > d->F) return fail(c, ROVER_E_INVALID, "obs_noise: first = %d outside 0 .. F = %d", d->first, d->F);
    if (d->F - d->first > (1 << 21)) return fail(c, ROVER_E_INVALID, "obs_noise: %d heightmap columns, more than 2^21", d->F - d->first);
    if (!(d->sigma_point >= 0.0f) || !std::isfinite(d->sigma_point) || !(d->sigma_offset >= 0.0f) || !std::isfinite(d->sigma_offset))
        return fail(c, ROVER_E_INVALID, "obs_noise: sigma_point = %g or sigma_offset = %g is negative or not finite", (double)d->sigma_point, (double)d->sigma_offset);
    if (!(d->dropout >= 0.0 && d->dropout <= 1.0)) return fail(c, ROVER_E_INVALID, "obs_noise: dropout = %g outside [0, 1]", d->dropout);
    if (!std::isfinite(d->drop_value)) return fail(c, ROVER_E_INVALID, "obs_noise: drop_value is not finite");
    if (d->row_offset < 0 || d->row_offset + (int64_t)d->M > (int64_t)1 << 32)
        return fail(c, ROVER_E_INVALID, "obs_noise: row_offset = %lld is negative or row_offset + M passes 2^32", (long long)d->row_offset);
    const bool empty = d->M == 0 || d->F == 0;
    if (!empty) {
        Operands ops("obs_noise");
        ops.read("in", d->in, d->in_stride, d->M, d->F, 4).written("out", d->out, d->out_stride, d->M, d->F, 4)
            .read("row_scale", d->row_scale, d->M, 1, d->M, 4, OP_OPTIONAL).read("episode", d->episode, d->M, 1, d->M, 8, OP_OPTIONAL)
            .read("step_dev", d->step_dev, 1, 1, 1, 8, OP_OPTIONAL)
            .same_array("out", "in");
        if (int e = check_operands(c, ops, false)) return e;
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "obs_noise: null ctx");
    if (empty) return ROVER_OK;
    USE_DEVICE(c);
    ObsNoiseArgs a{};
    a.in = d->in; a.in_stride = d->in_stride; a.out = d->out; a.out_stride = d->out_stride;
    a.M = d->M; a.F = d->F; a.first = d->first;
    a.sigma_point = d->sigma_point; a.sigma_offset = d->sigma_offset; a.drop_value = d->drop_value;
    (void)rover_obs_noise_threshold(d->dropout, &a.thr);
    a.row_scale = d->row_scale; a.episode = d->episode;
    a.seed = d->seed; a.step = d->step; a.step_dev = d->step_dev; a.row_offset = d->row_offset;
    HIP_TRY(c, launch_obs_noise(a, (hipStream_t)stream));
    return ROVER_OK;
}

// Host only: the dropout threshold rover_obs_noise compares a column's 24-bit word with
int rover_obs_noise_threshold(double dropout, uint32_t* thr) {
    if (!thr || !(dropout >= 0.0 && dropout <= 1.0)) return fail(nullptr, ROVER_E_INVALID, "obs_noise_threshold: null argument or dropout = %g outside [0, 1]", dropout);
    *thr = (uint32_t)llrint(dropout * 16777216.0);
    return ROVER_OK;
}

// Host only: the heightmap columns far first by the horizontal distance of their body point from the camera, ties in column order
int rover_occlusion_order(const double* points, int32_t P, const int64_t* sparse_idx, int32_t Ns, const int64_t* dense_idx, int32_t Nd,
                          const float camera[3], int32_t* order) {
    if (!points || !order || !camera || P <= 0 || Ns < 0 || Nd < 0 || (Ns > 0 && !sparse_idx) || (Nd > 0 && !dense_idx))
        return fail(nullptr, ROVER_E_INVALID, "occlusion_order: null argument or bad counts (P=%d Ns=%d Nd=%d)", P, Ns, Nd);
    if (!std::isfinite(camera[0]) || !std::isfinite(camera[1]) || !std::isfinite(camera[2]))
        return fail(nullptr, ROVER_E_INVALID, "occlusion_order: the camera is not finite");
    const int32_t C = Ns + Nd;
    std::vector<double> key((size_t)C);
    for (int32_t c = 0; c < C; ++c) {
        const int64_t j = c < Ns ? sparse_idx[c] : dense_idx[c - Ns];
        if (j < 0 || j >= P) return fail(nullptr, ROVER_E_INVALID, "occlusion_order: index %lld outside [0,%d)", (long long)j, P);
        const double ax = (double)(float)points[3 * j] - (double)camera[0], ay = (double)(float)points[3 * j + 1] - (double)camera[1];
        const double k = ax * ax + ay * ay;
        key[(size_t)c] = k == k ? k : -1.0;        // a NaN point goes last
    }
    for (int32_t c = 0; c < C; ++c) order[c] = c;
    std::stable_sort(order, order + C, [&](int32_t a, int32_t b) { return key[(size_t)a] > key[(size_t)b]; });
    return ROVER_OK;
}

// The cfg is validated before the ctx is looked at.  Builds the three derived tables whole, then moves them into the ctx in one assignment
// (a failure half way leaves the previous configuration in force).
int rover_set_occlusion(rover_ctx* c, const rover_occlusion_cfg* cfg) {
    if (!cfg) return fail(c, ROVER_E_INVALID, "set_occlusion: null cfg");
    if (!std::isfinite(cfg->camera[0]) || !std::isfinite(cfg->camera[1]) || !std::isfinite(cfg->camera[2]) || !std::isfinite(cfg->step) ||
        !std::isfinite(cfg->clearance) || !std::isfinite(cfg->miss))
        return fail(c, ROVER_E_INVALID, "set_occlusion: camera, step, clearance and miss must be finite");
    if (!(cfg->step > 0.0f)) return fail(c, ROVER_E_INVALID, "set_occlusion: step = %g is not > 0", (double)cfg->step);
    if (cfg->max_steps < 2 || cfg->max_steps > 4096) return fail(c, ROVER_E_INVALID, "set_occlusion: max_steps = %d outside 2 .. 4096", cfg->max_steps);
    if (!(cfg->miss > 0.0f)) return fail(c, ROVER_E_INVALID, "set_occlusion: miss = %g is not > 0", (double)cfg->miss);
    if (!c) return fail(nullptr, ROVER_E_INVALID, "set_occlusion: null ctx");
    if (!c->have_dist) return fail(c, ROVER_E_STATE, "set_occlusion: rover_set_distribution first");
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "set_occlusion: rover_set_heightfield first");
    USE_DEVICE(c);
    const int32_t C = c->Ns + c->Nd;
    std::vector<double> pts((size_t)c->P * 3);
    std::vector<int32_t> idx((size_t)C);
    HIP_TRY(c, hipMemcpy(pts.data(), c->d_dist.get(), pts.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (C) HIP_TRY(c, hipMemcpy(idx.data(), c->d_obs_idx.get(), idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> idx64(idx.begin(), idx.end());
    std::vector<float> body((size_t)C * 3);
    for (int32_t k = 0; k < C; ++k)
        for (int i = 0; i < 3; ++i) body[(size_t)3 * k + i] = (float)pts[(size_t)3 * idx[(size_t)k] + i];
    std::vector<int32_t> order((size_t)C);
    if (int e = rover_occlusion_order(pts.data(), c->P, idx64.data(), c->Ns, idx64.data() + c->Ns, c->Nd, cfg->camera, order.data()))
        return fail(c, e, "set_occlusion: %s", g_create_err.c_str());
    OcclusionTables t;
    t.cfg = *cfg;
    t.TN0 = (c->hf.N0 + OCC_TILE - 1) / OCC_TILE; t.TN1 = (c->hf.N1 + OCC_TILE - 1) / OCC_TILE;
    HIP_TRY(c, t.body3.alloc(body.size() + 1));
    HIP_TRY(c, t.order.alloc(order.size() + 1));
    HIP_TRY(c, t.tilemax.alloc((size_t)t.TN0 * t.TN1));
    if (C) HIP_TRY(c, hipMemcpy(t.body3.get(), body.data(), body.size() * sizeof(float), hipMemcpyHostToDevice));
    if (C) HIP_TRY(c, hipMemcpy(t.order.get(), order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, launch_occlusion_tiles(c->hf, t.tilemax.get(), t.TN0, t.TN1, nullptr));
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    t.dist_gen = c->dist_gen; t.hf_gen = c->hf_gen;
    t.set = true;
    c->occ = std::move(t);
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_obs_noise
int rover_obs_occlusion(rover_ctx* c, const rover_obs_occlusion_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "obs_occlusion: null descriptor");
    if (d->M < 0 || d->F < 0) return fail(c, ROVER_E_INVALID, "obs_occlusion: M = %d or F = %d is negative", d->M, d->F);
    if (d->first < 0 || d->first > d->F) return fail(c, ROVER_E_INVALID, "obs_occlusion: first = %d outside 0 .. F = %d", d->first, d->F);
    if (!std::isfinite(d->drop_value)) return fail(c, ROVER_E_INVALID, "obs_occlusion: drop_value is not finite");
    const bool empty = d->M == 0 || d->F == 0;
    const int64_t C = (int64_t)d->F - d->first;
    if (!empty) {
        Operands ops("obs_occlusion");
        ops.read("pos3", d->pos3, 3, d->M, 3, 4).read("quat4", d->quat4, 4, d->M, 4, 4)
            .read("clean", d->clean, d->clean_stride, d->M, d->F, 4).read("in", d->in, d->in_stride, d->M, d->F, 4)
            .written("out", d->out, d->out_stride, d->M, d->F, 4)
            .written("hidden_u8", d->hidden_u8, d->hidden_stride, d->M, C, 1, OP_OPTIONAL).written("target3", d->target3, 3 * C, d->M, 3 * C, 4, OP_OPTIONAL)
            .same_array("out", "in");
        if (int e = check_operands(c, ops, false)) return e;
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "obs_occlusion: null ctx");
    if (!c->have_dist) return fail(c, ROVER_E_STATE, "obs_occlusion: rover_set_distribution first");
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "obs_occlusion: rover_set_heightfield first");
    if (!c->occ.set) return fail(c, ROVER_E_STATE, "obs_occlusion: rover_set_occlusion first");
    if (c->occ.dist_gen != c->dist_gen || c->occ.hf_gen != c->hf_gen)
        return fail(c, ROVER_E_STATE, "obs_occlusion: the %s was set again after rover_set_occlusion: call rover_set_occlusion again",
                    c->occ.dist_gen != c->dist_gen ? "distribution" : "heightfield");
    if (C != (int64_t)c->Ns + c->Nd)
        return fail(c, ROVER_E_STATE, "obs_occlusion: F - first = %lld columns, the distribution has Ns + Nd = %d", (long long)C, c->Ns + c->Nd);
    if (empty) return ROVER_OK;
    USE_DEVICE(c);
    const OcclusionTables& t = c->occ;
    OcclusionArgs a{};
    a.h = c->hf;
    a.tilemax = t.tilemax.get(); a.TN0 = t.TN0; a.TN1 = t.TN1;
    a.body3 = t.body3.get(); a.order = t.order.get();
    a.pos3 = d->pos3; a.quat4 = d->quat4;
    a.clean = d->clean; a.clean_stride = d->clean_stride; a.in = d->in; a.in_stride = d->in_stride; a.out = d->out; a.out_stride = d->out_stride;
    a.hidden = d->hidden_u8; a.hidden_stride = d->hidden_stride; a.target3 = d->target3;
    a.M = d->M; a.F = d->F; a.first = d->first;
    for (int i = 0; i < 3; ++i) a.camera[i] = t.cfg.camera[i];
    a.step = t.cfg.step; a.clearance = t.cfg.clearance; a.miss = t.cfg.miss; a.drop_value = d->drop_value;
    a.max_steps = t.cfg.max_steps; a.route = c->occlusion_route;
    HIP_TRY(c, launch_obs_occlusion(a, (hipStream_t)stream));
    return ROVER_OK;
}

// Host only, a pure function of (M, N): the route, the chunking and the scratch of rover_scaler_update
int rover_scaler_plan(int32_t M, int32_t N, rover_scaler_plan_desc* plan) {
    if (!plan) return fail(nullptr, ROVER_E_INVALID, "scaler_plan: null plan");
    if (N < 1 || N > 4096) return fail(nullptr, ROVER_E_INVALID, "scaler_plan: N = %d outside 1 .. 4096", N);
    if (M < 0 || (int64_t)M * N >= (int64_t)1 << 31) return fail(nullptr, ROVER_E_INVALID, "scaler_plan: M = %d is negative or M N >= 2^31", M);
    const bool narrow = (uint32_t)N <= SCALER_NARROW_MAX_N;
    plan->route = narrow ? ROVER_SCALER_NARROW : ROVER_SCALER_WIDE;
    plan->rows_per_chunk = narrow ? 16384 : (M <= 8192 ? 32 : 128);
    plan->n_chunks = (int32_t)(((int64_t)M + plan->rows_per_chunk - 1) / plan->rows_per_chunk);
    plan->scratch_bytes = 8 + (int64_t)24 * plan->n_chunks * N;
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_obs_noise
int rover_scaler_update(rover_ctx* c, const rover_scaler_update_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "scaler_update: null descriptor");
    rover_scaler_plan_desc plan;
    if (d->N < 1 || d->N > 4096) return fail(c, ROVER_E_INVALID, "scaler_update: N = %d outside 1 .. 4096", d->N);
    if (d->M < 0 || (int64_t)d->M * d->N >= (int64_t)1 << 31) return fail(c, ROVER_E_INVALID, "scaler_update: M = %d is negative or M N >= 2^31", d->M);
    if (d->M < 2) return fail(c, ROVER_E_INVALID, "scaler_update: M = %d rows, a train call needs at least 2 (the unbiased variance of one row is undefined)", d->M);
    (void)rover_scaler_plan(d->M, d->N, &plan);
    if (d->scratch_bytes < plan.scratch_bytes)
        return fail(c, ROVER_E_INVALID, "scaler_update: scratch of %lld bytes, the plan needs %lld", (long long)d->scratch_bytes, (long long)plan.scratch_bytes);
    Operands ops("scaler_update");
    ops.read("x", d->x, d->x_stride, d->M, d->N, 4).written("scratch", d->scratch, 0, 1, d->scratch_bytes, 1, OP_BYTES, 8)
        .state("mean", d->mean, d->N, 1, d->N, 8, 0, 8).state("var", d->var, d->N, 1, d->N, 8, 0, 8).state("count", d->count, 1, 1, 1, 8, 0, 8)
        .read("skip_if", d->skip_if, 1, 1, 1, 4, OP_OPTIONAL, 4);
    if (int e = check_operands(c, ops)) return e;
    USE_DEVICE(c);
    ScalerUpdateArgs a{};
    a.x = d->x; a.x_stride = d->x_stride;
    a.M = (uint32_t)d->M; a.N = (uint32_t)d->N; a.rows_per_chunk = (uint32_t)plan.rows_per_chunk; a.n_chunks = (uint32_t)plan.n_chunks;
    a.partials = (double*)d->scratch + 1;
    a.mean = d->mean; a.var = d->var; a.count = d->count; a.skip_if = d->skip_if;
    HIP_TRY(c, launch_scaler_update(a, plan.route == ROVER_SCALER_NARROW ? SCALER_ROUTE_NARROW : SCALER_ROUTE_WIDE, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_scaler_apply(rover_ctx* c, const rover_scaler_apply_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "scaler_apply: null descriptor");
    if (d->N < 1 || d->N > 4096) return fail(c, ROVER_E_INVALID, "scaler_apply: N = %d outside 1 .. 4096", d->N);
    if (d->M < 0 || (int64_t)d->M * d->N >= (int64_t)1 << 31) return fail(c, ROVER_E_INVALID, "scaler_apply: M = %d is negative or M N >= 2^31", d->M);
    if (!(d->epsilon >= 0.0) || !std::isfinite(d->epsilon) || !(d->clip >= 0.0) || !std::isfinite(d->clip))
        return fail(c, ROVER_E_INVALID, "scaler_apply: epsilon = %g or clip = %g is negative or not finite", d->epsilon, d->clip);
    Operands ops("scaler_apply");
    if (d->M > 0) ops.read("x", d->x, d->x_stride, d->M, d->N, 4).written("y", d->y, d->y_stride, d->M, d->N, 4).same_array("y", "x");
    ops.state("mean", d->mean, d->N, 1, d->N, 8, 0, 8).state("var", d->var, d->N, 1, d->N, 8, 0, 8);      // only read here, but clear of x and y too
    if (int e = check_operands(c, ops)) return e;
    if (d->M == 0) return ROVER_OK;
    USE_DEVICE(c);
    ScalerApplyArgs a{d->x, d->x_stride, d->y, d->y_stride, (uint32_t)d->M, (uint32_t)d->N, d->mean, d->var, (float)d->epsilon, (float)d->clip};
    HIP_TRY(c, launch_scaler_apply(a, d->inverse != 0, (hipStream_t)stream));
    return ROVER_OK;
}

// The checks that rover_motion_step and rover_motion_step_bogie share, in two parts: the descriptor's own, which need no ctx ...
static int motion_check_desc(rover_ctx* c, const rover_motion_desc* d, const char* what) {
    if (!d) return fail(c, ROVER_E_INVALID, "%s: null descriptor", what);
    if (d->E < 0 || d->substeps < 1 || d->cmd_stride < 1)
        return fail(c, ROVER_E_INVALID, "%s: E = %d is negative, substeps = %d or cmd_stride = %d is below 1", what, d->E, d->substeps, d->cmd_stride);
    if (!std::isfinite(d->dt) || !(d->dt > 0.0f)) return fail(c, ROVER_E_INVALID, "%s: dt = %g is not finite or not > 0", what, (double)d->dt);
    if (d->E > 0 && (!d->pos3 || !d->quat4 || !d->lin || !d->ang)) return fail(c, ROVER_E_INVALID, "%s: pos3, quat4, lin and ang must be given", what);
    const int n_joint = (d->joint_pos_targets13 != nullptr) + (d->joint_vel_targets13 != nullptr) + (d->joint_pos13 != nullptr) + (d->joint_vel13 != nullptr);
    if (n_joint != 0 && n_joint != 4)
        return fail(c, ROVER_E_INVALID, "%s: joint_pos_targets13, joint_vel_targets13, joint_pos13 and joint_vel13 go together (%d of 4 given)", what, n_joint);
    return ROVER_OK;
}

// ... and the ctx's, after which the kernel's arguments are filled in
static int motion_check_ctx(rover_ctx* c, const rover_motion_desc* d, const char* what, MotionArgs& a) {
    if (!c) return fail(nullptr, ROVER_E_INVALID, "%s: null ctx", what);
    if (!c->have_hf) return fail(c, ROVER_E_STATE, "%s: rover_set_heightfield first", what);
    a.h = c->hf;
    a.pos3 = d->pos3; a.quat4 = d->quat4; a.lin = d->lin; a.ang = d->ang;
    a.cmd_stride = d->cmd_stride; a.E = (uint32_t)d->E; a.substeps = d->substeps;
    a.dt = d->dt; a.max_lin = d->max_lin; a.max_ang = d->max_ang; a.ride_height = d->ride_height;
    a.joint_pos_targets13 = d->joint_pos_targets13; a.joint_vel_targets13 = d->joint_vel_targets13;
    a.joint_pos13 = d->joint_pos13; a.joint_vel13 = d->joint_vel13;
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_obs_noise
int rover_motion_step(rover_ctx* c, const rover_motion_desc* d, void* stream) {
    const char* what = "motion_step";
    if (int e = motion_check_desc(c, d, what)) return e;
    MotionArgs a{};
    if (int e = motion_check_ctx(c, d, what, a)) return e;
    if (d->E == 0) return ROVER_OK;
    USE_DEVICE(c);
    motion_plane_fit(a.fit);
    HIP_TRY(c, launch_motion(a, (hipStream_t)stream));
    return ROVER_OK;
}

// The rocker-bogie posture mode: rover_motion_step's refusals and the two parameters', all before the ctx is looked at
int rover_motion_step_bogie(rover_ctx* c, const rover_motion_desc* d, const rover_bogie_params* p, void* stream) {
    const char* what = "motion_step_bogie";
    if (int e = motion_check_desc(c, d, what)) return e;
    if (!p) return fail(c, ROVER_E_INVALID, "%s: null parameters", what);
    if (p->iters < 1 || p->iters > ROVER_BOGIE_MAX_ITERS)
        return fail(c, ROVER_E_INVALID, "%s: iters = %d is outside 1 .. %d", what, p->iters, ROVER_BOGIE_MAX_ITERS);
    if (!std::isfinite(p->max_bogie) || !(p->max_bogie > 0.0f))
        return fail(c, ROVER_E_INVALID, "%s: max_bogie = %g is not finite or not > 0", what, (double)p->max_bogie);
    MotionArgs a{};
    if (int e = motion_check_ctx(c, d, what, a)) return e;
    if (d->E == 0) return ROVER_OK;
    USE_DEVICE(c);
    HIP_TRY(c, launch_motion_bogie(a, p->iters, p->max_bogie, (hipStream_t)stream));
    return ROVER_OK;
}

// Host only: the constant of the posture solve
int rover_motion_bogie_fit(float out[36]) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "motion_bogie_fit: null argument");
    float inv[MOTION_WHEELS][MOTION_WHEELS];
    motion_bogie_fit(inv);
    memcpy(out, inv, sizeof inv);
    return ROVER_OK;
}

// Host only: the constant of the motion model's plane fit
int rover_motion_plane_fit(float out[18]) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "motion_plane_fit: null argument");
    float fit[3][MOTION_WHEELS];
    motion_plane_fit(fit);
    memcpy(out, fit, sizeof fit);
    return ROVER_OK;
}

static bool track_shape_ok(int32_t E, int32_t W, int32_t K) {
    return E >= 0 && W >= 1 && W <= ROVER_TRACK_MAX_WINDOW && K >= 0 && K <= ROVER_TRACK_MAX_COMPONENTS;
}

// Host only: what the descriptor's scratch must cover
int rover_track_sizes(int32_t E, int32_t W, int32_t K, rover_track_sizes_out* out) {
    if (!out) return fail(nullptr, ROVER_E_INVALID, "track_sizes: null argument");
    if (!track_shape_ok(E, W, K))
        return fail(nullptr, ROVER_E_INVALID, "track_sizes: E = %d is negative, W = %d is outside 1 .. %d or K = %d is outside 0 .. %d", E, W,
                    ROVER_TRACK_MAX_WINDOW, K, ROVER_TRACK_MAX_COMPONENTS);
    out->workgroup = TRACK_BLOCK;
    out->n_partials = (int32_t)track_partials((uint32_t)E);
    out->partial_bytes = (int64_t)track_partial_bytes();
    out->finished_slots = (int64_t)out->n_partials * TRACK_BLOCK;
    out->scratch_bytes = (int64_t)track_scratch_bytes((uint32_t)E);
    return ROVER_OK;
}

// The descriptor is validated before the ctx is looked at, as for rover_motion_step
int rover_episode_track(rover_ctx* c, const rover_track_desc* d, void* stream) {
    if (!d) return fail(c, ROVER_E_INVALID, "episode_track: null descriptor");
    if (!track_shape_ok(d->E, d->W, d->K))
        return fail(c, ROVER_E_INVALID, "episode_track: E = %d is negative, W = %d is outside 1 .. %d or K = %d is outside 0 .. %d", d->E, d->W,
                    ROVER_TRACK_MAX_WINDOW, d->K, ROVER_TRACK_MAX_COMPONENTS);
    if (d->done_size != 1 && d->done_size != 8) return fail(c, ROVER_E_INVALID, "episode_track: done_size = %d is neither 1 nor 8", d->done_size);
    for (int32_t k = 0; k < d->K; ++k)
        if (d->comp_kind[k] != ROVER_TRACK_F32 && d->comp_kind[k] != ROVER_TRACK_I64)
            return fail(c, ROVER_E_INVALID, "episode_track: comp_kind[%d] = %d is neither ROVER_TRACK_F32 nor ROVER_TRACK_I64", k, d->comp_kind[k]);
    if (!d->ring_ret || !d->ring_len || !d->ring_count || !d->record)
        return fail(c, ROVER_E_INVALID, "episode_track: ring_ret, ring_len, ring_count and record must be given");
    if (d->E > 0) {
        if (!d->rewards || !d->done || !d->cum_reward || !d->cum_steps || !d->scratch)
            return fail(c, ROVER_E_INVALID, "episode_track: rewards, done, cum_reward, cum_steps and scratch must be given");
        for (int32_t k = 0; k < d->K; ++k)
            if (!d->comp[k]) return fail(c, ROVER_E_INVALID, "episode_track: comp[%d] is NULL (K = %d)", k, d->K);
        if (((uintptr_t)d->scratch & 7u) != 0) return fail(c, ROVER_E_INVALID, "episode_track: scratch is not 8-byte aligned");
        if (d->scratch_bytes < (int64_t)track_scratch_bytes((uint32_t)d->E))
            return fail(c, ROVER_E_INVALID, "episode_track: scratch_bytes = %lld is below the %llu of rover_track_sizes", (long long)d->scratch_bytes,
                        (unsigned long long)track_scratch_bytes((uint32_t)d->E));
    }
    if (!c) return fail(nullptr, ROVER_E_INVALID, "episode_track: null ctx");
    USE_DEVICE(c);
    TrackArgs a{};
    a.rewards = d->rewards; a.done = d->done; a.done8 = d->done_size == 8;
    a.E = (uint32_t)d->E; a.W = (uint32_t)d->W; a.K = (uint32_t)d->K;
    for (int32_t k = 0; k < d->K; ++k) {
        a.comp[k] = d->comp[k];
        if (d->comp_kind[k] == ROVER_TRACK_I64) a.comp_i64 |= 1u << k;
    }
    a.cum_reward = d->cum_reward; a.cum_steps = d->cum_steps;
    a.ring_ret = d->ring_ret; a.ring_len = d->ring_len; a.ring_count = d->ring_count;
    a.record = d->record; a.scratch = d->scratch;
    HIP_TRY(c, launch_track(a, (hipStream_t)stream));
    return ROVER_OK;
}

int rover_set_option(rover_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return ROVER_E_INVALID;
    USE_DEVICE(c);                                 // some options (re)allocate device workspace
    const KnobRow* k = knob_by_option(name);
    if (!k) return fail(c, ROVER_E_INVALID, "unknown option '%s'", name);
    if (!knob_option_accepts(*k, (double)value)) return fail(c, ROVER_E_INVALID, "%s must be %s", name, k->values);
    if ((k->flags & KNOB_MUST_RUN) && value == 4 && staged_tables_missing(plan_inputs(c)))
        return fail(c, ROVER_E_STATE, "raycast_variant 4 (staged) needs its tables for the arithmetic in force: they were not built (option "
                                      "staged_tables, or they did not fit when the maps were set)");
    k->set(c, (double)value);
    if (k->invalidates & KNOB_RAYS_OBS) {
        c->hf.rcp = c->cell_rcp;
        c->rays_valid = false;
        c->obs_valid = false;
    }
    return (k->invalidates & KNOB_REPLAN) ? replan(c, (k->invalidates & KNOB_BINS) ? REALLOC_BINS : REALLOC_QUEUE) : ROVER_OK;
}

int rover_plan_raycast(const rover_plan_query* q, rover_raycast_plan* out) {
    if (!q || !out) return fail(nullptr, ROVER_E_INVALID, "plan_raycast: null argument");
    if (q->num_envs <= 0 || q->P < 0 || (q->have_dist && q->P == 0))
        return fail(nullptr, ROVER_E_INVALID, "plan_raycast: num_envs=%d P=%d have_dist=%d", q->num_envs, q->P, q->have_dist);
    const struct { const char* option; int64_t value; } given[] = {
        {"raycast_variant", q->raycast_variant}, {"raycast_run", q->raycast_run}, {"lane_env_order", q->lane_env_order}, {"lane_rocks", q->lane_rocks},
        {"bin_low_bits", q->bin_low_bits}, {"cull_queue_mb", q->cull_queue_mb}, {"ray_precision", q->ray_precision}};
    for (const auto& g : given)
        if (!knob_option_accepts(*knob_by_option(g.option), (double)g.value))
            return fail(nullptr, ROVER_E_INVALID, "plan_raycast: %s must be %s", g.option, knob_by_option(g.option)->values);
    PlanInputs in;
    in.num_envs = q->num_envs; in.P = q->P; in.have_dist = q->have_dist != 0; in.precision = q->ray_precision;
    in.knobs.variant = q->raycast_variant; in.knobs.run = (uint32_t)q->raycast_run; in.knobs.lane_env_order = q->lane_env_order;
    in.knobs.lane_rocks = q->lane_rocks; in.knobs.cull_lazy = q->cull_lazy; in.knobs.low_bits_opt = (uint32_t)q->bin_low_bits;
    in.knobs.cull_budget = (uint64_t)q->cull_queue_mb << 20;
    for (int w = 0; w < 2; ++w) {
        MapShape& m = in.map[w];
        if (q->map_present[w] && (q->X[w] <= 0 || q->Y[w] <= 0 || q->K8[w] <= 0 || q->K8[w] % 8 || q->cells_with_far_bound[w] < 0 ||
                                  q->cells_with_far_bound[w] > (int64_t)q->X[w] * q->Y[w]))
            return fail(nullptr, ROVER_E_INVALID, "plan_raycast: map %d: X=%d Y=%d K8=%d cells_with_far_bound=%lld", w, q->X[w], q->Y[w], q->K8[w],
                        (long long)q->cells_with_far_bound[w]);
        if (!q->map_present[w]) continue;
        m.present = true; m.X = q->X[w]; m.Y = q->Y[w]; m.K8 = q->K8[w]; m.cells = (int64_t)q->X[w] * q->Y[w]; m.farok = q->cells_with_far_bound[w];
        m.has_cull_tables = q->has_cull_tables[w] != 0;
        for (int k = 0; k < 2; ++k) m.has_staged_tables[k] = q->has_staged_tables[w][k] != 0;
    }
    memset(out, 0, sizeof *out);
    plan_to_c(plan_step(in), out);
    return ROVER_OK;
}

int rover_set_profiling(rover_ctx* c, int32_t enable) {
    if (!c) return ROVER_E_INVALID;
    USE_DEVICE(c);
    if (enable && c->ev0.empty()) {
        // created into locals and swapped in only when all 2 x 256 exist: a partial failure leaves the ctx without events
        std::vector<hipEvent_t> e0, e1;
        hipError_t e = hipSuccess;
        for (int i = 0; i < kProfRing && e == hipSuccess; ++i) {
            hipEvent_t a = nullptr, b = nullptr;
            e = hipEventCreate(&a);
            if (e == hipSuccess) { e0.push_back(a); e = hipEventCreate(&b); }
            if (e == hipSuccess) e1.push_back(b);
        }
        if (e != hipSuccess) {
            for (auto& x : e0) (void)hipEventDestroy(x);
            for (auto& x : e1) (void)hipEventDestroy(x);
            return fail(c, ROVER_E_HIP, "set_profiling: hipEventCreate: %s", hipGetErrorString(e));
        }
        c->ev0.swap(e0); c->ev1.swap(e1);
    }
    if (c->prof_pending) (void)prof_drain(c);
    c->profiling = enable != 0;
    if (enable) { c->prof_ms = 0.0; c->prof_launches = 0; c->prof_seen = 0; c->prof_every = enable > 1 ? enable : 1; }
    return ROVER_OK;
}

int rover_get_profile(rover_ctx* c, rover_profile* out) {
    if (!c || !out) return ROVER_E_INVALID;
    USE_DEVICE(c);
    if (prof_drain(c)) return fail(c, ROVER_E_HIP, "get_profile: event drain failed");
    out->raycast_ms = c->prof_ms;
    out->launches = c->prof_launches;
    out->pairs_per_launch = (uint64_t)c->cfg.num_envs * ((uint64_t)c->P * (uint64_t)c->maps[0].knn.K + 26ull * (uint64_t)c->maps[1].knn.K);
    return ROVER_OK;
}

int rover_replay_raycast(rover_ctx* c, void* stream) {
    if (!c) return ROVER_E_INVALID;
    if (int r = check_ready(c)) return r;
    if (!c->rays_valid) return fail(c, ROVER_E_STATE, "replay_raycast: no ray records yet (run a step first)");
    USE_DEVICE(c);
    StepPlan p = c->plan;
    if (p.sorted && !c->ws_plan.sorted) { p = StepPlan{}; p.variant = 1; p.R8 = c->plan.R8; }     // no sorted list from the last step: only an env-order kernel can replay
    if (int r = check_queue(c, p)) return r;
    return run_raycast(c, p, (uint32_t)c->cfg.num_envs * (26u + (uint32_t)c->P), (hipStream_t)stream);
}

}  // extern "C"
