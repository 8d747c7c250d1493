// rover_plan.cpp — plan_step(): the ray cast of a step and the sizes that follow from it, from shapes and knobs alone (rover_plan.h).
// Every threshold is a named constant with the trade it settles; the measurements behind each are in EXPERIMENTS.md §10, by the same names.
#include "rover_plan.h"

namespace rover {

// ---- which kernel (EXPERIMENTS.md §10.1) ----
static const uint64_t kCullRaysF32 = 49152;       // f32, no staged tables: above this many rays the culled kernel's saving exceeds the sort's four launches
static const uint64_t kStagedRaysF32 = 24576;     // f32: from here the staged kernel (in env order: no sort to pay for) passes the env-order kernel
static const uint64_t kBinnedRaysF16 = 24576;     // as shipped: up to here the binned kernel, which has no tables to walk, stays ahead
static const uint64_t kStagedEnvRaysF16 = 98304;  // as shipped: below this the staged kernel in env order beats the culled one; beyond, the mesh decides
// ---- rays per wave behind the sort (§10.2): long runs amortise a cell's set-up, short ones fill the machine and balance long-lived waves ----
static const uint64_t kStagedRun64 = 12;          // staged kernel: r = rays / 65 536 from which a run is 64 rays (32 below)
static const uint64_t kQuickRun[3] = {3, 6, 20};  // culled kernel, regular mesh in f32: first r of runs of 16, 32, 64 (8 below)
static const uint64_t kSlowRun[3] = {12, 24, 48}; // culled kernel, irregular mesh or as shipped (more candidates per ray): the same, later
// ---- env order or sort for the staged kernel (§10.3): the sort pays once a cell's rays come from several rovers ----
static const uint64_t kEnvOrderRaysPerCellX2 = 3; // env order while heightmap rays per terrain cell < 3 / 2 ...
static const uint64_t kEnvOrderCellsPerEnv = 64;  // ... and a rover has more than 64 terrain cells to itself
// ---- slots per wave in env order (§10.4): enough waves to fill 1 024 SIMDs ----
static const uint64_t kEnvRun32Slots = 1ull << 17, kEnvRun64Slots = 1ull << 20;
// ---- the culled kernel's two choices (§10.5): what a bin's far records and a cleared cell's rays cost against what skipping them saves ----
static const int64_t kSparseRaysPerEnv = 100;     // 26 + P below this: few rays per bin at any batch size -> far records on demand
static const uint64_t kFewRaysPerCell = 8;        // ... or fewer heightmap rays per terrain cell than this
static const int64_t kDenseRaysPerEnv = 260;      // beyond this a ray set has next to no ray that clears its whole cell: no skip, no on-demand records
// ---- the sort's digit (§10.6) ----
static const uint32_t kMaxBuckets = 4096;         // bucket totals and starts live in one 4 096-entry scan

static uint64_t valid_rays(const PlanInputs& in) { return (uint64_t)in.num_envs * (26u + (uint64_t)in.P); }
static bool have_maps(const PlanInputs& in) { return in.map[0].present && in.map[1].present; }
static bool regular_mesh(const PlanInputs& in) { return 2 * in.map[0].farok >= in.map[0].cells; }      // most terrain cells have a usable far bound
static bool staged_tables_ok(const PlanInputs& in) {
    const int k = in.precision == 2 ? 1 : 0;
    return in.map[0].has_staged_tables[k] && in.map[1].has_staged_tables[k];
}

bool staged_tables_missing(const PlanInputs& in) {
    return have_maps(in) && in.map[0].K8 <= 256 && in.map[1].K8 <= 256 && !staged_tables_ok(in);
}

static int plan_variant(const PlanInputs& in) {
    const int asked = in.knobs.variant;
    const bool v2_ok = in.map[0].K8 <= 256 && in.map[1].K8 <= 256;      // 64 lanes x 4 triangles
    if (asked == 1 || !v2_ok) return 1;
    const bool v4_ok = staged_tables_ok(in);     // the staged kernel's tables of the proof in force, on both maps
    if (asked == 0 && in.precision != 2 && in.have_dist && valid_rays(in) < (v4_ok ? kStagedRaysF32 : kCullRaysF32 + 1u)) return 1;
    if (asked == 0 && in.precision == 2 && in.have_dist && valid_rays(in) <= kBinnedRaysF16) return 2;
    // variant 3 (culled): its exact phase runs either arithmetic (f32 / as shipped), each with its own proof tables
    const bool v3_ok = in.map[0].has_cull_tables && in.map[1].has_cull_tables;
    if (asked == 2 || !v3_ok) return 2;
    if (v4_ok && asked == 4) return 4;
    if (v4_ok && asked == 0 && in.have_dist) {
        if (in.precision != 2) { if (valid_rays(in) >= kStagedRaysF32) return 4; }
        // as shipped the culled kernel stays ahead on large sparse ray sets over an irregular terrain mesh only: staged below
        // kStagedEnvRaysF16, on a regular mesh, and from two heightmap rays per terrain cell
        else if (valid_rays(in) < kStagedEnvRaysF16 || regular_mesh(in) ||
                 (uint64_t)in.num_envs * (uint64_t)in.P >= 2ull * (uint64_t)in.map[0].cells) return 4;
    }
    return 3;
}

// sorted rays per wave
static uint32_t plan_run(const PlanInputs& in, int variant) {
    if (in.knobs.run) return in.knobs.run;
    const uint64_t r = valid_rays(in) / 65536u;
    if (variant == 4) return r < kStagedRun64 ? 32u : 64u;
    if (variant >= 3) {
        const uint64_t* at = in.precision != 2 && regular_mesh(in) ? kQuickRun : kSlowRun;      // powers of two: 63 instead of 64 cost 6 %
        return r < at[0] ? 8u : (r < at[1] ? 16u : (r < at[2] ? 32u : 64u));
    }
    return (uint32_t)(r < 4 ? 4 : (r > 32 ? 32 : r));
}

// The staged ray cast needs no bins: where a (map, cell) bin holds a ray or none the sort's launches buy it nothing and it walks the ray
// slots in env order (a run = consecutive slots: a rover's heightmap rays still share cells)
static bool plan_env_order(const PlanInputs& in, int variant) {
    if (variant != 4) return false;
    if (in.knobs.lane_env_order >= 0) return in.knobs.lane_env_order != 0;
    if (in.precision == 2) return in.have_dist && valid_rays(in) < kStagedEnvRaysF16;
    return in.have_dist && 2ull * (uint64_t)in.num_envs * (uint64_t)in.P < kEnvOrderRaysPerCellX2 * (uint64_t)in.map[0].cells &&
           kEnvOrderCellsPerEnv * (uint64_t)in.num_envs < (uint64_t)in.map[0].cells;
}

// bins per sort bucket = 2^low_bits: the option, or 10; raised while the buckets exceed kMaxBuckets; lowered (library's choice only) when
// that lets a sort entry — low bin bits | slot id — fit one dword and the buckets still fit
static uint32_t plan_low_bits(const PlanInputs& in, uint64_t n_bins, uint64_t n_slots) {
    auto buckets = [n_bins](uint32_t lb) { return (uint32_t)((n_bins + (1u << lb) - 1u) >> lb); };
    uint32_t low_bits = in.knobs.low_bits_opt ? in.knobs.low_bits_opt : 10u;
    while (low_bits < 12u && buckets(low_bits) > kMaxBuckets) ++low_bits;
    if (!in.knobs.low_bits_opt && in.have_dist) {
        uint32_t lb = low_bits;
        while (lb > 8u && n_slots > (1ull << (32u - lb)) && buckets(lb - 1u) <= kMaxBuckets) --lb;
        if (n_slots <= (1ull << (32u - lb))) low_bits = lb;
    }
    return low_bits;
}

StepPlan plan_step(const PlanInputs& in) {
    StepPlan p{};
    const Knobs& k = in.knobs;
    const uint64_t E = (uint64_t)in.num_envs, terrain_rays = E * (uint64_t)in.P;
    p.proof = in.precision == 2 ? 1 : 0;
    p.R8 = in.P > 0 ? (uint32_t)(((26 + in.P) + 7) / 8 * 8) : 0u;
    const uint64_t n_slots = E * p.R8;
    // the culled kernel: far records on demand where most bins skip them (few rays per bin, a mesh whose cells mostly have a far bound);
    // rays that clear their whole cell left out of the scan where some do
    const bool few_per_bin = in.P <= kDenseRaysPerEnv && terrain_rays < kFewRaysPerCell * (uint64_t)in.map[0].cells;
    const bool lazy_auto = (26 + in.P < kSparseRaysPerEnv || few_per_bin) && regular_mesh(in);
    p.lazy_far = k.cull_lazy < 0 ? lazy_auto : k.cull_lazy != 0;
    p.skip_clear = regular_mesh(in) && 26 + in.P <= kDenseRaysPerEnv;
    if (p.proof && !p.skip_clear) p.lazy_far = false;       // the fp16 proof's kernel without the whole-cell skip is the eager one
    if (!have_maps(in)) return p;
    p.variant = plan_variant(in);
    p.env_order = plan_env_order(in, p.variant);
    p.sorted = p.variant >= 2 && !p.env_order;
    // behind the sort the rocks part goes through the staged kernel too unless lane_rocks says 0 (§10.7); in env order one launch casts every slot
    p.rocks_staged = p.variant == 4 && (p.env_order || k.lane_rocks != 0);
    p.run = plan_run(in, p.variant);
    if (p.env_order) p.env_run = k.run ? (k.run > 64u ? 64u : k.run) : (n_slots >= kEnvRun64Slots ? 64u : (n_slots >= kEnvRun32Slots ? 32u : 16u));
    // the sort
    p.n_bins = (uint64_t)in.map[0].X * in.map[0].Y + (uint64_t)in.map[1].X * in.map[1].Y;
    p.low_bits = plan_low_bits(in, p.n_bins, n_slots);
    if (p.sorted && in.have_dist) {
        p.sort_entry_dwords = bin_entries_packed((uint32_t)n_slots, p.low_bits) ? 1u : 2u;
        p.hist_fused = bin_hist_fused((uint32_t)n_slots, p.R8, (uint32_t)p.n_bins, p.low_bits, &p.hist_blocks_per_tile);
    }
    // the candidate queue (one bounded region per resident wave) and its per-wave counters.  The counters are sized by the PADDED slot
    // count — in env order the staged kernel walks every slot of every env —, the queue, once capped by the budget, by neither
    if (p.variant >= 3 && in.have_dist) {
        p.queue_entries = cull_queue_entries(valid_rays(in), (uint32_t)in.num_envs * (uint32_t)in.P, p.run, k.cull_budget, &p.cull_launches);
        p.stat_slots = cull_stat_slots(n_slots, p.env_order ? p.env_run : p.run);
    }
    return p;
}

bool StepPlan::operator==(const StepPlan& o) const {
    return variant == o.variant && proof == o.proof && sorted == o.sorted && env_order == o.env_order && rocks_staged == o.rocks_staged &&
           run == o.run && env_run == o.env_run && lazy_far == o.lazy_far && skip_clear == o.skip_clear && R8 == o.R8 && n_bins == o.n_bins &&
           low_bits == o.low_bits && sort_entry_dwords == o.sort_entry_dwords && hist_fused == o.hist_fused &&
           hist_blocks_per_tile == o.hist_blocks_per_tile && queue_entries == o.queue_entries && cull_launches == o.cull_launches &&
           stat_slots == o.stat_slots;
}

}  // namespace rover
