// rover_plan.h — what a step launches and how its plan-dependent buffers are sized, as a pure function of shapes and knobs.
// Host only: no rover_ctx, no HIP call.  rover_capi.cpp plans with it (plan_inputs -> plan_step), rover_plan_raycast() answers from it
// without a device, and tests/test_raycast_plan_host.py pins every threshold on the CPU.
#pragma once
#include <stdint.h>

namespace rover {

// Integer helpers that depend on kernel constants: defined next to their kernels (rover_sort.hip, rover_cull.hip), called by plan_step.
// true when launch_bin_rays sorts one-dword entries (low bin bits | slot id) for this many slots, false for (bin, slot) pairs
bool bin_entries_packed(uint32_t n_slots, uint32_t low_bits);
// true when prep_rays_kernel can count the sort's coarse buckets itself (PrepArgs::hist): a 64-env block's keys lie inside one tile of the sort
bool bin_hist_fused(uint32_t n_slots, uint32_t R8, uint32_t n_bins, uint32_t low_bits, uint32_t* blocks_per_tile);
// entries of the candidate queue (capped by budget_bytes) and the launches a culled ray cast over n_rays rays is then cut into
uint64_t cull_queue_entries(uint64_t n_rays, uint32_t n_terrain, uint32_t run, uint64_t budget_bytes, uint32_t* n_launches);
uint32_t cull_stat_slots(uint64_t n_rays, uint32_t run);      // upper bound of the waves of a launch = slots of the per-wave counters
uint32_t lane_waves(uint32_t n_rays, uint32_t run);           // waves the staged kernel starts over n_rays rays
uint32_t lane_pairs_per_row(uint32_t K8);                     // pairs per row of the staged kernel's records

// Everything rover_set_option / the ROVER_* environment can set that enters a plan or a size (the knob table in rover_capi.cpp)
struct Knobs {
    int variant = 0;                    // "raycast_variant": 0 auto, 1 env-order kernel, 2 binned, 3 culled, 4 staged
    uint32_t run = 0;                   // "raycast_run": 0 auto
    int lane_env_order = -1;            // "lane_env_order": variant 4 without the sort: -1 auto, 0 / 1
    int lane_rocks = -1;                // "lane_rocks": variant 4, sorted: the rocks part through the staged kernel too: -1 auto (yes), 0 / 1
    int cull_lazy = -1;                 // ROVER_CULL_LAZY: the culled kernel's on-demand far records: < 0 auto, 0 / else force (experiments)
    uint32_t low_bits_opt = 0;          // "bin_low_bits": 0 chosen by the library, else 8..12
    uint64_t cull_budget = 1536ull << 20;   // "cull_queue_mb": most bytes the candidate queue may take
    int lane_box = -1;                  // "lane_box": the f32 proof's staged records of the next rover_set_knn_map as boxes: -1 auto (where most pairs fill theirs), 0 spheres, 1 boxes
    int lane_pair_rows = -1;            // "lane_pair_rows": the staged tables of the next rover_set_knn_map with one row per two cells: -1 auto (the terrain map), 0 no map, 1 both maps
    int staged_tables = 3;              // "staged_tables": which proofs' staged-kernel tables the next rover_set_knn_map builds (bit 0 f32, bit 1 fp16)
    uint32_t early_out = 1;             // "raycast_early_out": the binned kernel's whole-pair rejection (bit-identical results)
    double cull_eta_h = 0.08;           // ROVER_CULLH_ETA: free parameter of the fp16 proof (rover_cull.hip, cull_proof_h)
    double cull_split_h = 8.0;          // ROVER_CULLH_SPLIT: how test (A)'s cross term is split between its |h|^2 and rho^2 parts
};

struct MapShape {
    bool present = false;
    int32_t X = 0, Y = 0, K8 = 0;
    int64_t cells = 0;                  // X * Y
    int64_t farok = 0;                  // cells whose far bound can hold for a usual ray (rover_cull_info.cells_with_far_bound)
    bool has_cull_tables = false;       // the culled kernel's tables were built (K8 <= 256, ids fit)
    bool has_staged_tables[2] = {false, false};   // the staged kernel's, per proof
};

struct PlanInputs {
    int32_t num_envs = 0;
    int32_t P = 0;                      // heightmap rays per env (0: never set)
    bool have_dist = false;
    int precision = 0;                  // "ray_precision"
    Knobs knobs{};
    MapShape map[2];                    // terrain, rocks
};

// Every host-side value that selects a code path of a step or sizes a plan-dependent buffer.  The ctx holds one (replan); steps, replays,
// allocations and reports read it and derive nothing themselves.
struct StepPlan {
    int variant = 0;                    // 0: a map is missing; 1 env-order kernel, 2 binned, 3 culled, 4 staged
    int proof = 0;                      // the ProofTables in force: 1 for the as-shipped fp16 arithmetic (ray_precision 2), else 0
    bool sorted = false;                // the bucket sort by (map, cell) runs before the ray cast
    bool env_order = false;             // variant 4 over the ray slots in env order, one launch
    bool rocks_staged = false;          // variant 4: the rocks part through the staged kernel too (else the culled kernel casts it)
    uint32_t run = 0;                   // rays per wave of the sorted launches
    uint32_t env_run = 0;               // slots per wave of the staged kernel in env order
    bool lazy_far = false;              // culled kernel: a bin's far records fetched only when a ray needs them
    bool skip_clear = false;            // culled kernel: rays that clear their whole cell left out of the scan
    uint32_t R8 = 0;                    // ray slots per env: 26 + P rounded up to a multiple of 8 (0: no distribution yet)
    uint64_t n_bins = 0;                // (map, cell) bins of the sort: the cells of both maps
    uint32_t low_bits = 10;             // bins per sort bucket = 2^low_bits
    uint32_t sort_entry_dwords = 0;     // 1: low bin bits | slot id, 2: (bin, slot); 0: the step does not sort
    bool hist_fused = false;            // prep_rays_kernel counts the sort's coarse buckets itself
    uint32_t hist_blocks_per_tile = 0;  // ... and this many of its 64-env blocks share a tile of the sort
    uint64_t queue_entries = 0;         // candidate queue of the culled / staged ray cast (0: none)
    uint32_t cull_launches = 0;         // launches the queue budget cuts a culled ray cast over the whole ray set into (0: no queue)
    uint32_t stat_slots = 0;            // per-wave counter slots
    bool operator==(const StepPlan& o) const;
    bool operator!=(const StepPlan& o) const { return !(*this == o); }
};

StepPlan plan_step(const PlanInputs& in);

// raycast_variant 4 asked for by name cannot run: the staged kernel's tables of the arithmetic in force are not there (K > 256 on a map is the
// documented exception: every variant then runs as the streaming kernel 1, and rover_get_info says so)
bool staged_tables_missing(const PlanInputs& in);

}  // namespace rover
