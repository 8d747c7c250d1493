"""The ray-cast plan table: one row per plan the library can choose, with the plan it must report.

Shared by tests/test_raycast_plans_gpu.py (every row on an engine, stepped against the oracle) and tests/test_raycast_plan_host.py (every
row through `_lib.plan_raycast`, the ctx-free planner, on the CPU).  A tuning change edits the expected plans here and says so."""
import pytest

PLAN_FIELDS = ("variant", "proof", "sorted", "env_order", "rocks_staged", "run", "env_run", "lazy_far", "skip_clear", "cull_launches",
               "low_bits", "sort_entry_dwords", "hist_fused")


def plan(variant, proof, sorted, env_order, rocks_staged, run, env_run, lazy_far, skip_clear, cull_launches, low_bits,
         sort_entry_dwords, hist_fused):
    return dict(zip(PLAN_FIELDS, (variant, proof, sorted, env_order, rocks_staged, run, env_run, lazy_far, skip_clear, cull_launches,
                                  low_bits, sort_entry_dwords, hist_fused)))


# ---- (a) the table ---------------------------------------------------------------------------------------------------------------
# (id, scene, rays, envs, precision, options in the order they are set, rover_create extras, expected plan)
# precision: 0 the f32 arithmetic, 2 the reference's as-shipped fp16 arithmetic.  options = {}: the plan is the library's auto choice.
# The expected plans are derived from plan_step() (csrc/rover_plan.cpp) and the helpers it calls (bin_hist_fused(), cull_queue_entries());
# r = envs x (26 + P) / 65 536 (integer division) is what the run length switches on.
def _case(id, scene, rays, envs, precision, options, expect, **create):
    return pytest.param(dict(id=id, scene=scene, rays=rays, envs=envs, precision=precision, options=options, create=create, plan=expect), id=id)


SHARD = dict(env_offset=32768, num_envs_global=262144)      # BASELINE configs[3], rank 1 of 8
PLAN_CASES = [
    # what bench.py times at BASELINE configs[1]: 258 048 rays, 0.84 heightmap rays per cell, one rover per 88 cells -> env order; 2^18 slots -> env_run 32
    _case("cfg1-f32-auto", "A", "37", 4096, 0, {}, plan(4, 0, 0, 1, 1, 32, 32, 1, 1, 1, 10, 0, 0)),
    # as shipped: >= 98 304 rays on a regular mesh -> staged behind the sort; r = 3 -> run 32; R8 = 64 -> fused histogram
    _case("cfg1-shipped-auto", "A", "37", 4096, 2, {}, plan(4, 1, 1, 0, 1, 32, 0, 1, 1, 1, 10, 1, 1)),
    # configs[3], a shard that is not rank 0: 3.4 heightmap rays per cell -> sorted; r = 31 -> run 64; 2^21 slots -> the big sort tile
    _case("cfg3-rank1-f32-auto", "A", "37", 32768, 0, {}, plan(4, 0, 1, 0, 1, 64, 0, 1, 1, 1, 10, 1, 1), **SHARD),
    _case("cfg3-rank1-shipped-auto", "A", "37", 32768, 2, {}, plan(4, 1, 1, 0, 1, 64, 0, 1, 1, 1, 10, 1, 1), **SHARD),
    # 120 + 26 rays (R8 = 152, six padding slots per env): 1.37 heightmap rays per cell -> env order
    _case("p120-f32-auto", "A", "120", 4096, 0, {}, plan(4, 0, 0, 1, 1, 32, 32, 1, 1, 1, 10, 0, 0)),
    # ... as shipped: sorted; 64 x 152 keys of a prep block exceed the sort tile -> no fused histogram
    _case("p120-shipped-auto", "A", "120", 4096, 2, {}, plan(4, 1, 1, 0, 1, 32, 0, 1, 1, 1, 10, 1, 0)),
    # below 2^17 slots: env_run 16; as shipped env order below 98 304 rays
    _case("e512-f32-auto", "A", "37", 512, 0, {}, plan(4, 0, 0, 1, 1, 32, 16, 1, 1, 1, 10, 0, 0)),
    _case("e512-shipped-auto", "A", "37", 512, 2, {}, plan(4, 1, 0, 1, 1, 32, 16, 1, 1, 1, 10, 0, 0)),
    _case("e1024-f32-auto", "A", "37", 1024, 0, {}, plan(4, 0, 0, 1, 1, 32, 16, 1, 1, 1, 10, 0, 0)),
    _case("e1024-shipped-auto", "A", "37", 1024, 2, {}, plan(4, 1, 0, 1, 1, 32, 16, 1, 1, 1, 10, 0, 0)),
    # fewer than 24 576 rays: the env-order kernel (f32), the binned one (as shipped: up to 24 576); no candidate queue
    _case("e256-f32-auto", "A", "37", 256, 0, {}, plan(1, 0, 0, 0, 0, 4, 0, 1, 1, 0, 10, 0, 0)),
    _case("e384-f32-auto", "A", "37", 384, 0, {}, plan(1, 0, 0, 0, 0, 4, 0, 1, 1, 0, 10, 0, 0)),
    _case("e384-shipped-auto", "A", "37", 384, 2, {}, plan(2, 1, 1, 0, 0, 4, 0, 1, 1, 0, 10, 1, 1)),
    # irregular mesh, as shipped, 129 024 rays, 0.84 heightmap rays per cell: the culled kernel as the auto choice, eager far records
    _case("irregular-shipped-auto", "I", "37", 2048, 2, {}, plan(3, 1, 1, 0, 0, 8, 0, 0, 0, 1, 10, 1, 1)),
    # the native 1 634 + 26 rays (R8 = 1 664): dense -> sorted, lazy_far 0, skip_clear 0; r = 12 -> run 64 (staged) / 32 (culled)
    _case("native-f32-auto", "A", "native", 512, 0, {}, plan(4, 0, 1, 0, 1, 64, 0, 0, 0, 1, 10, 1, 0)),
    _case("native-f32-culled", "A", "native", 512, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 32, 0, 0, 0, 1, 10, 1, 0)),
    # the culled kernel's run, regular mesh in f32 (plan_run's first branch): r = 1, 3, 6, 20 — the first r of 16, 32 and 64
    _case("culled-regular-run8", "A", "37", 2048, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 8, 0, 1, 1, 1, 10, 1, 1)),
    _case("culled-regular-run16", "A", "37", 3200, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 16, 0, 1, 1, 1, 10, 1, 1)),
    _case("culled-regular-run32", "A", "37", 6272, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 32, 0, 1, 1, 1, 10, 1, 1)),
    _case("culled-regular-run64", "A", "37", 20864, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 64, 0, 1, 1, 1, 10, 1, 1)),
    # ... irregular mesh (the second branch): r = 1, 12, 24, 48
    _case("culled-irregular-run8", "I", "37", 2048, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 8, 0, 0, 0, 1, 10, 1, 1)),
    _case("culled-irregular-run16", "I", "37", 12544, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 16, 0, 0, 0, 1, 10, 1, 1)),
    _case("culled-irregular-run32", "I", "37", 25088, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 32, 0, 0, 0, 1, 10, 1, 1)),
    _case("culled-irregular-run64", "I", "37", 50176, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 64, 0, 0, 0, 1, 10, 1, 1)),
    # ... as shipped on the regular mesh: the second branch too, the on-demand kernel of the fp16 proof
    _case("culled-regular-shipped-run8", "A", "37", 2048, 2, {"raycast_variant": 3}, plan(3, 1, 1, 0, 0, 8, 0, 1, 1, 1, 10, 1, 1)),
    # eight heightmap rays per cell or more with 146 rays per env: far records eagerly, the whole-cell skip stays (r = 53: run 64 on either branch);
    # R8 = 152 at 3.7 M slots: the big sort tile, no fused histogram
    _case("culled-dense-f32", "A", "120", 24064, 0, {"raycast_variant": 3}, plan(3, 0, 1, 0, 0, 64, 0, 0, 1, 1, 10, 1, 0)),
    _case("culled-dense-shipped", "A", "120", 24064, 2, {"raycast_variant": 3}, plan(3, 1, 1, 0, 0, 64, 0, 0, 1, 1, 10, 1, 0)),
    # staged behind the sort, the rocks part on the culled kernel (two launches): 8 192 envs are one rover per 44 cells -> sorted
    _case("staged-lane-rocks0-f32", "A", "37", 8192, 0, {"lane_rocks": 0}, plan(4, 0, 1, 0, 0, 32, 0, 1, 1, 1, 10, 1, 1)),
    _case("staged-lane-rocks0-shipped", "A", "37", 8192, 2, {"lane_rocks": 0}, plan(4, 1, 1, 0, 0, 32, 0, 1, 1, 1, 10, 1, 1)),
    # a 1 MiB queue holds the regions of 6 block slots per XCD; the grid of 516 096 rays in runs of 32 / 16 has 296 + 416: 119 launches
    _case("queue-1mb-culled", "A", "37", 8192, 0, {"raycast_variant": 3, "cull_queue_mb": 1}, plan(3, 0, 1, 0, 0, 32, 0, 1, 1, 119, 10, 1, 1)),
    _case("queue-1mb-staged-lane-rocks0", "A", "37", 8192, 0, {"lane_rocks": 0, "cull_queue_mb": 1}, plan(4, 0, 1, 0, 0, 32, 0, 1, 1, 119, 10, 1, 1)),
    # env_run 64 as the auto choice needs 2^20 slots in env order, i.e. more than 600 x 600 cells: reached through raycast_run
    _case("cfg1-f32-run64", "A", "37", 4096, 0, {"raycast_run": 64}, plan(4, 0, 0, 1, 1, 64, 64, 1, 1, 1, 10, 0, 0)),
    # 2 359 296 slots do not fit beside 12 low bin bits in one dword: (bin, slot) entries, the 512-thread sort tile
    _case("two-dword-entries", "A", "37", 36864, 0, {"bin_low_bits": 12}, plan(4, 0, 1, 0, 1, 64, 0, 1, 1, 1, 12, 2, 1)),
]
# env order forced: a last partial run of 16 slots (1 x 40, 63 x 72, 65 x 40, 1 000 x 72 ...), padding slots (1, 5, 1 and 6 per env), one env
for _envs in (1, 63, 65, 1000):
    for _p, _r8 in ((5, 32), (9, 40), (37, 64), (40, 72)):
        for _prec in ((0, 2) if (_envs, _p) in ((1, 9), (63, 40), (65, 5), (1000, 37)) else (0,)):
            assert (26 + _p + 7) // 8 * 8 == _r8
            PLAN_CASES.append(_case(f"env-order-e{_envs}-r8_{_r8}-{'shipped' if _prec else 'f32'}", "S", _p, _envs, _prec,
                                    {"raycast_variant": 4, "lane_env_order": 1}, plan(4, 1 if _prec else 0, 0, 1, 1, 32, 16, 0, 0, 1, 10, 0, 0)))


# ---- what the planner needs to know about a row's scene (the scenes themselves: _build_scene in test_raycast_plans_gpu.py) -----------------
# Both maps of a scene have the same cells and K.  far_bound: terrain cells with a usable far bound, as the fact the planner uses — it
# only asks whether they are at least half of the cells ("most": A, 319 586 of 360 000;
# "few": S, a K = 40 list reaches too short, and I).  The GPU test checks every entry against what an engine on the built scene
# reports, so this dict cannot drift from the scenes.
SCENE_INPUTS = {
    "A": dict(X=600, Y=600, K8=200, far_bound="most"),
    "S": dict(X=64, Y=64, K8=40, far_bound="few"),
    "I": dict(X=300, Y=300, K8=200, far_bound="few"),
}
RAYS_P = {"37": 37, "120": 120, "native": 1634}          # heightmap points of the named ray distributions (an int is its own P)


def scene_maps(scene, cells_with_far_bound=None, staged_tables=(1, 1)):
    """The ``maps`` argument of `_lib.plan_raycast` for a scene of SCENE_INPUTS (K8 <= 256: the culled kernel's tables exist); the terrain's
    far-bound count as reported by an engine, or a representative of the scene's far_bound fact."""
    s = SCENE_INPUTS[scene]
    if cells_with_far_bound is None:
        cells_with_far_bound = s["X"] * s["Y"] if s["far_bound"] == "most" else 1
    one = dict(X=s["X"], Y=s["Y"], K8=s["K8"], cells_with_far_bound=cells_with_far_bound, has_cull_tables=1, has_staged_tables=staged_tables)
    return (one, dict(one))


def planner_inputs(row, cells_with_far_bound=None):
    """keyword arguments of `_lib.plan_raycast` for a PLAN_CASES row"""
    p = row["rays"] if isinstance(row["rays"], int) else RAYS_P[row["rays"]]
    return dict(num_envs=row["envs"], maps=scene_maps(row["scene"], cells_with_far_bound), P=p, ray_precision=row["precision"], **row["options"])
