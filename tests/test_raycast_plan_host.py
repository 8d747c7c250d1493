"""CPU: the ray-cast planner (plan_step, csrc/rover_plan.cpp) through its ctx-free query `_lib.plan_raycast` — no device.

(a) every row of the plan table (tests/raycast_plan_cases.py): the planner gives the row's expected plan from the row's scene inputs.
    tests/test_raycast_plans_gpu.py asserts the same rows on real engines, and that the query agrees with each engine.
(b) both sides of every threshold in plan_step, the expected values written out by hand from the rule each comment states."""
import pytest

from isaac_rover_amd import _lib
from raycast_plan_cases import PLAN_CASES, PLAN_FIELDS, planner_inputs


@pytest.mark.parametrize("row", PLAN_CASES)
def test_plan_table_row_on_the_cpu(row):
    got = _lib.plan_raycast(**planner_inputs(row))
    assert tuple(got) == PLAN_FIELDS
    assert got == row["plan"], f"{row['id']}: plan_step gives another plan than the table expects"


def grid(n, k8=200, far="all", staged=(1, 1)):
    """both maps n x n cells; far: terrain cells with a far bound ("all", or a count)"""
    one = dict(X=n, Y=n, K8=k8, cells_with_far_bound=n * n if far == "all" else far, has_cull_tables=k8 <= 256, has_staged_tables=staged)
    return (one, dict(one))


A = grid(600)                      # the bench scene's shape: 360 000 cells, every one with a far bound
NO_STAGED = grid(600, staged=(0, 0))
IRREGULAR = grid(600, far=1000)    # fewer than half of the cells with a far bound
SHIPPED = dict(ray_precision=2)
CULLED = dict(raycast_variant=3)
ENV_ORDER = dict(raycast_variant=4, lane_env_order=1)

# (what, envs, P, maps, options, the plan fields the threshold decides).  rays = envs x (26 + P); P = 38 makes 64 rays and 64 slots per env,
# so envs = r x 1 024 is the first batch with rays // 65 536 = r.
SWITCH_POINTS = [
    # ---- which kernel ----
    ("f32: 24 575 rays -> env-order kernel", 25, 957, A, {}, dict(variant=1, sorted=0, cull_launches=0)),
    ("f32: 24 576 rays -> staged", 384, 38, A, {}, dict(variant=4, env_order=1, sorted=0)),
    ("f32, no staged tables: 24 576 rays -> still the env-order kernel", 384, 38, NO_STAGED, {}, dict(variant=1)),
    ("f32, no staged tables: 49 152 rays -> env-order kernel", 768, 38, NO_STAGED, {}, dict(variant=1)),
    ("f32, no staged tables: 49 153 rays -> culled", 247, 173, NO_STAGED, {}, dict(variant=3, sorted=1)),
    ("as shipped: 24 576 rays -> binned", 384, 38, A, SHIPPED, dict(variant=2, proof=1, sorted=1, cull_launches=0)),
    ("as shipped: 24 577 rays -> staged in env order", 7, 3485, A, SHIPPED, dict(variant=4, proof=1, env_order=1, sorted=0)),
    ("as shipped: 98 303 rays -> staged in env order", 197, 473, A, SHIPPED, dict(variant=4, env_order=1, sorted=0)),
    ("as shipped: 98 304 rays, regular mesh -> staged behind the sort", 1536, 38, A, SHIPPED, dict(variant=4, env_order=0, sorted=1)),
    ("as shipped: 98 303 rays, irregular mesh -> staged in env order", 197, 473, IRREGULAR, SHIPPED, dict(variant=4, env_order=1)),
    ("as shipped: 98 304 rays, irregular mesh, 0.16 rays per cell -> culled", 1536, 38, IRREGULAR, SHIPPED, dict(variant=3, sorted=1)),
    # E P against 2 cells on a mesh with few far bounds (128 x 128 = 16 384 cells), as shipped, beyond 98 304 rays
    ("as shipped, irregular: E P = 2 cells -> staged", 4096, 8, grid(128, far=100), SHIPPED, dict(variant=4, sorted=1)),
    ("as shipped, irregular: E P < 2 cells -> culled", 4096, 7, grid(128, far=100), SHIPPED, dict(variant=3, sorted=1)),
    # 2 farok against cells, everything else as in the row above
    ("as shipped: half of the cells with a far bound -> regular -> staged", 4096, 7, grid(128, far=8192), SHIPPED, dict(variant=4, skip_clear=1)),
    ("as shipped: one cell fewer -> irregular -> culled, eager, no skip", 4096, 7, grid(128, far=8191), SHIPPED, dict(variant=3, skip_clear=0, lazy_far=0)),
    # K8 = 256 is the widest list the binned / culled / staged kernels hold (64 lanes x 4 triangles)
    ("K8 = 256: the variant asked for runs", 4096, 38, grid(600, k8=256), CULLED, dict(variant=3)),
    ("K8 = 264: every variant runs as the env-order kernel", 4096, 38, grid(600, k8=264), CULLED, dict(variant=1, sorted=0)),
    # ---- env order or sort (f32; 512 x 512 = 262 144 cells) ----
    ("2 E P < 3 cells -> env order", 3072, 127, grid(512), {}, dict(variant=4, env_order=1, sorted=0, rocks_staged=1)),
    ("2 E P = 3 cells -> sorted", 3072, 128, grid(512), {}, dict(variant=4, env_order=0, sorted=1)),
    ("64 E < cells -> env order", 4095, 37, grid(512), {}, dict(variant=4, env_order=1, sorted=0)),
    ("64 E = cells -> sorted", 4096, 37, grid(512), {}, dict(variant=4, env_order=0, sorted=1)),
    # ---- rays per wave behind the sort ----
    ("culled, regular f32: r = 2 -> 8", 3071, 38, A, CULLED, dict(variant=3, run=8)),
    ("culled, regular f32: r = 3 -> 16", 3072, 38, A, CULLED, dict(variant=3, run=16)),
    ("culled, regular f32: r = 5 -> 16", 6143, 38, A, CULLED, dict(run=16)),
    ("culled, regular f32: r = 6 -> 32", 6144, 38, A, CULLED, dict(run=32)),
    ("culled, regular f32: r = 19 -> 32", 20479, 38, A, CULLED, dict(run=32)),
    ("culled, regular f32: r = 20 -> 64", 20480, 38, A, CULLED, dict(run=64)),
    ("culled, irregular: r = 11 -> 8", 12287, 38, IRREGULAR, CULLED, dict(variant=3, run=8)),
    ("culled, irregular: r = 12 -> 16", 12288, 38, IRREGULAR, CULLED, dict(run=16)),
    ("culled, irregular: r = 23 -> 16", 24575, 38, IRREGULAR, CULLED, dict(run=16)),
    ("culled, irregular: r = 24 -> 32", 24576, 38, IRREGULAR, CULLED, dict(run=32)),
    ("culled, irregular: r = 47 -> 32", 49151, 38, IRREGULAR, CULLED, dict(run=32)),
    ("culled, irregular: r = 48 -> 64", 49152, 38, IRREGULAR, CULLED, dict(run=64)),
    ("culled, as shipped on the regular mesh: the later table, r = 11 -> 8", 12287, 38, A, dict(CULLED, **SHIPPED), dict(variant=3, run=8)),
    ("culled, as shipped on the regular mesh: r = 12 -> 16", 12288, 38, A, dict(CULLED, **SHIPPED), dict(variant=3, run=16)),
    ("staged behind the sort: r = 11 -> 32", 12287, 38, A, {}, dict(variant=4, sorted=1, run=32)),
    ("staged behind the sort: r = 12 -> 64", 12288, 38, A, {}, dict(variant=4, sorted=1, run=64)),
    ("binned: r clamped to 4 from below", 1024, 38, A, dict(raycast_variant=2), dict(variant=2, run=4)),
    ("binned: r = 5", 5120, 38, A, dict(raycast_variant=2), dict(run=5)),
    ("binned: r clamped to 32 from above", 40960, 38, A, dict(raycast_variant=2), dict(run=32)),
    # ---- slots per wave in env order (64 slots per env) ----
    ("env order: 2^17 - 64 slots -> 16", 2047, 38, A, ENV_ORDER, dict(env_order=1, env_run=16, run=32)),
    ("env order: 2^17 slots -> 32", 2048, 38, A, ENV_ORDER, dict(env_run=32)),
    ("env order: 2^20 - 64 slots -> 32", 16383, 38, A, ENV_ORDER, dict(env_run=32)),
    ("env order: 2^20 slots -> 64", 16384, 38, A, ENV_ORDER, dict(env_run=64)),
    ("env order: raycast_run caps at 64", 2048, 38, A, dict(ENV_ORDER, raycast_run=100), dict(env_run=64, run=100)),
    # ---- the culled kernel's far records and whole-cell skip (64 x 64 = 4 096 cells, all with a far bound) ----
    ("99 rays per env: far records on demand at any density", 1024, 73, grid(64), CULLED, dict(lazy_far=1, skip_clear=1)),
    ("100 rays per env, 18 heightmap rays per cell: eager", 1024, 74, grid(64), CULLED, dict(lazy_far=0, skip_clear=1)),
    ("E P < 8 cells: on demand", 255, 128, grid(64), CULLED, dict(lazy_far=1, skip_clear=1)),
    ("E P = 8 cells: eager", 256, 128, grid(64), CULLED, dict(lazy_far=0, skip_clear=1)),
    ("260 rays per env: rays that clear their cell are skipped", 64, 234, A, CULLED, dict(lazy_far=1, skip_clear=1)),
    ("261 rays per env: no skip (f32: on demand stays)", 64, 235, A, CULLED, dict(lazy_far=1, skip_clear=0)),
    ("261 rays per env, as shipped: without the skip the eager kernel", 64, 235, A, dict(CULLED, **SHIPPED), dict(lazy_far=0, skip_clear=0)),
    ("P = 260: still a sparse set where E P < 8 cells", 64, 260, A, CULLED, dict(lazy_far=1, skip_clear=0)),
    ("P = 261: dense whatever the batch", 64, 261, A, CULLED, dict(lazy_far=0, skip_clear=0)),
    ("few far bounds: eager, no skip", 64, 37, IRREGULAR, CULLED, dict(lazy_far=0, skip_clear=0)),
    ("ROVER_CULL_LAZY 0 overrides the auto choice", 1024, 73, grid(64), dict(CULLED, cull_lazy=0), dict(lazy_far=0, skip_clear=1)),
    # ---- the sort's digit and entry width (720 000 bins at 600 x 600; 64 slots per env) ----
    ("2^22 slots fit beside 10 low bits", 65536, 38, A, {}, dict(sorted=1, low_bits=10, sort_entry_dwords=1)),
    ("2^22 + 64 slots: 9 low bits (1 407 buckets) keep the entry in one dword", 65537, 38, A, {}, dict(sorted=1, low_bits=9, sort_entry_dwords=1)),
    ("... bin_low_bits 10 by name: two dwords", 65537, 38, A, dict(bin_low_bits=10), dict(low_bits=10, sort_entry_dwords=2)),
    ("... 2 420 000 bins: 9 low bits would be 4 727 buckets -> 10 stay, two dwords", 65537, 38, grid(1100), {}, dict(sorted=1, low_bits=10, sort_entry_dwords=2)),
    ("4 500 000 bins: 10 low bits would be 4 395 buckets -> 11; 2^21 slots fit beside them", 32768, 38, grid(1500), CULLED, dict(sorted=1, low_bits=11, sort_entry_dwords=1)),
    ("... 2^21 + 64 slots do not, and fewer low bits are too many buckets: two dwords", 32769, 38, grid(1500), CULLED, dict(low_bits=11, sort_entry_dwords=2)),
    # ---- the big sort tile from 2 M slots: 16 384 slots hold the 64 x 128 keys of a prep block, 4 096 do not (P = 102: 128 slots per env) ----
    ("2^21 - 128 slots: small tile, histogram not fused", 16383, 102, A, {}, dict(sorted=1, run=64, hist_fused=0)),
    ("2^21 slots: big tile, histogram fused", 16384, 102, A, {}, dict(sorted=1, run=64, hist_fused=1)),
    # ---- nothing to plan yet ----
    ("no distribution: the culled kernel by default, no queue, no sort entry", 4096, 0, A, {}, dict(variant=3, sorted=1, cull_launches=0, sort_entry_dwords=0)),
]


@pytest.mark.parametrize("what,envs,P,maps,options,expect", SWITCH_POINTS, ids=[s[0] for s in SWITCH_POINTS])
def test_plan_at_switch_points(what, envs, P, maps, options, expect):
    got = _lib.plan_raycast(envs, maps, P=P, **options)
    assert {k: got[k] for k in expect} == expect, f"{what}: envs {envs}, P {P}, {envs * (26 + P)} rays -> {got}"


def test_plan_without_maps_and_refusals():
    assert _lib.plan_raycast(4096, (None, None), P=37)["variant"] == 0
    assert _lib.plan_raycast(4096, (A[0], None), P=37)["variant"] == 0
    for bad in (dict(raycast_variant=5), dict(raycast_run=4097), dict(bin_low_bits=7), dict(lane_env_order=2), dict(cull_queue_mb=0),
                dict(ray_precision=3)):
        with pytest.raises(_lib.RoverError, match=next(iter(bad))):
            _lib.plan_raycast(4096, A, P=37, **bad)
    with pytest.raises(_lib.RoverError, match="num_envs"):
        _lib.plan_raycast(0, A, P=37)
