"""GPU (-m gpu): every ray-cast plan the library can choose (plan_raycast, csrc/rover_capi.cpp) against the CPU oracle.

(a) PLAN_CASES: one row per plan — the plan the library reports (`Engine.raycast_plan()`) is asserted field by field, which pins
    today's thresholds (a tuning change edits the table and says so); two fused steps on one engine, each with the device's own rays
    through the oracle's per-ray arithmetic (`_rays_vs_oracle`: zero differing distances, every ray, both maps) and the whole step
    against `oracle.step`.
(b) the plans the rows report cover every value each plan field can take.
(c) a bounded, seeded fuzz (tests/raycast_fuzz.py, shared with tools/fuzz_shapes.py) of every kernel route against the oracle."""
import numpy as np
import pytest
import torch

from conftest import assert_step_close
from hip_helpers import _oracle_maps, _rays_vs_oracle, hip_step, make_engine
import raycast_fuzz

pytestmark = pytest.mark.gpu

PLAN_FIELDS = ("variant", "proof", "sorted", "env_order", "rocks_staged", "run", "env_run", "lazy_far", "skip_clear", "cull_launches",
               "low_bits", "sort_entry_dwords", "hist_fused")


def plan(variant, proof, sorted, env_order, rocks_staged, run, env_run, lazy_far, skip_clear, cull_launches, low_bits,
         sort_entry_dwords, hist_fused):
    return dict(zip(PLAN_FIELDS, (variant, proof, sorted, env_order, rocks_staged, run, env_run, lazy_far, skip_clear, cull_launches,
                                  low_bits, sort_entry_dwords, hist_fused)))


# ---- scenes (built once per module) ---------------------------------------------------------------------------------------------
#   A     the bench scene: regular mesh, 600 x 600 cells, K = 200 (built on the GPU)
#   S     regular, 64 x 64 cells, K = 40: the padding / partial-run shapes of the env-order launch (a K = 40 list reaches too short for a
#         far bound — one cell of 4 096 has one —, so the plan carries lazy_far 0 / skip_clear 0 as on an irregular mesh)
#   I     irregular (decimated-style) mesh of 30 m x 30 m, K = 200, maps by the library's builder: fewer than half of its cells have a
#         usable far bound
def _build_scene(name):
    from isaac_rover_amd import _lib, assets, synth
    if name == "A":
        return synth.make_scene(n_cells=600, k=200, n_stones=1024, device="cuda"), None, 60.0
    if name == "S":
        return synth.make_scene(n_cells=64, k=40, n_stones=16), None, 6.4
    assert name == "I"
    spec = synth.IrregularSpec(extent_x=30.0, extent_y=30.0, n_rocks=256, seed=6, fine=0.05)
    tool = _lib.Engine(8, device=0)
    scene, zf = assets.build_irregular_scene(tool, spec, 200)
    tool.close()
    return scene, zf, 30.0


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name):
        if name not in cache:
            scene, zf, extent = _build_scene(name)
            cache[name] = (scene, zf, extent, _oracle_maps(scene))
        return cache[name]
    return get


def _points(p, seed):
    """p heightmap points in the rover's frame (the fuzz generator's box), all in the sparse part"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0.1, 2.5, p).round(4), rng.uniform(-1.5, 1.5, p).round(4), np.full(p, -0.26878)], axis=1)
    return pts, np.arange(p, dtype=np.int64), np.arange(0, dtype=np.int64)


def _distribution(rays):
    from isaac_rover_amd import synth
    if rays == "native":
        from isaac_rover_amd.tasks.utils.heightmap_distribution import generate_native
        return tuple(np.asarray(x) for x in generate_native())
    if isinstance(rays, int):
        return _points(rays, seed=rays)
    return synth.ray_distribution(rays)


# ---- (a) the table ---------------------------------------------------------------------------------------------------------------
# (id, scene, rays, envs, precision, options in the order they are set, rover_create extras, expected plan)
# precision: 0 the f32 arithmetic, 2 the reference's as-shipped fp16 arithmetic.  options = {}: the plan is the library's auto choice.
# The expected plans are derived from plan_raycast() / plan_variant() / plan_run() / plan_env_order() / alloc_bins() / bin_hist_fused();
# r = envs x (26 + P) / 65 536 (integer division) is what plan_run() switches on.
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


def _engine_for(row, scenes):
    scene, zf, extent, maps = scenes(row["scene"])
    distn = _distribution(row["rays"])
    eng = make_engine(scene, distn, row["envs"], variant=None, **row["create"])
    if row["precision"]:
        eng.set_option("ray_precision", row["precision"])
    for name, value in row["options"].items():
        eng.set_option(name, value)
    return eng, distn


def _step_vs_oracle(eng, maps, distn, st, row, label):
    """one fused step: the ray phase on the device's own rays (zero differences), then the whole step against the oracle's"""
    from oracle import oracle as orc
    half = row["precision"] == 2
    env_offset = row["create"].get("env_offset", 0)
    n_global = row["create"].get("num_envs_global", 0) or row["envs"]
    got = hip_step(eng, st)
    src, _, _ = _rays_vs_oracle(eng, maps, half, label)
    assert src.shape[0] == row["envs"] and src.shape[1] == 26 + distn[0].shape[0], "every ray of every env went through the oracle"
    want = orc.step(*maps, st, *distn, num_envs_global=n_global, precision="fp16_as_shipped" if half else "fp32")
    g = dict(got)
    np.testing.assert_array_equal(g.pop("reset_ids"), np.nonzero(got["reset_buf"])[0] + env_offset, err_msg=f"{label}: reset_ids")
    flips = float(((got["ray_dist"] < 11.0) != (want["ray_dist"] < 11.0)).mean())
    f_reset = float((got["reset_buf"] != want["reset_buf"]).mean())
    f_coll = float((got["rock_collision"] != want["rock_collision"]).mean())
    print(f"[{label}] whole step vs the oracle: hit<->miss flips {flips:.5%}, reset flags {f_reset:.5%}, collision flags {f_coll:.5%}; "
          f"terrain hit rate {(want['ray_dist'] < 11.0).mean():.4f}")
    assert_step_close(g, {"out_" + k: v for k, v in want.items()}, label)
    np.testing.assert_array_equal(got["progress_buf"], want["progress_buf"], err_msg=f"{label}: progress_buf")
    return got


@pytest.mark.parametrize("row", PLAN_CASES)
def test_plan_case_against_the_oracle(row, scenes):
    from isaac_rover_amd import synth
    scene, zf, extent, maps = scenes(row["scene"])
    eng, distn = _engine_for(row, scenes)
    got_plan = eng.raycast_plan()
    print(f"[{row['id']}] reported plan: {got_plan}")
    assert got_plan == row["plan"], f"{row['id']}: the library reports another plan than the table expects"
    kw = {} if zf is None else dict(heightfn=zf)
    for step, seed in enumerate((31, 32)):          # the second step: other poses on the same engine
        st = synth.make_states(row["envs"], extent, seed=seed, **kw)
        _step_vs_oracle(eng, maps, distn, st, row, f"{row['id']} step {step}")
    assert eng.raycast_plan() == got_plan
    eng.close()


# ---- (b) the table covers the plan space -----------------------------------------------------------------------------------------
def _culled_kernel_runs(p):
    return p["variant"] == 3 or (p["variant"] == 4 and p["sorted"] and not p["rocks_staged"])


def _coverage_gaps(rows, plans):
    """-> what the plans of ``rows`` leave out, as a list of sentences (empty: every value of every plan field is visited)"""
    gaps = []

    def need(what, have, wanted):
        missing = set(wanted) - set(have)
        if missing:
            gaps.append(f"{what}: no row with {sorted(missing)}")

    auto = [p for r, p in zip(rows, plans) if not r["options"]]
    need("variant as the auto choice", {p["variant"] for p in auto}, {1, 2, 3, 4})
    need("proof", {p["proof"] for p in plans}, {0, 1})
    need("sorted", {p["sorted"] for p in plans if p["variant"] == 4}, {0, 1})
    need("env_order", {p["env_order"] for p in plans if p["variant"] == 4}, {0, 1})
    need("rocks_staged (variant 4, sorted)", {p["rocks_staged"] for p in plans if p["variant"] == 4 and p["sorted"]}, {0, 1})
    # plan_run's two branches for the culled kernel: the f32 arithmetic on a regular mesh (most cells have a far bound) / everything else
    first = [p for r, p in zip(rows, plans) if p["variant"] == 3 and r["precision"] != 2 and r["scene"] != "I"]
    second = [p for r, p in zip(rows, plans) if p["variant"] == 3 and (r["precision"] == 2 or r["scene"] == "I")]
    need("run of the culled kernel, first branch of plan_run", {p["run"] for p in first}, {8, 16, 32, 64})
    need("run of the culled kernel, second branch of plan_run", {p["run"] for p in second}, {8, 16, 32, 64})
    need("run of the staged kernel behind the sort", {p["run"] for p in plans if p["variant"] == 4 and p["sorted"]}, {32, 64})
    need("env_run", {p["env_run"] for p in plans if p["env_order"]}, {16, 32, 64})
    culled = [p for p in plans if _culled_kernel_runs(p)]
    for proof in (0, 1):
        need(f"lazy_far where the culled kernel runs, proof {proof}", {p["lazy_far"] for p in culled if p["proof"] == proof}, {0, 1})
        need(f"skip_clear where the culled kernel runs, proof {proof}", {p["skip_clear"] for p in culled if p["proof"] == proof}, {0, 1})
    # the six cull_scan_kernel instantiations launch_raycast_culled selects from (proof, lazy_far, skip_clear); lazy_far without skip_clear
    # is no auto plan (plan_raycast: 26 + P <= 260 wherever lazy_far holds)
    need("(proof, lazy_far, skip_clear) where the culled kernel runs", {(p["proof"], p["lazy_far"], p["skip_clear"]) for p in culled},
         {(0, 1, 1), (0, 0, 1), (0, 0, 0), (1, 1, 1), (1, 0, 1), (1, 0, 0)})
    need("cull_launches = 1", {p["cull_launches"] == 1 for p in culled}, {True})
    need("cull_launches > 1 on the culled kernel alone", {p["cull_launches"] > 1 for p in plans if p["variant"] == 3}, {True})
    need("cull_launches > 1 for the rocks part of the staged ray cast", {p["cull_launches"] > 1 for p in culled if p["variant"] == 4}, {True})
    need("sort_entry_dwords", {p["sort_entry_dwords"] for p in plans if p["sorted"]}, {1, 2})
    need("hist_fused", {p["hist_fused"] for p in plans if p["sorted"]}, {0, 1})
    need("low_bits", {p["low_bits"] for p in plans}, {10, 12})
    return gaps


def test_plan_cases_cover_the_plan_space(scenes):
    """Every value each plan field can take is visited by a row (no step needed: the plans the engines report).  A field the library
    adds to rover_raycast_plan without a rule here fails the first assertion.  Deleting a row that is the only one of its kind (the five
    named below are tried) fails the second; rows that share their field values with another row (e1024-*, e384-f32-auto, most env-order
    rows) can go without a gap: they are there for their shapes, not for the coverage.

    What the `run` / `env_run` values of the rows pin is plan_run()'s REPORTING: the run length does not enter a ray's arithmetic, so a
    library that reports run 16 and launches its waves over 32 rays gives the same bits, and no row here (nor any other test of the suite)
    fails on it — tried with a seeded mutation.  The same holds for the sort key: the kernels take map and cell from the ray record, the
    (map, cell) key only orders the list, so a rocks bin offset one cell too low changes no result and fails no test either.  The rows
    with other run lengths, and the lane_rocks 0 rows, check that those traversals compute the oracle's distances, not that the library
    launches what it reports."""
    rows = [p.values[0] for p in PLAN_CASES]
    plans = []
    for row in rows:
        eng, _ = _engine_for(row, scenes)
        plans.append(eng.raycast_plan())
        eng.close()
    for p in plans:
        assert tuple(p) == PLAN_FIELDS, "rover_raycast_plan has fields this test has no coverage rule for"
    assert _coverage_gaps(rows, plans) == []
    # the rule set has teeth: without the rows that are the only ones of their kind it reports a gap
    for only in ("irregular-shipped-auto", "two-dword-entries", "cfg1-f32-run64", "culled-regular-run8", "queue-1mb-staged-lane-rocks0"):
        keep = [i for i, r in enumerate(rows) if r["id"] != only]
        assert len(keep) == len(rows) - 1
        assert _coverage_gaps([rows[i] for i in keep], [plans[i] for i in keep]), f"the table without {only} still counts as complete"


# ---- (c) bounded, seeded fuzz against the oracle ---------------------------------------------------------------------------------
FUZZ_SEEDS = (1, 11, 23)
FUZZ_CASES_PER_SEED = 4


def _fuzz_cases():
    out = []
    for seed in FUZZ_SEEDS:
        rng = np.random.default_rng(seed)
        for c in range(FUZZ_CASES_PER_SEED):
            out.append(pytest.param(seed, c, raycast_fuzz.draw_case(rng), id=f"seed{seed}-case{c}"))
    return out


@pytest.mark.parametrize("seed,index,case", _fuzz_cases())
def test_fuzz_every_route_against_the_oracle(seed, index, case):
    """Random shapes (tests/raycast_fuzz.py), two steps per engine, a quarter of the envs in adversarial poses; for every route — the
    env-order kernel (f32 only: it has no fp16 arithmetic), binned, culled, staged behind the sort with the rocks part on either kernel,
    staged in env order — the device's own rays through the oracle: zero differing distances on every ray, both steps.  The first route
    of a step goes through `_rays_vs_oracle`; the others must export bit-identical rays (prep_rays_kernel does not depend on the
    route) and are compared, by the same rule, with the oracle's distances of those rays."""
    from isaac_rover_amd import synth
    assert max(case["k"], (case["k"] + 7) // 8 * 8) <= 256
    scene = synth.make_scene(n_cells=case["cells"], k=case["k"], n_stones=8, device="cuda")
    maps = _oracle_maps(scene)
    extent, n, prec, distn = case["cells"] * 0.1, case["envs"], case["precision"], case["distribution"]
    half = prec == 2
    print(f"[fuzz seed {seed} case {index}] {raycast_fuzz.describe(case)}")
    states, plain = [], 0
    for step in range(2):
        st = synth.make_states(n, extent, seed=100000 * seed + 1000 * index + step)
        plain = raycast_fuzz.add_adversarial_poses(st, seed=seed + step)
        states.append(st)
    first = {}          # step -> (src, dirs, cell, the oracle's distances) of the first route
    for name, variant, options in raycast_fuzz.ROUTES:
        if variant == 1 and half:
            continue
        eng = make_engine(scene, distn, n, variant=variant)
        eng.set_option("ray_precision", prec)
        for k, v in options.items():
            eng.set_option(k, v)
        p = eng.raycast_plan()
        assert p["variant"] == variant and p["proof"] == (1 if half else 0)
        if variant == 4:
            assert p["env_order"] == options["lane_env_order"] and p["rocks_staged"] == (p["env_order"] or options["lane_rocks"])
        for step, st in enumerate(states):
            label = f"fuzz seed {seed} case {index}, {name}, step {step}"
            hip_step(eng, st)
            src, dirs, cell, dist = (x.cpu().numpy() for x in eng.export_rays())
            assert dist.shape == (n, 26 + case["points"]), "every ray of every env"
            if step not in first:
                _, _, want = _rays_vs_oracle(eng, maps, half, label)       # (the oracle runs once per step)
                # the rovers make_states placed mostly see the terrain, in the oracle
                rate = float((want[:plain, 26:] < 11.0).mean())
                assert 0.3 < rate <= 1.0, f"{label}: terrain hit rate {rate:.4f} of the plain envs in the oracle"
                first[step] = (src, dirs, cell, want)
                continue
            src0, dirs0, cell0, want = first[step]
            for a, b, what in ((src, src0, "origins"), (dirs, dirs0, "directions")):
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{label}: ray {what} differ from the first route's")
            np.testing.assert_array_equal(cell, cell0, err_msg=f"{label}: ray cells differ from the first route's")
            differ = ~((dist == want) | (np.isnan(dist) & np.isnan(want)))
            print(f"[{label}] ray phase on the device's own rays vs the oracle: {int(differ.sum())} of {dist.size} distances differ")
            for e, sl in list(zip(*np.nonzero(differ)))[:8]:
                print(f"   env {e} slot {sl}: src {src[e, sl].tolist()} dir {dirs[e, sl].tolist()} cell {cell[e, sl]}: device {dist[e, sl]!r} oracle {want[e, sl]!r}")
            assert not differ.any(), f"{label}: {int(differ.sum())} of {dist.size} ray distances differ from the oracle on IDENTICAL rays"
        eng.close()
