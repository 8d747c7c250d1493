"""GPU (-m gpu): every ray-cast plan the library can choose (plan_step, csrc/rover_plan.cpp) against the CPU oracle.

(a) PLAN_CASES (tests/raycast_plan_cases.py): one row per plan — the plan the library reports (`Engine.raycast_plan()`) is asserted
    field by field, which pins today's thresholds (a tuning change edits the table and says so), and the ctx-free planner
    (`_lib.plan_raycast`) must report the same plan from what the engine says about itself, which ties the CPU test of the table
    (tests/test_raycast_plan_host.py) to real engines; two fused steps on one engine, each with the device's own rays
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
from raycast_plan_cases import PLAN_CASES, PLAN_FIELDS, SCENE_INPUTS, planner_inputs

pytestmark = pytest.mark.gpu

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


def _engine_for(row, scenes):
    scene, zf, extent, maps = scenes(row["scene"])
    distn = _distribution(row["rays"])
    eng = make_engine(scene, distn, row["envs"], variant=None, **row["create"])
    if row["precision"]:
        eng.set_option("ray_precision", row["precision"])
    for name, value in row["options"].items():
        eng.set_option(name, value)
    return eng, distn


def _planner_inputs_from_engine(eng, row):
    """What `_lib.plan_raycast` takes, read back from the engine (rover_get_info, rover_get_cull_info) plus the options the row set; on
    the way, the row's SCENE_INPUTS entry is checked against what the built scene turned into."""
    info, cull = eng.info(), eng.cull_info()
    want = SCENE_INPUTS[row["scene"]]
    far, cells = cull["cells_with_far_bound"][0], info.X[0] * info.Y[0]
    for w in range(2):
        assert (info.X[w], info.Y[w], info.K8[w]) == (want["X"], want["Y"], want["K8"]), f"SCENE_INPUTS[{row['scene']!r}] is not the scene the test built"
    assert (2 * far >= cells) == (want["far_bound"] == "most"), f"SCENE_INPUTS[{row['scene']!r}]: {far} of {cells} terrain cells have a far bound"
    tabled = planner_inputs(row)
    assert (info.P, info.ray_precision) == (tabled["P"], tabled["ray_precision"])
    maps = tuple(dict(X=info.X[w], Y=info.Y[w], K8=info.K8[w], cells_with_far_bound=cull["cells_with_far_bound"][w], has_cull_tables=info.K8[w] <= 256,
                      has_staged_tables=(1, 1)) for w in range(2))          # (option "staged_tables" at its default: both proofs)
    return dict(num_envs=eng.num_envs, maps=maps, P=info.P, ray_precision=info.ray_precision, **row["options"])


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
    from isaac_rover_amd import _lib
    assert _lib.plan_raycast(**_planner_inputs_from_engine(eng, row)) == got_plan, f"{row['id']}: the ctx-free planner disagrees with the engine"
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
    # is no auto plan (plan_step: 26 + P <= 260 wherever lazy_far holds)
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
