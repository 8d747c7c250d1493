"""GPU: the reset path of csrc/rover_reset.hip (clearance_kernel, collides_grid of csrc/rover_stones.h, shift_spawns_kernel, goals_draw_kernel,
goals_env0_kernel, reset_envs_kernel and the stone grid of rover_set_stones) at its own dispatch edges, against the float64 restatement
and the seeded, decided cases of tests/reset_ref.py (checked on the CPU by tests/test_reset_path_host.py), the C oracle and the host
Philox.  Two tolerances: the derived float32 bound of one clearance evaluation, and the project's 1e-5 (goal xy) / 1e-6 (yaw quaternion);
every decision (collides or not, steps walked, draws used) is compared exactly."""
import functools

import numpy as np
import pytest
import torch

import reset_ref as R
from conftest import load_golden, scene_for

pytestmark = pytest.mark.gpu
E = 2304
OFFSET = 5000
FILL = 12345.0              # what an output holds before a call: a row the call must not write keeps it
MAX_DRAWS = (1, 7, 8, 9, 63, 64, 65, 130)
RANDOM_GOAL_CASES = ((1, "first"), (1, "absent"), (31, "first"), (32, "last"), (33, "absent"), (1023, "last"), (1024, "absent"),
                     (1025, "first"), (2304, "last"), (2304, "first"))
STEP_MARGINS = (0.0, 0.37, 1.0, 1.4)
GRID_SETS = ("clusters", "big", "negative", "one_point", "empty", "nan")


@pytest.fixture(scope="module")
def engines():
    """One small engine on the reset_path golden scene (and its twin as the shard at env_offset 5000; a 257-env one for the step)."""
    from hip_helpers import make_engine
    from isaac_rover_amd import _lib, synth
    fx = load_golden("reset_path")
    scene = scene_for(fx)
    distn = synth.ray_distribution("9")
    made = {0: _lib.Engine(E, device=0), OFFSET: _lib.Engine(E, device=0, num_envs_global=OFFSET + E, env_offset=OFFSET)}
    for e in made.values():
        e.set_scene(scene, distn)
    made["step"] = make_engine(scene, distn, 257)
    yield made
    for e in made.values():
        e.close()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))                   # a copy: the cases are read-only
    return (t if dtype is None else t.to(dtype)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def clearance_case(S):
    return R.clearance_case(S)


@functools.lru_cache(maxsize=None)
def grid_sets():
    return R.grid_stone_sets()


@functools.lru_cache(maxsize=None)
def random_goal_case(n, env0):
    c = R.random_goal_case(n, env0)
    return c, R.goals64(c["info"], c["ids"], c["initial"], c["draws"], c["radius"])


@functools.lru_cache(maxsize=None)
def scheduled(T):
    return {k: (c, R.goals64(c["info"], c["ids"], c["initial"], c["draws"], c["radius"])) for k, c in R.scheduled_cases(T).items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# clearance value
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (0, 1, 1023, 1024, 1025, 2049, 3000))
def test_clearance_value_at_the_tile_edges(engines, S):
    """S around the 1024-stone tile x n around the 256-thread block, every output against float64 within 8 * 2^-24 * (dist + |r|).  The
    last rows of each launch (its partial block) sit next to stone 0, 1023, 1024, S - 1 and the last stone of each tile, at least 0.5 m
    ahead of the runner-up: a dropped or shifted tile changes their answer by far more than the bound."""
    from oracle import oracle as orc
    eng = engines[0]
    c = clearance_case(S)
    eng.set_stones(c["info"])
    k = len(c["dedicated"])
    rows = [np.arange(1000 - n, 1000) for n in (255, 256, 257, 1000)] + [np.array([r]) for r in [0] + list(range(1000 - k, 1000))]
    for sel in rows:
        xy = c["xy"][sel]
        got = eng.clearance(dev(xy)).cpu().numpy()
        assert got.shape == (len(sel),) and got.dtype == np.float32
        if S == 0:
            assert np.isposinf(got).all()
            continue
        err = np.abs(got.astype(np.float64) - c["want"][sel])
        same = int((got.view(np.uint32) == orc.clearance(c["info"], xy).view(np.uint32)).sum())
        print(f"clearance S={S} n={len(sel)}: max err / bound = {float((err / c['tol'][sel]).max()):.3f}, "
              f"bit-equal to the C oracle on {same} of {len(sel)}")
        assert (err <= c["tol"][sel]).all(), f"S={S} n={len(sel)}: rows {sel[np.nonzero(err > c['tol'][sel])[0][:8]]}"


@pytest.mark.parametrize("where", ((3, 0), (1023, 1), (1024, 6), (2048, 0)))
def test_clearance_of_a_nan_stone_is_nan_for_every_query(engines, where):
    """torch.min propagates NaN (rover.py:538): one NaN stone among finite ones, in any tile and any of x, y, r, makes every query NaN —
    as the C oracle and the stone grid (nothing collides) already have it."""
    from oracle import oracle as orc
    eng = engines[0]
    c = clearance_case(2049)
    info = c["info"].copy()
    info[where[0], where[1]] = np.nan
    eng.set_stones(info)
    for n in (1, 257, 1000):
        xy = c["xy"][1000 - n:]
        assert np.isnan(R.clearance64(info, xy)).all() and np.isnan(orc.clearance(info, xy)).all()
        got = eng.clearance(dev(xy)).cpu().numpy()
        assert np.isnan(got).all(), f"{int((~np.isnan(got)).sum())} of {n} queries are not NaN"
    pos = np.concatenate((c["xy"], np.full((1000, 1), FILL, np.float32)), axis=1)
    np.testing.assert_array_equal(eng.shift_spawns(dev(pos)).cpu().numpy(), pos)          # and nothing collides


# ---------------------------------------------------------------------------------------------------------------------------------
# the grid decision
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_SETS)
def test_grid_decision_at_1_4(engines, name):
    """Probe: shift_spawns(max_iter=1) advances x by exactly one float32 0.05f if and only if collides64(..., 1.4).  Cell lists of 1, 3,
    4, 5, 8 and 9 stones in which only the last one is within reach, a 5 m stone over many cells, negative coordinates, coincident
    stones, no stones, a NaN stone; queries on cell corners, outside the grid, and NaN / inf (x stays what it was, nothing faults)."""
    eng = engines[0]
    info = grid_sets()[name]
    eng.set_stones(info)
    xy = np.concatenate((R.grid_queries(name, info), R.NONFINITE_XY))
    hit, margin = R.collides64(info, xy, R.THR_SPAWN)
    assert (margin >= R.MARGIN).all()
    pos = np.concatenate((xy, np.full((len(xy), 1), FILL, np.float32)), axis=1)
    want = pos.copy()
    want[hit, 0] = pos[hit, 0] + R.STEP_X
    got = eng.shift_spawns(dev(pos), max_iter=1).cpu().numpy()
    print(f"grid {name}: {len(xy)} queries, {int(hit.sum())} collide")
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", GRID_SETS)
def test_step_stone_mask_equals_collides64(engines, name):
    """The same stone sets and positions through the step's stone_collision mask, for margins 0, 0.37, 1.0 and 1.4, at 257 envs."""
    from hip_helpers import hip_step
    from isaac_rover_amd import synth
    eng = engines["step"]
    info = grid_sets()[name]
    eng.set_stones(info)
    margins = [float(np.float32(m)) for m in STEP_MARGINS]
    xy = R.grid_queries(name, info, thr=tuple(margins))
    n = eng.num_envs
    st = synth.make_states(n, 12.8, seed=3)
    for lo in range(0, len(xy), n):
        chunk = xy[lo:lo + n]
        rows = np.concatenate((chunk, xy[: n - len(chunk)]))            # the last chunk is filled up with the first rows
        st["pos"][:, 0:2] = torch.from_numpy(rows.copy())
        for m in margins:
            hit, margin = R.collides64(info, rows, m)
            assert (margin >= R.MARGIN).all()
            got = hip_step(eng, st, stone_margin=m)["stone_collision"]
            assert set(np.unique(got)) <= {0, 1}
            np.testing.assert_array_equal(got != 0, hit, err_msg=f"{name} margin {m} rows {lo}..")


# ---------------------------------------------------------------------------------------------------------------------------------
# spawn walks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_stones", (1, 2, 3))
def test_spawn_walks_equal_the_sequential_walk(engines, n_stones):
    """Walks past 1, 2 and 3 stones in sequence, cut at max_iter in {0, 1, 3, 100000}: the final x bit for bit (the same decisions, the
    same float32 sums), y and z untouched; 257 spawns, and the longest walk alone."""
    eng = engines[0]
    c = R.walk_case(257, n_stones)
    eng.set_stones(c["info"])
    longest = int(c["steps"].argmax())
    for sel in (np.arange(257), np.array([longest])):
        pos = c["pos"][sel]
        for max_iter in (0, 1, 3, 100000):
            x, steps, margin = R.walk_spawn(c["info"], pos, max_iter)
            assert (margin >= R.MARGIN).all() and (steps == np.minimum(c["steps"][sel], max_iter)).all()
            want = pos.copy()
            want[:, 0] = x
            got = eng.shift_spawns(dev(pos), max_iter=max_iter).cpu().numpy()
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"max_iter {max_iter}")


# ---------------------------------------------------------------------------------------------------------------------------------
# goals from supplied draws
# ---------------------------------------------------------------------------------------------------------------------------------
def run_goals(eng, c, via_reset=False):
    """generate_goals (local ids), or the same through reset_envs on a shard (global ids = local + env_offset) -> target [E,3], used."""
    eng.set_stones(c["info"])
    target = torch.full((E, 3), FILL, device="cuda:0")
    used = torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
    initial, draws, n = dev(c["initial"]), dev(c["draws"]), len(c["ids"])
    if not via_reset:
        eng.generate_goals(dev(c["ids"]), initial, target, radius=c["radius"], draws=draws, n_draws_used=used)
    else:
        ids = np.full(E, eng.cfg.env_offset, np.int64)
        ids[:n] = c["ids"] + eng.cfg.env_offset
        pos, quat = torch.zeros(E, 3, device="cuda:0"), torch.zeros(E, 4, device="cuda:0")
        reset, progress = torch.ones(E, dtype=torch.int64, device="cuda:0"), torch.ones(E, dtype=torch.int64, device="cuda:0")
        eng.reset_envs(dev(ids), initial, pos, quat, reset, progress, n_reset_host=n, target3=target, radius=c["radius"], draws=draws,
                       n_draws_used=used)
    torch.cuda.synchronize()
    return target, int(used.item())


def check_goals(eng, c, ref, target, used, label):
    assert ref["margin"] >= R.MARGIN
    assert used == ref["used"], f"{label}: draws used {used}, the sequential loop uses {ref['used']}"
    got = target.cpu().numpy()
    ids = c["ids"]
    wrote = ~np.isnan(ref["target"][:, 0])
    wrote[ids] = True
    untouched = ~wrote
    np.testing.assert_array_equal(got[untouched], np.full((int(untouched.sum()), 3), FILL, np.float32), err_msg=label)
    if used < 0:
        return                                  # the draws ran out: the target values are unspecified
    wrote = ~np.isnan(ref["target"][:, 0])
    assert wrote[ids].all()
    np.testing.assert_allclose(got[wrote, 0:2], ref["target"][wrote], rtol=0, atol=1e-5, err_msg=label)
    # z = the heightfield at the written xy for the listed envs (set_targets rover.py:581-583); env 0's only if it was listed
    z = eng.sample_height(target[dev(ids)][:, 0:2].contiguous()).cpu().numpy()
    np.testing.assert_array_equal(got[ids, 2].view(np.uint32), z.view(np.uint32), err_msg=label)
    if 0 not in ids:
        assert got[0, 2] == FILL, label


@pytest.mark.parametrize("n,env0", RANDOM_GOAL_CASES)
def test_goals_random_stones_equal_the_sequential_loop(engines, n, env0):
    c, ref = random_goal_case(n, env0)
    target, used = run_goals(engines[0], c)
    print(f"goals n={n} env0={env0}: used {used}, tmax {ref['tmax']}, lz {ref['lz']}")
    check_goals(engines[0], c, ref, target, used, f"n={n} {env0}")


@pytest.mark.parametrize("T", MAX_DRAWS)
def test_goals_scheduled_cases_equal_the_sequential_loop(engines, T):
    """Prescribed first-clear indices around the 8-lane and 64-lane trips, an entry that never clears (used == -1), env 0 clearing only
    in the second 64-draw trip of its replay, env 0 running out of draws, no writer for env 0, only the zero id."""
    eng = engines[0]
    cases = scheduled(T)
    order = [k for k in cases if k != "never"] + ["never"]      # "never" after runs that end: its work list holds an earlier run's entries
    for name in order:
        c, ref = cases[name]
        target, used = run_goals(eng, c)
        print(f"scheduled T={T} {name}: used {used}, tmax {ref['tmax']}, lz {ref['lz']}, env-0 trips {ref['env0_trips']}")
        check_goals(eng, c, ref, target, used, f"T={T} {name}")
    # an entry that never clears, straight after a run over the same entries in which every entry clears at once
    c, ref = cases["never"]
    easy = dict(c, draws=np.full_like(c["draws"], 0.5))
    assert run_goals(eng, easy)[1] == 1
    assert run_goals(eng, c)[1] == -1


@pytest.mark.parametrize("T", (9, 65, 130))
def test_goals_through_reset_envs_on_a_shard(engines, T):
    """The same cases through reset_envs(n_reset_host=, draws=) on the shard at env_offset 5000: ids are global, results equal after the
    shift (bit for bit where the run ends)."""
    cases = dict(scheduled(T))
    cases["random"] = random_goal_case(1025, "first")
    for name, (c, ref) in cases.items():
        target, used = run_goals(engines[OFFSET], c, via_reset=True)
        check_goals(engines[OFFSET], c, ref, target, used, f"shard T={T} {name}")
        if used > 0:
            plain, used0 = run_goals(engines[0], c)
            assert used0 == used and torch.equal(plain, target), name


# ---------------------------------------------------------------------------------------------------------------------------------
# goals and yaw from the library's Philox
# ---------------------------------------------------------------------------------------------------------------------------------
PHILOX_T = 64


@functools.lru_cache(maxsize=None)
def philox_case():
    c = dict(R.random_goal_case(120, "first"))
    return c


@functools.lru_cache(maxsize=None)
def philox_draws(seed, offset):
    return R.philox_draws(seed, PHILOX_T, philox_case()["ids"] + offset)


def reset_call(eng, ids_local, target, used, **kw):
    ids = np.full(E, eng.cfg.env_offset, np.int64)
    ids[:len(ids_local)] = ids_local + eng.cfg.env_offset
    c = philox_case()
    pos, quat = torch.zeros(E, 3, device="cuda:0"), torch.zeros(E, 4, device="cuda:0")
    reset, progress = torch.ones(E, dtype=torch.int64, device="cuda:0"), torch.ones(E, dtype=torch.int64, device="cuda:0")
    eng.reset_envs(dev(ids), dev(c["initial"]), pos, quat, reset, progress, target3=target, radius=c["radius"], n_draws_used=used, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("offset", (0, OFFSET))
@pytest.mark.parametrize("seed", (1234, 2 ** 40 + 7))
def test_philox_goals_equal_host_philox_draws(engines, seed, offset):
    """generate_goals(seed=s) and reset_envs(seed=s, seed_dev=[5]) against the same calls fed with draws= built on the host from
    rover_philox4x32 — counter {global id, t, 0, 0}, key {seed lo, seed hi} —: the same device arithmetic on the same uniforms, so
    targets and draws used are equal bit for bit.  Seeds below and above 2^32, shards at env_offset 0 and 5000."""
    eng = engines[offset]
    c = philox_case()
    eng.set_stones(c["info"])
    n = len(c["ids"])
    initial = dev(c["initial"])

    def fresh():
        return torch.full((E, 3), FILL, device="cuda:0"), torch.full((1,), -7, dtype=torch.int32, device="cuda:0")

    # generate_goals takes local ids and keys the draw by the id it is given
    ta, ua = fresh()
    eng.generate_goals(dev(c["ids"]), initial, ta, radius=c["radius"], seed=seed, max_draws=PHILOX_T, n_draws_used=ua)
    tb, ub = fresh()
    eng.generate_goals(dev(c["ids"]), initial, tb, radius=c["radius"], draws=dev(philox_draws(seed, 0)), n_draws_used=ub)
    torch.cuda.synchronize()
    print(f"philox generate_goals seed={seed} offset={offset}: used {int(ua.item())}")
    assert int(ua.item()) == int(ub.item()) and int(ua.item()) > 1
    assert torch.equal(ta, tb)
    # reset_envs: global ids, the seed is host seed + *seed_dev, the count comes from the device
    ta, ua = fresh()
    reset_call(eng, c["ids"], ta, ua, n_reset_dev=torch.tensor([n], dtype=torch.int32, device="cuda:0"), seed=seed, max_draws=PHILOX_T,
               seed_dev=torch.tensor([5], dtype=torch.int64, device="cuda:0"))
    tb, ub = fresh()
    reset_call(eng, c["ids"], tb, ub, n_reset_host=n, draws=dev(philox_draws(seed + 5, offset)))
    print(f"philox reset_envs seed={seed}+5 offset={offset}: used {int(ua.item())}")
    assert int(ua.item()) == int(ub.item()) and int(ua.item()) > 1
    assert torch.equal(ta, tb)


@pytest.mark.parametrize("offset,count,seed,seed_dev", ((OFFSET, 255, R.YAW_SEED, None), (OFFSET, 256, R.YAW_SEED - 5, 5),
                                                        (OFFSET, 257, R.YAW_SEED, None), (0, 257, 2 ** 40 + 7, 5)))
def test_reset_envs_yaw_and_state(engines, offset, count, seed, seed_dev):
    """The yaw of every listed env is the host's integer floor(f32(u) * f32(361)) of (seed ^ 0x9E37..., global id) — 0 and 360 included
    —, q = (sin(h), 0, 0, cos(h)) to 1e-6; pose = initial pose, joints, reset and progress zeroed for the listed ids and untouched
    elsewhere; the count (255, 256, 257: around one block) is read from n_reset_dev."""
    eng = engines[offset]
    gids = R.YAW_IDS + offset
    ids = np.full(E, offset, np.int64)
    ids[:len(gids)] = gids
    rng = np.random.default_rng(5)
    initial = rng.uniform(1, 11, (E, 3)).astype(np.float32)
    f = dict(device="cuda:0")
    pos, base, quat = torch.full((E, 3), FILL, **f), torch.full((E, 3), FILL, **f), torch.full((E, 4), FILL, **f)
    jp, jv = torch.full((E, 13), FILL, **f), torch.full((E, 13), FILL, **f)
    reset, progress = torch.full((E,), 3, dtype=torch.int64, **f), torch.full((E,), 7, dtype=torch.int64, **f)
    eng.reset_envs(dev(ids), dev(initial), pos, quat, reset, progress, n_reset_dev=torch.tensor([count], dtype=torch.int32, **f),
                   joint_pos13=jp, joint_vel13=jv, base_pos3=base, seed=seed,
                   seed_dev=None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int64, **f))
    torch.cuda.synchronize()
    listed = R.YAW_IDS[:count]
    want = R.philox_yaw_deg(seed + (seed_dev or 0), gids[:count])
    if offset == OFFSET:
        assert want.min() == 0 and want.max() == 360
    q = quat.cpu().numpy()
    deg = np.round(np.degrees(2.0 * np.arctan2(q[listed, 0].astype(np.float64), q[listed, 3].astype(np.float64)))).astype(np.int64) % 720
    np.testing.assert_array_equal(deg, want)
    h = np.radians(want.astype(np.float64)) / 2
    np.testing.assert_allclose(q[listed], np.stack((np.sin(h), 0 * h, 0 * h, np.cos(h)), axis=1), rtol=0, atol=1e-6)
    other = np.ones(E, bool)
    other[listed] = False
    for t in (pos, base):
        np.testing.assert_array_equal(t.cpu().numpy()[listed], initial[listed])
    for t, fill in ((pos, FILL), (base, FILL), (quat, FILL), (jp, FILL), (jv, FILL), (reset, 3), (progress, 7)):
        a = t.cpu().numpy()
        assert (a[other] == fill).all()
        if t is not pos and t is not base and t is not quat:
            assert (a[listed] == 0).all()
