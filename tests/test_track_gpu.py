"""GPU: rover_episode_track (csrc/rover_track.hip) and learning/tracking.py:EpisodeTracker against the numpy restatement of the
definition (tests/track_ref.py).  After EVERY call the per-env state, the ring's valid slots, ring_count, every integer and every
float32 minimum / maximum must have the restatement's bits, and every f64 sum must lie within the any-order bound n * 2^-53 * sum|x| of
the correctly rounded sum (track_ref.py's docstring derives it, and what a window mean adds to it).  Nothing is left out of a comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import track_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BIG_INT = 65536 * 3000              # the size of the reference's collision_penalty sums


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    yield e
    e.close()


def tracker(eng, e, w=100, names=()):
    from isaac_rover_amd.learning.tracking import EpisodeTracker
    return EpisodeTracker(eng, e, window=w, components=names)


def bits(x):
    return np.atleast_1d(np.asarray(x, dtype=np.float32)).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def columns(rng, e, kinds):
    """One column per entry of ``kinds``: 'f' float32 in [0, 3), 'i' int64 in [0, 5), 'I' int64 up to 65 536 * 3 000."""
    out = []
    for k in kinds:
        if k == "f":
            out.append(rng.uniform(0, 3, e).astype(F))
        else:
            out.append(rng.integers(0, 5 if k == "i" else BIG_INT, e).astype(np.int64))
    return tuple(out)


def feed(tr, ref, rewards, done, cols=()):
    """One call on both sides -> the restatement's snapshot."""
    tr.step(dev(rewards), dev(done), {n: dev(c) for n, c in zip(tr.components, cols)})
    return ref.call(rewards, done, cols)


def state_bytes(tr):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in (tr.cum_reward, tr.cum_steps, tr.ring_ret, tr.ring_len, tr.ring_count, tr.record)]


def compare(tr, snapshot, what):
    """The tracker's whole state and record against the restatement's snapshot."""
    st, rec, bounds = snapshot
    got = tr.read(reset=False, ring=True).raw
    assert np.array_equal(bits(tr.cum_reward.cpu().numpy()), bits(st["cum_reward"])), f"{what}: cum_reward"
    assert np.array_equal(tr.cum_steps.cpu().numpy(), st["cum_steps"]), f"{what}: cum_steps"
    assert got["ring_count"] == st["ring_count"], f"{what}: ring_count {got['ring_count']} != {st['ring_count']}"
    assert np.array_equal(bits(got["ring_ret"]), bits(st["ring_ret"])), f"{what}: ring_ret"
    assert np.array_equal(got["ring_len"], st["ring_len"]), f"{what}: ring_len"
    for k in R.INT_FIELDS:
        assert got[k] == rec[k], f"{what}: {k} {got[k]} != {rec[k]}"
    for k in R.F32_FIELDS:
        assert bits(got[k])[0] == bits(rec[k])[0], f"{what}: {k} {got[k]!r} != {rec[k]!r}"
    for k in R.F64_FIELDS:
        assert abs(got[k] - rec[k]) <= bounds[k], f"{what}: {k} {got[k]!r} vs {rec[k]!r}, bound {bounds[k]:.3e}"
    assert len(got["comp_sum"]) == len(bounds["comp_sum"]) == len(tr.components)
    for i, b in enumerate(bounds["comp_sum"]):
        assert abs(got["comp_sum"][i] - rec["comp_sum"][i]) <= b, f"{what}: comp_sum[{i}] {got['comp_sum'][i]!r} vs {rec['comp_sum'][i]!r}, bound {b:.3e}"
    full = tr.record.cpu().numpy().tobytes()
    assert full[72 + 8 * len(tr.components):200] == bytes(8 * (16 - len(tr.components))), f"{what}: an unused comp_sum is not zero"


def prepare(tr, ref, rng, ring_count):
    """A state in mid-run on both sides: random cumulative rewards and step counts, a full ring, ``ring_count`` episodes so far."""
    e, w = ref.E, ref.W
    ref.cum_reward = rng.uniform(-5, 5, e).astype(F)
    ref.cum_steps = rng.integers(0, 400, e).astype(np.int64)
    ref.ring_ret = rng.uniform(-9, 9, w).astype(F)
    ref.ring_len = rng.integers(1, 500, w).astype(np.int64)
    ref.ring_count = ring_count
    tr.cum_reward.copy_(dev(ref.cum_reward))
    tr.cum_steps.copy_(dev(ref.cum_steps.astype(np.int32)))
    tr.ring_ret.copy_(dev(ref.ring_ret))
    tr.ring_len.copy_(dev(ref.ring_len.astype(np.int32)))
    tr.ring_count.fill_(ring_count)


@pytest.mark.parametrize("w", [1, 4, 100])
@pytest.mark.parametrize("e", [1, 63, 64, 65, 255, 256, 257, 333])
def test_sequence_of_40_calls(eng, e, w):
    rng = np.random.default_rng(1000 * e + w)
    tr, ref = tracker(eng, e, w, ("x", "n")), R.Tracker(e, w, 2)
    finished = 0
    for i in range(40):
        r = rng.uniform(-1, 1, e).astype(F)
        d = rng.random(e) < 0.1
        compare(tr, feed(tr, ref, r, d, columns(rng, e, "fi")), f"E {e} W {w} call {i}")
        finished += int(d.sum())
    assert ref.ring_count == finished and (e < 63 or finished > w)          # the ring wrapped, except for the single env


def test_ring_nobody_finishes(eng):
    rng = np.random.default_rng(1)
    tr, ref = tracker(eng, 333), R.Tracker(333)
    prepare(tr, ref, rng, 250)
    before = ref.ring_ret.copy()
    compare(tr, feed(tr, ref, rng.uniform(-1, 1, 333).astype(F), np.zeros(333, dtype=bool)), "nobody")
    assert np.array_equal(tr.ring_ret.cpu().numpy(), before) and ref.record["win_calls"] == 1 and ref.record["ep_count"] == 0


def test_ring_everybody_finishes(eng):
    """E = 333 > W = 100 from ring_count = 1234: the ring holds envs 233 .. 332, env 233 + i at slot (1234 + 233 + i) mod 100."""
    rng = np.random.default_rng(2)
    tr, ref = tracker(eng, 333), R.Tracker(333)
    prepare(tr, ref, rng, 1234)
    r = rng.uniform(-1, 1, 333).astype(F)
    c, n = ref.cum_reward + r, ref.cum_steps + 1
    compare(tr, feed(tr, ref, r, np.ones(333, dtype=bool)), "everybody")
    ring_ret, ring_len = tr.ring_ret.cpu().numpy(), tr.ring_len.cpu().numpy()
    for j in range(233, 333):
        assert bits(ring_ret[(1234 + j) % 100])[0] == bits(c[j])[0] and ring_len[(1234 + j) % 100] == n[j], j
    assert int(tr.ring_count.item()) == 1234 + 333 and not tr.cum_reward.any() and not tr.cum_steps.any()


@pytest.mark.parametrize("n_fin", [99, 100, 101])
def test_ring_about_a_window_finishes(eng, n_fin):
    rng = np.random.default_rng(n_fin)
    tr, ref = tracker(eng, 333), R.Tracker(333)
    prepare(tr, ref, rng, 57)
    d = np.zeros(333, dtype=bool)
    d[rng.choice(333, n_fin, replace=False)] = True
    compare(tr, feed(tr, ref, rng.uniform(-1, 1, 333).astype(F), d), f"{n_fin} finish")
    assert ref.ring_count == 57 + n_fin


def test_ring_wraps_across_two_calls(eng):
    rng = np.random.default_rng(4)
    tr, ref = tracker(eng, 333), R.Tracker(333)
    prepare(tr, ref, rng, 70)
    for n_fin in (50, 90):                               # 70 -> 120 (wraps at slot 20) -> 210
        d = np.zeros(333, dtype=bool)
        d[rng.choice(333, n_fin, replace=False)] = True
        compare(tr, feed(tr, ref, rng.uniform(-1, 1, 333).astype(F), d), f"wrap, {n_fin} finish")
    assert ref.ring_count == 210 and ref.ring_count % 100 != 0


def test_more_workgroups_than_merge_threads(eng):
    """E = 257 * 256 + 1: 258 partial records for the 256 threads of the merge kernel, the last workgroup holding one env."""
    e = 65793
    rng = np.random.default_rng(5)
    tr, ref = tracker(eng, e, 100, ("x",)), R.Tracker(e, 100, 1)
    assert tr.sizes["n_partials"] == 258
    d = np.zeros(e, dtype=bool)
    d[::997] = True
    d[-1] = True
    for i in range(3):
        compare(tr, feed(tr, ref, rng.uniform(-1, 1, e).astype(F), d, columns(rng, e, "f")), f"E {e} call {i}")
    assert ref.ring_count == 3 * int(d.sum()) and int(d.sum()) == 67


@pytest.mark.parametrize("kind", ["bool", "uint8", "int64"])
def test_done_kinds_give_the_same_state(eng, kind):
    rng = np.random.default_rng(6)
    tr, ref = tracker(eng, 300, 8), R.Tracker(300, 8)
    for i in range(5):
        d = rng.random(300) < 0.2
        as_kind = d if kind == "bool" else (d.astype(np.uint8) * 7 if kind == "uint8" else d.astype(np.int64) * (2 ** 40))   # any non-zero value
        tr.step(dev(rng.uniform(-1, 1, 300).astype(F)), dev(as_kind))
    rng = np.random.default_rng(6)
    for i in range(5):
        d = rng.random(300) < 0.2
        snap = ref.call(rng.uniform(-1, 1, 300).astype(F), d)
    compare(tr, snap, f"done as {kind}")


@pytest.mark.parametrize("kinds", ["", "I", "fffIffff", "fIfififfffiIffff"], ids=["K0", "K1", "K8", "K16"])
def test_component_columns(eng, kinds):
    """float32 and int64 columns, among them one holding values of the size of the reference's collision_penalty sums."""
    rng = np.random.default_rng(7)
    e = 300
    names = tuple(f"c{i}" for i in range(len(kinds)))
    tr, ref = tracker(eng, e, 100, names), R.Tracker(e, 100, len(kinds))
    for i in range(4):
        compare(tr, feed(tr, ref, rng.uniform(-1, 1, e).astype(F), rng.random(e) < 0.1, columns(rng, e, kinds)), f"K {len(kinds)} call {i}")
    if "I" in kinds:
        assert ref.snapshot()[1]["comp_sum"][kinds.index("I")] > 4 * e * BIG_INT / 4


def test_two_runs_end_in_the_same_bytes(eng):
    e = 65793
    rng = np.random.default_rng(8)
    names = tuple(f"c{i}" for i in range(8))
    steps = [(dev(rng.uniform(-1, 1, e).astype(F)), dev(rng.random(e) < 0.05), {n: dev(c) for n, c in zip(names, columns(rng, e, "fffIffff"))})
             for _ in range(4)]
    ends = []
    for _ in range(2):
        tr = tracker(eng, e, 100, names)
        for s in steps:
            tr.step(*s)
        ends.append(state_bytes(tr))
    assert ends[0] == ends[1]


def test_captured_graph_equals_eager_calls(eng):
    e = 333
    rng = np.random.default_rng(9)
    names = ("x", "n")
    steps = [(dev(rng.uniform(-1, 1, e).astype(F)), dev((rng.random(e) < 0.1).astype(np.int64)), {n: dev(c) for n, c in zip(names, columns(rng, e, "fi"))})
             for _ in range(11)]
    eager, replayed = tracker(eng, e, 16, names), tracker(eng, e, 16, names)
    for s in steps:
        eager.step(*s)
    static = (steps[0][0].clone(), steps[0][1].clone(), {n: t.clone() for n, t in steps[0][2].items()})
    replayed.step(*static)                                   # the warm-up call builds the descriptor
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.step(*static)
    for s in steps[1:]:
        static[0].copy_(s[0])
        static[1].copy_(s[1])
        for n in names:
            static[2][n].copy_(s[2][n])
        graph.replay()
    assert state_bytes(replayed) == state_bytes(eager)
    assert replayed.read(reset=False).raw["calls"] == 11


def test_read_resets_the_record_only(eng):
    from isaac_rover_amd import _lib
    rng = np.random.default_rng(10)
    tr, ref = tracker(eng, 100, 8, ("x",)), R.Tracker(100, 8, 1)
    for i in range(6):
        snap = feed(tr, ref, rng.uniform(-1, 1, 100).astype(F), rng.random(100) < 0.2, columns(rng, 100, "f"))
    compare(tr, snap, "before the read")
    before = state_bytes(tr)
    out = tr.read()                                          # reset=True
    assert out["Episodes / finished"] == snap[1]["ep_count"] > 8 and "Reward / Total reward (mean)" in out and "Info / x (mean)" in out
    after = state_bytes(tr)
    assert after[:5] == before[:5] and after[5] == bytes(_lib.track_fresh_record()) != before[5]
    ref.reset_record()
    compare(tr, feed(tr, ref, rng.uniform(-1, 1, 100).astype(F), rng.random(100) < 0.2, columns(rng, 100, "f")), "after the read")
    assert ref.record["calls"] == 1 and ref.record["win_calls"] == 1


def test_zero_envs_is_a_counted_call(eng):
    from isaac_rover_amd import _lib
    tr, ref = tracker(eng, 0, 5), R.Tracker(0, 5)
    empty = torch.zeros(0, device=DEV)
    for i in range(2):
        tr.step(empty, empty.bool())
        compare(tr, ref.call(np.zeros(0, dtype=F), np.zeros(0, dtype=bool)), f"E 0 call {i}")
    want = _lib.track_fresh_record()
    want.calls = 2
    assert state_bytes(tr)[5] == bytes(want) and int(tr.ring_count.item()) == 0
    assert dict(tr.read()) == {"Episodes / finished": 0}


def test_engine_episode_track_checks_its_tensors(eng):
    from isaac_rover_amd import _lib
    tr = tracker(eng, 10, 4)
    r, d = torch.zeros(10, device=DEV), torch.zeros(10, dtype=torch.bool, device=DEV)
    kw = dict(cum_reward=tr.cum_reward, cum_steps=tr.cum_steps, ring_ret=tr.ring_ret, ring_len=tr.ring_len, ring_count=tr.ring_count,
              record=tr.record, scratch=tr.scratch)
    for bad in (dict(rewards=r.double()), dict(rewards=r.cpu()), dict(done=d.float()), dict(done=d[:9]), dict(cum_steps=tr.cum_steps.long()),
                dict(ring_len=tr.ring_len[:3]), dict(record=tr.record[:100]), dict(scratch=tr.scratch[:16]), dict(components=(r.double(),)),
                dict(components=(torch.zeros(20, device=DEV)[::2],)), dict(components=(r,) * 17), dict(ring_count=None)):
        args = dict(rewards=r, done=d, **kw)
        args.update(bad)
        with pytest.raises(_lib.RoverError):
            eng.episode_track(args.pop("rewards"), args.pop("done"), **args)
    assert tr.read(reset=False).raw["calls"] == 0
    eng.episode_track(r, d, **kw)
    assert tr.read(reset=False).raw["calls"] == 1


def test_rover_task_end_to_end():
    """60 VecEnv.step()s of a RoverTask (64 envs, 37 rays, the small synthetic scene) with the task's own rew_buf, int64 reset_buf and
    extras handed to EpisodeTracker.step, and a copy of them to the restatement.  Episodes are made short the way test_task_gpu.py does:
    progress_buf is set just below max_episode_length, so the envs time out a few steps later, at different steps."""
    from isaac_rover_amd import _lib, synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.learning.tracking import EpisodeTracker
    from isaac_rover_amd.tasks.rover import RoverTask
    from isaac_rover_amd.vec_env import VecEnv
    e = 64
    scene = synth.make_scene(n_cells=128, k=16, n_stones=10)
    env = VecEnv(headless=True)
    g = torch.Generator().manual_seed(3)
    spawn = torch.zeros(e, 3)
    spawn[:, 0:2] = 4.0 + 4.8 * torch.rand(e, 2, generator=g)
    task = RoverTask("Rover", SimConfig(num_envs=e, device="cuda:0"), env, scene=scene, distribution=synth.ray_distribution("37"))
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    env.reset()
    tr, ref = EpisodeTracker.for_task(task, window=16), R.Tracker(e, 16, 8)
    assert tr.components == _lib.EXTRAS and len(tr.components) == 8
    for i in range(60):
        if i % 15 == 0:
            task.progress_buf.copy_(task.max_episode_length - 2 - torch.randint(0, 12, (e,), generator=g).to(task.progress_buf.device))
        obs, rew, done, extras = env.step((2 * torch.rand(e, 2, generator=g) - 1).cuda())
        assert rew.dtype == torch.float32 and done.dtype == torch.int64 and extras["collision_penalty"].dtype == torch.int64
        tr.step(rew, done, extras)
        snap = ref.call(rew.cpu().numpy(), done.cpu().numpy(), tuple(extras[k].cpu().numpy() for k in _lib.EXTRAS))
        compare(tr, snap, f"task step {i}")
    assert ref.ring_count > 2 * 16 and ref.record["ep_len_max"] > 1
    out = tr.read()
    assert set(out) >= {"Reward / Total reward (mean)", "Episodes / return (mean)"} | {f"Info / {k} (mean)" for k in _lib.EXTRAS}
    env.close()


def _example(name, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name), *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


TAG = "Reward / Total reward (mean)"


def test_rollout_example_prints_the_statistics_when_asked():
    base = ("--envs", "512", "--steps", "20")
    out = _example("rollout.py", *base, "--track-interval", "10")
    lines = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(lines) == 2 and lines[0].startswith("step 10: ") and lines[1].startswith("step 20: "), out
    assert TAG in lines[1] and "Info / pos_reward (mean)" in lines[1] and "Episodes / finished" in lines[0], out
    assert TAG not in _example("rollout.py", *base) and "20 steps x 512 envs" in out


def test_train_example_prints_the_statistics_when_asked():
    base = ("--envs", "512", "--steps", "20", "--rollouts", "10", "--mini-batches", "4", "--epochs", "1")
    out = _example("train.py", *base, "--track-interval", "20", "--track-window", "50")
    lines = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(lines) == 1 and TAG in lines[0], out
    assert len([l for l in out.splitlines() if l.startswith("update ")]) == 2, out          # train.py keeps its own print
    plain = _example("train.py", *base)
    assert TAG not in plain and len([l for l in plain.splitlines() if l.startswith("update ")]) == 2


def test_distill_example_prints_the_statistics_when_asked():
    out = _example("distill.py", "--envs", "64", "--window", "4", "--updates", "2", "--track-interval", "8")
    lines = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(lines) == 1 and lines[0].startswith("step 8: ") and "Episodes / finished" in lines[0] and "Info / pos_reward (mean)" in lines[0], out
    assert len([l for l in out.splitlines() if l.startswith("update ")]) == 2, out
