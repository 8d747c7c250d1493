"""CPU: the task layer's cached launch state (`tasks/rover.py`: `RoverTask._launch_tensors`, `RoverTask._launches`, `_StepLaunches`) and
`Engine.generation`, on CPU tensors with a stub engine — no GPU, no library.

The task under test is a `RoverTask` that skipped `__init__`: its attributes are set from the list of launch tensors itself, so a name
added to the list is covered by every test here without another line."""
import types

import pytest
import torch

from isaac_rover_amd import _abi, _lib
from isaac_rover_amd.tasks import rover
from isaac_rover_amd.tasks.rover import RoverTask, _StepLaunches

E = 4
PACKERS = ("make_in", "make_out", "bind_pre_physics", "bind_reset_envs")


class StubEngine:
    """Records what the four packing calls receive; `reset_envs` / `step` record that they ran."""

    def __init__(self):
        self.generation = 0
        self.calls = []

    def _record(self, name, result):
        def call(*args, **kw):
            self.calls.append((name, args, kw))
            return result
        return call

    def __getattr__(self, name):
        if name in PACKERS:
            return self._record(name, types.SimpleNamespace() if name.startswith("make") else self._record(name + "()", None))
        if name in ("reset_envs", "step"):
            return self._record(name, None)
        raise AttributeError(name)

    def packed(self):
        """Every tensor the LAST round of the four packing calls received (identity-keyed)."""
        last = {}
        for name, args, kw in self.calls:
            if name in PACKERS:
                last[name] = (args, kw)
        assert set(last) == set(PACKERS)
        seen = {}
        for args, kw in last.values():
            for v in list(args) + list(kw.values()):
                for t in (v.values() if isinstance(v, dict) else [v]):
                    if isinstance(t, torch.Tensor):
                        seen[id(t)] = t
        return seen


def _get(task, name):
    if name.startswith("extras."):
        return task.extras[name[7:]]
    obj = task
    for part in name.split("."):
        obj = getattr(obj, part)
    return obj


def _set(task, name, value):
    if name.startswith("extras."):
        task.extras[name[7:]] = value
        return
    *path, last = name.split(".")
    obj = task
    for part in path:
        if not hasattr(obj, part):
            setattr(obj, part, types.SimpleNamespace())
        obj = getattr(obj, part)
    setattr(obj, last, value)


def make_task():
    task = RoverTask.__new__(RoverTask)
    task.extras = {}
    for i, name in enumerate(rover._LAUNCH_NAMES):
        _set(task, name, torch.full((E, 3), float(i)))
    task._engine = StubEngine()
    task._device, task._stone_margin, task._launch = "cpu", None, None
    task._balls = types.SimpleNamespace(_pos=None)
    return task


def test_the_list_names_what_the_task_holds():
    task = make_task()
    t = task._launch_tensors()
    assert tuple(t) == rover._LAUNCH_NAMES and len(set(t)) == len(t)
    for name in t:
        assert t[name] is _get(task, name)
    # the arguments of the four packing calls are exactly the list: nothing bound that is not listed, nothing listed that is not bound
    task._launches()
    assert set(task._engine.packed()) == {id(v) for v in t.values()}


def test_accessor_returns_the_same_object_while_nothing_changes():
    task = make_task()
    cur = task._launches()
    n = len(task._engine.calls)
    assert task._launches() is cur and task._launches() is cur and len(task._engine.calls) == n
    assert task._sin is cur.sin and task._sout is cur.sout


@pytest.mark.parametrize("name", rover._LAUNCH_NAMES)
def test_every_name_is_in_the_key(name):
    """Replacing that one tensor by a clone rebuilds, and the next pack holds the clone, not the original."""
    task = make_task()
    first = task._launches()
    first.pre_graph = first.post_graph = object()
    old = _get(task, name)
    new = old.clone()
    _set(task, name, new)
    cur = task._launches()
    assert cur is not first and task._launches() is cur
    assert first.key == ((), None) and first.pre_graph is None and first.post_graph is None      # the replaced state cannot be launched
    assert cur.pre_graph is None and cur.post_graph is None
    packed = task._engine.packed()
    assert id(new) in packed and id(old) not in packed
    assert task._sin is cur.sin and task._sout is cur.sout
    assert _get(task, name) is new                                                            # (the caller's tensor stays in place)


@pytest.mark.parametrize("name", rover._LAUNCH_NAMES)
def test_in_place_writes_do_not_rebuild(name):
    task = make_task()
    cur = task._launches()
    n = len(task._engine.calls)
    t = _get(task, name)
    t.fill_(1)
    assert task._launches() is cur
    t.copy_(torch.ones(E, 3) * 5)
    assert task._launches() is cur
    t[:] += 1
    assert task._launches() is cur and len(task._engine.calls) == n and bool((t == 6).all())


def test_a_rebound_actions_nn_is_converted_once():
    """`actions_nn` is shifted in place by the kernel: a replacement of another dtype or layout becomes the contiguous float32 tensor
    the kernel needs — one case of the general rule (it is a listed tensor), not a check of its own."""
    task = make_task()
    task._launches()
    task.actions_nn = torch.arange(E * 6, dtype=torch.float64).reshape(E, 3, 2).transpose(1, 2)
    want = task.actions_nn.clone()
    cur = task._launches()
    a = task.actions_nn
    assert a.dtype == torch.float32 and a.is_contiguous() and torch.equal(a, want.float())
    assert id(a) in task._engine.packed() and task._launches() is cur


def test_generation_is_in_the_key():
    task = make_task()
    first = task._launches()
    first.pre_graph = first.post_graph = object()
    task._engine.generation += 1
    cur = task._launches()
    assert cur is not first and first.pre_graph is None and first.post_graph is None
    assert cur.pre_graph is None and cur.post_graph is None and task._launches() is cur


def _stub_lib():
    class Lib:
        def __getattr__(self, name):
            return lambda *a, **k: 0
    return Lib()


def _engine_setter_args():
    import numpy as np
    from isaac_rover_amd import synth
    scene = synth.make_scene(n_cells=16, k=4, n_stones=4)
    distn = synth.ray_distribution("9")
    return {
        "set_knn_map": (0, np.zeros((2, 2, 1), np.int32), np.zeros((1, 3), np.int32), np.zeros((3, 3), np.float32)),
        "set_distribution": distn,
        "set_heightfield": (np.zeros((4, 4), np.float32),),
        "set_stones": (np.zeros((2, 7), np.float32),),
        "set_curriculum_level": (1,),
        "set_option": ("ray_precision", 0),
        "set_evaluation": (True,),
        "set_profiling": (True,),
        "set_scene": (scene, distn),
        "eval_clear": (),
    }


def test_every_engine_setter_bumps_the_generation(monkeypatch):
    """Every `Engine.set_*` method and `eval_clear` changes something a cached launch may have baked in, by value or by address: each
    must bump `generation`.  The methods are enumerated from the class, so a new setter without arguments here, or without a bump, fails."""
    monkeypatch.setattr(_abi, "_stream", lambda *a: None)        # where Engine._call looks the accessor up
    names = sorted(n for n in dir(_lib.Engine) if n.startswith("set_")) + ["eval_clear"]
    args = _engine_setter_args()
    assert set(names) == set(args), "give every Engine.set_* method its arguments in _engine_setter_args()"
    assert {"set_knn_map", "set_distribution", "set_heightfield", "set_stones", "set_curriculum_level", "set_option", "set_evaluation",
            "eval_clear"} <= set(names)
    for name in names:
        eng = _lib.Engine.__new__(_lib.Engine)
        eng.lib, eng._h, eng._dev_index, eng.num_envs, eng.generation = _stub_lib(), 1, 0, E, 0
        getattr(eng, name)(*args[name])
        assert eng.generation >= 1, name
        eng._h = None


class _Graph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


def _captured(step):
    """A `_StepLaunches` as `capture()` leaves it, with stand-ins for the graphs (a replay here does not advance the word)."""
    task = make_task()
    cur = task._launches()
    cur.pre_graph, cur.post_graph = _Graph(), _Graph()
    cur.actions, cur.seed_word, cur.seed_step = torch.zeros(E, 2), torch.full((1,), -7, dtype=torch.int64), step
    return cur


def test_seed_word_is_set_from_the_host_exactly_when_it_is_not_the_previous_steps():
    word = lambda step: rover._to_i64(step * rover._STEP_KEY)
    acts = torch.rand(E, 2)
    # steady state: the word stands for step 20, step 21 replays — nothing is written
    cur = _captured(20)
    cur.replay_pre(acts, 21)
    assert int(cur.seed_word) == -7 and cur.seed_step == 21 and cur.pre_graph.replays == 1 and torch.equal(cur.actions, acts)
    cur.replay_pre(acts, 22)
    assert int(cur.seed_word) == -7 and cur.seed_step == 22
    # an eager step in between (22 replayed, 23 eager, 24 replays), a caller's global_step, and the first replay after capture()
    for recorded, step in ((22, 24), (22, 3000), (22, 22), (22, 5), (None, 12)):
        cur = _captured(recorded)
        cur.replay_pre(acts, step)
        assert int(cur.seed_word) == word(step - 1), (recorded, step)        # the captured add_ makes it this step's
        assert cur.seed_step == step and cur.pre_graph.replays == 1


def test_a_rebuilt_state_starts_without_a_seed_step():
    task = make_task()
    assert task._launches().seed_step is None and isinstance(task._launches(), _StepLaunches)


def test_eager_pre_physics_step_launches_pre_before_reset():
    """`rover_pre_physics_step` reads the PRE-reset orientation (rover.py:343 runs before :359): the bound pre-physics call goes first,
    the reset second — bound with the step's seed, or packed per call when the caller gives the yaws."""
    task = make_task()
    eng = task._engine
    eng.compact_resets = eng._record("compact_resets", None)
    task._rover.get_world_poses = lambda: (task._rover._pos, task._rover._quat)
    task.global_step, task._seed, task._compaction_fresh, task._device_reset, task._use_graph = 20, 3, True, True, False
    actions = torch.rand(E, 2)
    task.pre_physics_step(actions)
    names = [c[0] for c in eng.calls]
    assert names[-2:] == ["bind_pre_physics()", "bind_reset_envs()"] and "compact_resets" not in names
    assert eng.calls[-2][1][0] is actions and eng.calls[-1][1] == (task._rng_seed(),) and task.global_step == 21
    yaw = torch.zeros(E, dtype=torch.int32)
    task.pre_physics_step(actions, reset_yaw_deg=yaw)
    names = [c[0] for c in eng.calls]
    assert names[-3:] == ["compact_resets", "bind_pre_physics()", "reset_envs"]
    kw = eng.calls[-1][2]
    assert kw["yaw_deg"] is yaw and kw["seed"] == task._rng_seed() and kw["pos3"] is task._rover._pos and "seed_dev" not in kw
