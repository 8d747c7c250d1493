"""GPU (-m gpu): the RoverTask / RLTask / VecEnv mirror of the reference API, driven like the reference's own
post_physics_step (rl_task.py:239-259) and pre_physics_step (rover.py:338-414)."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_step_close, load_golden, scene_for, states_of

pytestmark = pytest.mark.gpu


def _make_task(fx, fused, level=2, device_reset=True):
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.tasks.rover import RoverTask
    from isaac_rover_amd.vec_env import VecEnv
    scene = scene_for(fx)
    st = states_of(fx)
    e = st["pos"].shape[0]
    cfg = SimConfig(num_envs=e, device="cuda:0")
    env = VecEnv(headless=True)
    task = RoverTask("Rover", cfg, env, scene=scene, distribution=(fx["distribution"], fx["sparse_idx"], fx["dense_idx"]),
                     fused=fused, device_reset=device_reset,
                     cell_index_mode="cpu_div")      # the golden vectors were captured from the reference on the CPU (ATen division)
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=st["pos"].clone())
    # feed the captured sim state (the reference harness does the same on its SimpleNamespace)
    dev = task.device
    task._rover.feed(st["pos"].to(dev), st["quat"].to(dev), st["joints"].to(dev))
    task.target_positions.copy_(st["target"].to(dev))
    task.linear_velocity.tracker.copy_(st["lin_hist"].to(dev))
    task.angular_velocity.tracker.copy_(st["ang_hist"].to(dev))
    task.rover_rot.copy_(st["euler_pre"].to(dev))
    task.progress_buf.copy_(st["progress"].to(dev))
    task.curriculum_level = level
    task._engine.set_curriculum_level(level)
    return task, env


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["step_e64_p37_fp32", "step_e8_native_fp32", "step_e64_p37_fp32_level1"])
def test_post_physics_step_matches_reference(name, fused):
    fx = load_golden(name)
    task, env = _make_task(fx, fused, level=int(fx["curriculum_level"]))
    obs, rew, reset, extras = task.post_physics_step()
    assert obs is task.obs_buf and rew is task.rew_buf and reset is task.reset_buf      # same objects every step
    assert obs.dtype == torch.float32 and reset.dtype == torch.int64 and task.progress_buf.dtype == torch.int64
    got = dict(obs_buf=obs, rew_buf=rew, reset_buf=reset, progress_buf=task.progress_buf, euler=task.rover_rotation,
               heading_diff=task.heading_diff, rock_collision=task.rock_collison)
    got.update({"extras_" + k: v for k, v in extras.items()})
    torch.cuda.synchronize()
    assert_step_close(got, fx, name)
    assert set(extras) == {"pos_reward", "collision_penalty", "uprightness_penalty", "heading_contraint_penalty",
                           "motion_contraint_penalty", "goal_angle_penalty", "torque_penalty_driving",
                           "torque_penalty_steering"}
    env.close()


def test_camera_get_depths_on_the_task():
    """The drop-in task's `self.Camera.get_depths(positions, rotations)` (camera.py:60, bound by rover.py:286): the reference's triple
    on the reference's own inputs (tests/golden/get_depths_e64_p37.npz)."""
    fx = load_golden("get_depths_e64_p37")
    step_fx = load_golden("step_e64_p37_fp32")
    task, env = _make_task(step_fx, True)
    dev = task.device
    d, pt, src = task.Camera.get_depths(torch.from_numpy(fx["in_pos"]).to(dev), torch.from_numpy(fx["in_euler"]).to(dev))
    torch.cuda.synchronize()
    np.testing.assert_allclose(src.cpu().numpy(), fx["out_fp32_src"], rtol=1e-6, atol=2e-6)
    close = np.abs(d.cpu().numpy() - fx["out_fp32_dist"]) <= 2e-3
    assert close.mean() >= 0.999
    np.testing.assert_allclose(pt.cpu().numpy()[close], fx["out_fp32_pt"][close], rtol=0, atol=2.5e-3)
    env.close()


def test_rock_detector_get_collisions_on_the_task():
    """The drop-in task's `self.Rock_detector.get_collisions(positions, rotations, joints)` (rock_detect.py:52, held at rover.py:94,
    called at rover.py:291): the reference's (wheel_dist, body_dist) on the reference's own inputs; `check_collision` on them gives the
    fixture's collision mask."""
    fx = load_golden("step_e64_p37_fp32")
    task, env = _make_task(fx, True)
    dev = task.device
    wheel, body = task.Rock_detector.get_collisions(torch.from_numpy(fx["in_pos"]).to(dev), torch.from_numpy(fx["out_euler"]).to(dev),
                                                    torch.from_numpy(fx["in_joints"]).to(dev))
    torch.cuda.synchronize()
    for got, want in ((wheel, fx["out_wheel_dist"]), (body, fx["out_body_dist"])):
        d = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64))
        assert float((d > 2e-3).mean()) <= 1e-3
    task.check_collision(wheel, body)                                                           # rover.py:663-668
    np.testing.assert_array_equal(task.rock_collison.cpu().numpy(), fx["out_rock_collision"])
    env.close()


def test_native_observation_layout():
    """1634 rays -> 1750-float observation = [4 | 634 sparse | 1112 dense] (learning/model.py:186-192)."""
    fx = load_golden("step_e8_native_fp32")
    task, env = _make_task(fx, True)
    assert task.num_observations == 1750 and task.num_actions == 2
    assert task.observation_space.shape == (1750,) and task.action_space.shape == (2,)
    assert task.Camera.heightmap.get_num_sparse_vector() == 634 and task.Camera.heightmap.get_num_dense_vector() == 1112
    env.close()


@pytest.mark.parametrize("device_reset", [True, False])
def test_pre_physics_step_reset_branch(device_reset):
    """rover.py:356-361,416-453,566-584: compaction order, reset bookkeeping, goal validity."""
    fx = load_golden("step_e64_p37_fp32")
    task, env = _make_task(fx, True, device_reset=device_reset)
    task.post_physics_step()
    reset_before = task.reset_buf.clone()
    ids = reset_before.nonzero(as_tuple=False).squeeze(-1)
    assert len(ids) > 0
    task.global_step = 20
    actions = torch.zeros(task.num_envs, 2, device=task.device)
    actions[:, 0] = 0.5
    hist_before = task.linear_velocity.tracker.clone()
    task.pre_physics_step(actions)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(task.reset_env_ids_buf[: len(ids)].cpu().numpy(), ids.cpu().numpy())
    assert int(task.reset_buf[ids].sum()) == 0 and int(task.progress_buf[ids].sum()) == 0
    keep = (reset_before == 0).nonzero().squeeze(-1)
    assert bool((task.progress_buf[keep] > 0).all())
    # goals: 8 m from the spawn, clearance > 1.0, z on the heightfield
    tgt = task.target_positions[ids]
    r = (tgt[:, 0:2] - task.initial_pos[ids][:, 0:2]).norm(dim=1)
    if 0 not in ids.tolist():
        np.testing.assert_allclose(r.cpu().numpy(), 8.0, atol=1e-4)
    assert bool((task._engine.clearance(tgt[:, 0:2].contiguous()) > 1.0).all())
    np.testing.assert_array_equal(tgt[:, 2].cpu().numpy(), task._engine.sample_height(tgt[:, 0:2].contiguous()).cpu().numpy())
    # rovers back at their spawn, joints zeroed, history shifted (Memory, rover.py:60-77)
    pos, quat = task._rover.get_world_poses()
    np.testing.assert_array_equal(pos[ids].cpu().numpy(), task.initial_pos[ids].cpu().numpy())
    np.testing.assert_allclose(quat[ids].norm(dim=1).cpu().numpy(), 1.0, atol=1e-6)
    assert float(task._rover.get_joint_positions()[ids].abs().sum()) == 0.0
    np.testing.assert_array_equal(task.linear_velocity.tracker[:, 0].cpu().numpy(), actions[:, 0].cpu().numpy())
    np.testing.assert_array_equal(task.linear_velocity.tracker[:, 1:].cpu().numpy(), hist_before[:, :2].cpu().numpy())
    env.close()


def test_device_reset_equals_host_reset():
    """The no-host-sync orchestration (rover_pre_physics_step + rover_reset_envs) and the reference-shaped control flow
    leave identical state when fed the same yaw draws (goal draws come from the same Philox stream)."""
    fx = load_golden("step_e64_p37_fp32")
    states = []
    for device_reset in (True, False):
        task, env = _make_task(fx, True, device_reset=device_reset)
        task.post_physics_step()
        task.global_step = 20
        g = torch.Generator().manual_seed(5)
        actions = (2 * torch.rand(task.num_envs, 2, generator=g) - 1).cuda()
        yaw = torch.randint(0, 361, (task.num_envs,), generator=g, dtype=torch.int32).cuda()
        task.pre_physics_step(actions, reset_yaw_deg=yaw)
        torch.cuda.synchronize()
        pos, quat = task._rover.get_world_poses()
        states.append(dict(pos=pos.clone(), quat=quat.clone(), joints=task._rover.get_joint_positions().clone(),
                           target=task.target_positions.clone(), reset=task.reset_buf.clone(), progress=task.progress_buf.clone(),
                           lin=task.linear_velocity.tracker.clone(), ang=task.angular_velocity.tracker.clone(),
                           rot=task.rover_rot.clone(), jpt=task._rover._joint_pos_targets.clone(),
                           jvt=task._rover._joint_vel_targets.clone(), base=task.base_pos.clone()))
        env.close()
    a, b = states
    for k in a:
        if k == "quat":
            np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), atol=1e-6, err_msg=k)
        else:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=k)


def _assert_twins_equal(a, b, label):
    """Two tasks driven by the same actions hold identical buffers (what `test_task_graph_replay_equals_eager` compares at every step)."""
    for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "target_positions", "rover_rot", "rover_rotation", "heading_diff",
                 "rock_collison", "stone_collision", "actions_nn", "reset_env_ids_buf", "_n_reset", "base_pos"):
        x, y = getattr(a, name), getattr(b, name)
        if name == "reset_env_ids_buf":
            n = int(a._n_reset.item())
            x, y = x[:n], y[:n]
        assert torch.equal(x, y), f"{label}: {name}"
    for k in a.extras:
        assert torch.equal(a.extras[k], b.extras[k]), f"{label}: extras.{k}"
    for x, y in zip(a._rover.get_world_poses() + (a._rover._joint_pos_targets, a._rover._joint_vel_targets, a.linear_velocity.tracker),
                    b._rover.get_world_poses() + (b._rover._joint_pos_targets, b._rover._joint_vel_targets, b.linear_velocity.tracker)):
        assert torch.equal(x, y), f"{label}: rover state"


def test_task_graph_replay_equals_eager():
    """graph=True: from global step 11 on `pre_physics_step` and `post_physics_step` replay captured hipGraphs.  Two tasks — one eager, one
    replaying — driven through VecEnv.step() by the same actions over the curriculum switch, a reset() in the middle and 60 steps leave
    identical buffers at every step: obs, reward, done, progress, extras, poses, targets (the device RNG's step counter lives on the
    device in graph mode and must draw what the eager call of the same step draws), histories, joint targets."""
    from isaac_rover_amd import synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.vec_env import VecEnv, initialize_task
    scene = synth.make_scene(n_cells=128, k=16, n_stones=24)
    e = 192
    envs, tasks = [], []
    for graph in (False, True):
        env = VecEnv(headless=True)
        tasks.append(initialize_task(SimConfig(num_envs=e, device="cuda:0"), env, scene, distribution=synth.ray_distribution("37"),
                                     graph=graph, stone_mask_margin=0.0))
        envs.append(env)
    obs = [env.reset() for env in envs]
    g = torch.Generator().manual_seed(11)
    n_resets, redrawn = 0, 0
    for i in range(60):
        actions = (2 * torch.rand(e, 2, generator=g) - 1).cuda()
        if i == 30:
            for t in tasks:
                t.reset()                     # every env flagged: the next pre_physics_step re-spawns all of them
        if i == 40:
            for t in tasks:
                t.progress_buf[::3] = 2995    # a third of the envs time out a few steps later (rover.py:614): partial resets
        prev_target = tasks[1].target_positions.clone()
        outs = [env.step(actions.clone()) for env in envs]
        torch.cuda.synchronize()
        a, b = tasks
        _assert_twins_equal(a, b, f"step {i}")
        for x, y in zip(outs[0][:3], outs[1][:3]):
            assert torch.equal(x, y)
        n_resets += int(a._n_reset.item())
        if i > 12:
            redrawn += int((b.target_positions != prev_target).any(dim=1).sum().item())
    graphs = [(t._launches().pre_graph, t._launches().post_graph) for t in tasks]
    assert graphs[1][0] is not None and graphs[1][1] is not None and graphs[0] == (None, None)
    # the replayed graph did reset envs and draw new goals: all of them after reset(), then the timed-out third
    assert n_resets >= e // 3 and redrawn >= e + e // 3 - 8, (n_resets, redrawn)
    for env in envs:
        env.close()


_TWIN_ENVS = 64          # one wavefront, env 0 (the goal-aliasing quirk of rover.py:544-549) included


def _twins(graph, steps=14):
    """(eager twin, task under test, their envs, the generator of their actions) after `steps` identical steps — past global step 12, so a
    graph task has captured and replayed.  The scene of `test_task_graph_replay_equals_eager`, the 37-ray distribution."""
    from isaac_rover_amd import synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.vec_env import VecEnv, initialize_task
    if "scene" not in _TWIN_SCENE:
        _TWIN_SCENE["scene"] = synth.make_scene(n_cells=128, k=16, n_stones=24)
    envs, tasks = [], []
    for g in (False, graph):
        env = VecEnv(headless=True)
        tasks.append(initialize_task(SimConfig(num_envs=_TWIN_ENVS, device="cuda:0"), env, _TWIN_SCENE["scene"],
                                     distribution=synth.ray_distribution("37"), graph=g, stone_mask_margin=0.0))
        envs.append(env)
    for env in envs:
        env.reset()
    gen = torch.Generator().manual_seed(17)
    for i in range(steps):
        _twin_step(tasks, envs, gen, f"warm-up step {i}")
    if graph:
        assert tasks[1]._launches().pre_graph is not None and tasks[1]._launches().post_graph is not None
    return tasks[0], tasks[1], envs, gen


_TWIN_SCENE = {}


def _twin_step(tasks, envs, gen, label, yaw=None):
    """One step of both tasks on the same actions (with ``yaw``: the reset yaws given, which both tasks run eagerly), then the comparison."""
    actions = (2 * torch.rand(_TWIN_ENVS, 2, generator=gen) - 1).cuda()
    for task, env in zip(tasks, envs):
        if yaw is None:
            env.step(actions.clone())
        else:
            task.pre_physics_step(actions.clone(), reset_yaw_deg=yaw)
            env._world.step()
            task.post_physics_step()
    torch.cuda.synchronize()
    _assert_twins_equal(tasks[0], tasks[1], label)


def test_task_graph_eager_step_between_replays():
    """A step that the graph task runs eagerly (reset yaws given) between two replays: the device RNG's step word, which only a replay
    advances, must be brought up to date before the next replay.  Every env is reset on both steps, so a replay that drew with the
    earlier step's Philox key would give every env the goal it already has.  "Most envs": the goal angle is a continuous draw, so two
    keys give an env the same goal with probability ~0; more than half of the envs leaves room for nothing but that."""
    a, b, envs, gen = _twins(graph=True)
    yaw = torch.randint(0, 361, (_TWIN_ENVS,), generator=gen, dtype=torch.int32).cuda()
    for t in (a, b):
        t.reset()
    _twin_step((a, b), envs, gen, "eager step", yaw=yaw)
    first = b.target_positions.clone()
    for t in (a, b):
        t.reset()
    _twin_step((a, b), envs, gen, "replay after the eager step")
    changed = int((b.target_positions != first).any(dim=1).sum().item())
    assert changed > _TWIN_ENVS // 2, changed
    assert b._launches().pre_graph is not None
    for env in envs:
        env.close()


@pytest.mark.parametrize("graph", [False, True])
def test_task_rebound_buffers_are_written(graph):
    """Replacing `rew_buf`, `obs_buf` and an `extras` entry by fresh tensors (what the reference's `cleanup()` does): the next step
    writes the new tensors, and `task._sout` points at them."""
    a, b, envs, gen = _twins(graph=graph)
    b.rew_buf, b.obs_buf = torch.zeros_like(b.rew_buf), torch.zeros_like(b.obs_buf)
    b.extras["pos_reward"] = torch.zeros_like(b.extras["pos_reward"])
    new = (b.rew_buf, b.obs_buf, b.extras["pos_reward"])
    _twin_step((a, b), envs, gen, "step after rebinding")
    assert b.rew_buf is new[0] and b.obs_buf is new[1] and b.extras["pos_reward"] is new[2]
    assert torch.equal(new[0], a.rew_buf) and torch.equal(new[1], a.obs_buf) and torch.equal(new[2], a.extras["pos_reward"])
    assert bool(new[1].abs().sum() > 0)
    assert (b._sout.rew, b._sout.obs, b._sout.ex_pos_reward) == tuple(t.data_ptr() for t in new)
    _twin_step((a, b), envs, gen, "second step after rebinding")
    for env in envs:
        env.close()


def test_task_second_set_up_scene_then_post_physics_step():
    """`set_up_scene` again after the graphs were captured, the same poses fed in, then `post_physics_step()` with no `pre_physics_step`
    before it: the step runs on the new views' tensors (a captured graph addresses the old ones)."""
    a, b, envs, gen = _twins(graph=True)
    spawn = a.initial_pos.clone()
    pos, quat = a._rover.get_world_poses(clone=True)
    joints = a._rover.get_joint_positions().clone()
    for t in (a, b):
        t.set_up_scene(spawn_positions=spawn)
        t._rover.feed(pos, quat, joints)
        t.post_physics_step()
    torch.cuda.synchronize()
    _assert_twins_equal(a, b, "post_physics_step after a second set_up_scene")
    assert bool(a.obs_buf.abs().sum() > 0) and b._sin.pos == b._rover._pos.data_ptr()
    for env in envs:
        env.close()


def test_task_engine_setter_reaches_a_captured_graph():
    """A value the kernels take by value (the curriculum level; no device buffer is re-sized) set on the engine after the capture:
    the next step runs with it, as the eager twin's does."""
    a, b, envs, gen = _twins(graph=True)
    before = b._launches()
    for t in (a, b):
        t._engine.set_curriculum_level(1)
    _twin_step((a, b), envs, gen, "step after set_curriculum_level(1)")
    assert b._launches() is not before and before.post_graph is None
    for env in envs:
        env.close()


def test_vec_env_rollout():
    """train.py-style loop: reset, then env.step(actions) for a while; curriculum flips at global step 10."""
    from isaac_rover_amd import synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.vec_env import VecEnv, initialize_task
    scene = synth.make_scene(n_cells=128, k=16, n_stones=10)
    cfg = SimConfig(num_envs=128, device="cuda:0")
    env = VecEnv(headless=True)
    g = torch.Generator().manual_seed(3)
    spawn = torch.zeros(128, 3)
    spawn[:, 0:2] = 4.0 + 4.8 * torch.rand(128, 2, generator=g)
    from isaac_rover_amd.tasks.rover import RoverTask
    task = RoverTask("Rover", cfg, env, scene=scene, distribution=synth.ray_distribution("37"))
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    obs = env.reset()
    assert obs.shape == (128, 41)
    n_resets = 0
    for i in range(30):
        actions = 2 * torch.rand(128, 2, generator=g) - 1
        obs, rew, done, info = env.step(actions.cuda())
        assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
        assert float(obs.abs().max()) <= 5.0                     # clipObservations, Rover.yaml:16
        n_resets += int(done.sum())
    assert task.curriculum_level == 2 and task.global_step == 31
    assert int(task.progress_buf.max()) <= 31
    env.close()


_RCCL_CHILD = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["ROVER_ROOT"])
import bench
from isaac_rover_amd.distributed import StepGather
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
bench._init_process_group(dist, dev)                      # init_process_group("nccl", device_id=cuda:0): RCCL loads and binds the device
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
dist.barrier()
t = torch.tensor([1.25], dtype=torch.float64, device=dev)
dist.all_reduce(t, op=dist.ReduceOp.MAX)
assert float(t.item()) == 1.25
g = StepGather(64, 41, dev, world=1, rank=0, depth=2)
obs, rew, done = g.local_views(1)
obs.fill_(0.5); rew.fill_(2.0); done.fill_(1)            # done travels as uint8
mine = torch.stack([bench._checksums(torch, *g.local_views(d)) for d in range(2)])
got = [torch.zeros_like(mine)]
dist.all_gather(got, mine)                                # the int64 checksum exchange of bench.py's gather_check
assert torch.equal(got[0], mine)
u8 = [torch.zeros_like(done)]
dist.all_gather(u8, done)                                 # uint8 tensors through RCCL
assert torch.equal(u8[0], done)
assert g.gather(1) is not None and g.global_views(1)[2].dtype == torch.uint8
torch.cuda.synchronize()
dist.barrier()
dist.destroy_process_group()
print("rccl world-size-1 ok")
"""


def test_rccl_world_size_1_in_a_fresh_process(tmp_path):
    """First contact with RCCL before the 8-GPU node: in a FRESH child process (the parent test process has long initialised the
    GPU: nothing is re-exec'ed, a new process is started and waited for) `init_process_group("nccl", device_id=...)` exactly as
    bench.py does it, barrier, all_reduce(MAX) of the f64 elapsed time, all_gather of the int64 checksum tensor and of a uint8 done
    tensor, StepGather(world=1), destroy_process_group."""
    import subprocess
    import sys
    script = tmp_path / "rccl_child.py"
    script.write_text(_RCCL_CHILD)
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29000 + os.getpid() % 2000),
               ROVER_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and "rccl world-size-1 ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
