"""GPU: rover_motion_step_bogie (csrc/rover_motion.hip) against the numpy restatement of its definition (tests/bogie_ref.py), in the
pattern of tests/test_motion_gpu.py and on its map and inputs — at a vertical scale of 0.1, where the wheel-height differences stay
inside the chord iteration's range (angles up to 0.30 rad) —; sub-steps, the clamp, the joint rows, graph replay, strided commands,
VecEnv(sim="terrain", suspension="bogie") on a task, and the plane mode's bits behind the new keyword.

The tolerance is test_motion_gpu's: for every compared quantity, d = max |float32 restatement - float64 restatement| over the inputs of
this file; the kernel must agree with the float64 restatement within 8 d, but never less than 4 float32 ulp of the quantity's largest
magnitude.  An env one of whose wheel contacts lies within 1e-3 cell of a rounding boundary of the height lookup is left out of the
terrain-dependent quantities (z, roll, pitch, the quaternion and the three joints) only; at most 5 % of the envs may be (1.6 % are)."""
import numpy as np
import pytest
import torch

import bogie_ref as B
import motion_ref as R
from test_motion_gpu import E_MAX, EPS32, HEIGHTS, HSCALE, INPUTS, KW, MAX_EXCLUDED, NEAR, SHIFT, deviation, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VSCALE = 0.1
BOGIE = dict(KW, suspension="bogie")
_ref_cache = {}


def quantities(pos, quat, joints):
    pos, quat, joints = (np.asarray(a, dtype=np.float64) for a in (pos, quat, joints))
    eul = R.quat_to_eul(quat)
    return dict(x=pos[:, 0], y=pos[:, 1], z=pos[:, 2], roll=eul[:, 0], pitch=eul[:, 1], yaw=eul[:, 2], quat=quat,
                j0=joints[:, 0], j1=joints[:, 1], j2=joints[:, 2])


def dev_of(name, got, want, near):
    """test_motion_gpu.deviation, with the joints among the terrain-dependent quantities."""
    dev = deviation(name, got, want, near)
    return dev[~near] if name in ("j0", "j1", "j2") else dev


def reference(rcp):
    """The two restatements on INPUTS at one sub-step, the envs near a rounding boundary and the measured d per quantity — computed
    once per cell_index_mode and shared."""
    if rcp not in _ref_cache:
        field = R.Field(HEIGHTS, HSCALE, VSCALE, SHIFT, rcp)
        r64 = B.step(field, *INPUTS, dtype=np.float64, **KW)
        r32 = B.step(field, *INPUTS, dtype=np.float32, **KW)
        near = R.boundary_distance(field, r64["contacts"]) < NEAR
        q64, q32 = quantities(r64["pos"], r64["quat"], r64["joints"]), quantities(r32["pos"], r32["quat"], r32["joints"])
        d = {k: dev_of(k, q32[k], q64[k], near).max(initial=0.0) for k in q64}
        _ref_cache[rcp] = (r64, q64, near, d)
    return _ref_cache[rcp]


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    e.set_heightfield(HEIGHTS, HSCALE, VSCALE, SHIFT)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def default_cell_index_mode(eng):
    yield
    eng.set_option("cell_index_mode", 0)


def dev_inputs(n, pad=0, inputs=INPUTS):
    return tuple(torch.from_numpy(np.ascontiguousarray(a[:n + pad])).to(DEV) for a in inputs)


def joint_tensors(n, pad=0, seed=0):
    """Targets with garbage in EVERY column (0-2 included), a state full of another garbage, `pad` guard rows."""
    g = torch.Generator().manual_seed(1000 + seed)
    tp, tv, jp, jv = (torch.randn(n + pad, 13, generator=g).to(DEV) for _ in range(4))
    return tp, tv, jp, jv


def run(eng, n, substeps=1, **kw):
    """-> pos, quat, joint_pos [n, 13] after one call on INPUTS' first n envs, and the targets it was given."""
    pos, quat, lin, ang = dev_inputs(n)
    tp, tv, jp, jv = joint_tensors(n)
    eng.motion_step(pos, quat, lin, ang, substeps=substeps, joints=(tp, tv, jp, jv), **dict(BOGIE, **kw))
    torch.cuda.synchronize()
    return pos, quat, jp, (tp, tv, jv)


@pytest.mark.parametrize("rcp", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_against_the_restatement(eng, n, rcp):
    eng.set_option("cell_index_mode", rcp)
    assert eng.info().cell_index_mode == rcp
    r64, q64, near, d = reference(rcp)
    assert near.mean() <= MAX_EXCLUDED, f"{near.mean():.3%} of the envs lie within {NEAR} cell of a rounding boundary"
    assert r64["residual"].max() <= 1e-6 and np.abs(r64["joints_raw"]).max() < B.MAX_BOGIE       # converged, and nothing is clamped
    pos, quat, jp, _ = run(eng, n)
    got = quantities(pos.cpu().numpy(), quat.cpu().numpy(), jp[:, 0:3].cpu().numpy())
    assert np.abs(np.linalg.norm(got["quat"], axis=1) - 1).max() <= 1e-6
    worst = {}
    for k in q64:
        tol = max(8.0 * d[k], 4.0 * EPS32 * float(np.abs(q64[k]).max()))
        dev = dev_of(k, got[k], q64[k][:n], near[:n]).max(initial=0.0)
        worst[k] = (dev, d[k], tol)
    print(f"E = {n}, cell_index_mode {rcp}, {int(near[:n].sum())} envs near a boundary; quantity: kernel's worst deviation / measured d / tolerance")
    print("  " + "  ".join(f"{k} {dev:.3e}/{dk:.3e}/{tol:.3e}" for k, (dev, dk, tol) in worst.items()))
    for k, (dev, dk, tol) in worst.items():
        assert dev <= tol, f"{k}: the kernel deviates by {dev:.3e} from the float64 restatement, tolerance {tol:.3e} (d = {dk:.3e})"


def test_substeps_fold_bit_for_bit(eng):
    pos1, quat1, lin, ang = dev_inputs(E_MAX)
    tp, tv, jp1, jv1 = joint_tensors(E_MAX)
    for _ in range(3):
        eng.motion_step(pos1, quat1, lin, ang, substeps=1, joints=(tp, tv, jp1, jv1), **BOGIE)
    pos, quat, jp, _ = run(eng, E_MAX, substeps=3)
    assert torch.equal(pos, pos1) and torch.equal(quat, quat1) and torch.equal(jp, jp1)
    assert not torch.equal(pos, torch.from_numpy(INPUTS[0]).to(DEV))
    one = run(eng, E_MAX)
    assert not torch.equal(one[0], pos) and not torch.equal(one[2][:, 0:3], jp[:, 0:3])          # and three steps are not one


def test_the_clamp_acts_on_the_joints_alone(eng):
    lim = 0.25
    pos, quat, jp, _ = run(eng, E_MAX)
    cpos, cquat, cjp, _ = run(eng, E_MAX, max_bogie=lim)
    assert torch.equal(cpos, pos) and torch.equal(cquat, quat)                 # the pose is not re-solved
    j, cj = jp[:, 0:3], cjp[:, 0:3]
    over = j.abs() > lim
    share = float(over.any(1).float().mean())
    print(f"{share:.2%} of the envs have a joint beyond {lim} rad")
    assert 0 < int(over.any(1).sum()) < E_MAX // 4                               # some envs, not all (1.6 % in the restatement)
    lim32 = torch.tensor(lim, dtype=torch.float32, device=DEV)
    assert torch.equal(cj[over], torch.where(j[over] > 0, lim32, -lim32))       # exactly +-0.25f
    assert torch.equal(cj[~over], j[~over])                                     # every other joint keeps its bits
    assert torch.equal(cjp[:, 3:], jp[:, 3:])


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_joint_rows(eng, n, aligned):
    """Columns 3-12 of joint_pos and all of joint_vel become the targets bit for bit; columns 0-2 hold the solve whatever the targets
    hold there; the guard rows after E stay; without the quadruple only the pose is written.  255, 256, 257: one short of a workgroup,
    exactly one, one more; the misaligned bases take the 4-byte copy."""
    pad = 3
    inputs = make_inputs(n, seed=n)
    if aligned:
        tp, tv, jp, jv = joint_tensors(n, pad, seed=n)
    else:
        flat = torch.randn(4 * ((n + pad) * 13 + 1), generator=torch.Generator().manual_seed(n)).to(DEV)
        stride = (n + pad) * 13 + 1
        tp, tv, jp, jv = (flat[i * stride + 1:(i + 1) * stride].view(n + pad, 13) for i in range(4))
        assert any(t.data_ptr() % 16 for t in (tp, tv, jp, jv))
    jp0, jv0, tp0, tv0 = jp.clone(), jv.clone(), tp.clone(), tv.clone()
    pos, quat, lin, ang = dev_inputs(n, inputs=inputs)
    eng.motion_step(pos, quat, lin, ang, **BOGIE)                                # no quadruple: the pose alone
    assert torch.equal(jp, jp0) and torch.equal(jv, jv0)
    ref_pos, ref_quat = pos.clone(), quat.clone()
    assert not torch.equal(ref_pos, torch.from_numpy(inputs[0]).to(DEV))
    pos, quat, lin, ang = dev_inputs(n, inputs=inputs)
    eng.motion_step(pos, quat, lin, ang, joints=(tp[:n], tv[:n], jp[:n], jv[:n]), **BOGIE)
    torch.cuda.synchronize()
    assert torch.equal(pos, ref_pos) and torch.equal(quat, ref_quat)            # the pose does not depend on the joint rows
    assert torch.equal(tp, tp0) and torch.equal(tv, tv0)                        # the targets are only read
    assert torch.equal(jp[:n, 3:], tp[:n, 3:]) and torch.equal(jv[:n], tv[:n])
    assert torch.equal(jp[n:], jp0[n:]) and torch.equal(jv[n:], jv0[n:])        # guard rows
    # columns 0-2: the solve, not the targets' garbage — the same bits whatever the targets and the alignment
    tp2, tv2, jp2, jv2 = joint_tensors(n, seed=n + 7)
    pos, quat, lin, ang = dev_inputs(n, inputs=inputs)
    eng.motion_step(pos, quat, lin, ang, joints=(tp2, tv2, jp2, jv2), **BOGIE)
    assert torch.equal(jp[:n, 0:3], jp2[:, 0:3]) and not torch.equal(jp2[:, 0:3], tp2[:, 0:3])
    assert float(jp[:n, 0:3].abs().max()) <= float(np.float32(B.MAX_BOGIE)) and (n == 1 or bool((jp[:n, 0:3] != 0).any()))


def test_graph_replay_and_a_strided_command_column(eng):
    n = 257
    want_pos, want_quat, want_jp, (tp, tv, _) = run(eng, n, substeps=2)
    pos, quat, lin, ang = dev_inputs(n)
    jp, jv = torch.zeros(n, 13, device=DEV), torch.zeros(n, 13, device=DEV)
    lin_hist, ang_hist = torch.full((n, 3), 9.0, device=DEV), torch.full((n, 3), -9.0, device=DEV)     # newest first, like the task's histories
    lin_hist[:, 0], ang_hist[:, 0] = lin, ang
    assert lin_hist[:, 0].stride(0) == 3
    eng.motion_step(pos, quat, lin_hist[:, 0], ang_hist[:, 0], substeps=2, joints=(tp, tv, jp, jv), **BOGIE)      # eager, strided (and the warm-up)
    assert torch.equal(pos, want_pos) and torch.equal(quat, want_quat) and torch.equal(jp, want_jp) and torch.equal(jv, tv)
    start = dev_inputs(n)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.motion_step(pos, quat, lin_hist[:, 0], ang_hist[:, 0], substeps=2, joints=(tp, tv, jp, jv), **BOGIE)
    for _ in range(2):
        pos.copy_(start[0]), quat.copy_(start[1]), jp.zero_(), jv.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pos, want_pos) and torch.equal(quat, want_quat) and torch.equal(jp, want_jp) and torch.equal(jv, tv)


def test_in_place_guard_rows_and_refusals(eng):
    """A window of a longer tensor: the rows around it stay.  E = 0 does nothing.  The parameters' refusals reach Python as RoverError
    and launch nothing; a ctx without a heightfield is ROVER_E_STATE."""
    from isaac_rover_amd import _lib
    from isaac_rover_amd._lib import RoverError
    n, pad = 70, 5
    want_pos, want_quat, _, _ = run(eng, n)
    pos, quat, lin, ang = dev_inputs(n, pad)
    p0, q0 = pos.clone(), quat.clone()
    eng.motion_step(pos[3:n], quat[3:n], lin[3:n], ang[3:n], **BOGIE)
    assert torch.equal(pos[:3], p0[:3]) and torch.equal(quat[:3], q0[:3]) and torch.equal(pos[n:], p0[n:]) and torch.equal(quat[n:], q0[n:])
    assert torch.equal(pos[3:n], want_pos[3:]) and torch.equal(quat[3:n], want_quat[3:])
    assert eng.motion_step(pos[:0], quat[:0], lin[:0], ang[:0], **BOGIE) is None
    pos, quat, lin, ang = dev_inputs(n)
    p0, q0 = pos.clone(), quat.clone()
    for kw in (dict(iters=0), dict(iters=9), dict(max_bogie=0.0), dict(max_bogie=-1.0), dict(max_bogie=float("nan")), dict(max_bogie=float("inf")),
               dict(suspension="rigid"), dict(dt=0.0), dict(substeps=0)):
        with pytest.raises(RoverError):
            eng.motion_step(pos, quat, lin, ang, **dict(BOGIE, **kw))
    bare = _lib.Engine(8, device=0)
    try:
        with pytest.raises(RoverError, match="rover_set_heightfield"):
            bare.motion_step(pos, quat, lin, ang, **BOGIE)
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert torch.equal(pos, p0) and torch.equal(quat, q0)


def test_the_plane_mode_is_untouched(eng):
    """Engine.motion_step without ``suspension`` gives the bits of suspension="plane" — pose and joint state, iters and max_bogie not
    read —, and they are not the bogie mode's."""
    n = E_MAX
    out = []
    for kw in ({}, dict(suspension="plane"), dict(suspension="plane", iters=99, max_bogie=-1.0), dict(suspension="bogie")):
        pos, quat, lin, ang = dev_inputs(n)
        tp, tv, jp, jv = joint_tensors(n)
        eng.motion_step(pos, quat, lin, ang, substeps=2, joints=(tp, tv, jp, jv), **dict(KW, **kw))
        out.append((pos, quat, jp, jv))
        if kw.get("suspension") != "bogie":
            assert torch.equal(jp, tp) and torch.equal(jv, tv)                  # all 13 columns, as ever
    for other in out[1:3]:
        assert all(torch.equal(a, b) for a, b in zip(out[0], other))
    assert not torch.equal(out[0][0], out[3][0]) and not torch.equal(out[0][2], out[3][2])


def _task_run(suspension, steps=20):
    from isaac_rover_amd import synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.tasks.rover import RoverTask
    from isaac_rover_amd.vec_env import TerrainSim, VecEnv
    e = 64
    scene = synth.make_scene(n_cells=128, k=16, n_stones=10)
    env = VecEnv(headless=True, sim="terrain", suspension=suspension)
    task = RoverTask("Rover", SimConfig(num_envs=e, device=DEV), env, scene=scene, distribution=synth.ray_distribution("37"))
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(e, 3)
    spawn[:, 0:2] = 0.15 * 12.8 + 0.7 * 12.8 * torch.rand(e, 2, generator=g)
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    assert isinstance(env._world, TerrainSim) and env._world.suspension == suspension
    env.reset()
    actions = torch.tensor([[0.8, 0.25]], device=DEV).repeat(e, 1)
    scale = torch.tensor(task.rew_scales["boogie_contraint_reward"], dtype=torch.float32, device=DEV)
    assert float(scale) == 0.5
    seen = []
    for _ in range(steps):
        obs, rew, done, extras = env.step(actions)
        # resets happen in the NEXT pre_physics_step: the joint state is still the one this step read
        j = task._rover.get_joint_positions()[:, 0:3].abs()
        want = ((j[:, 0] + j[:, 1]) + j[:, 2]) * scale
        assert torch.equal(extras["uprightness_penalty"], want)
        assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
        seen.append(extras["uprightness_penalty"].clone())
    jp = task._rover.get_joint_positions()
    assert torch.equal(jp[:, 3:], task._rover._joint_pos_targets[:, 3:])
    assert torch.equal(task._rover.get_joint_velocities(), task._rover._joint_vel_targets)
    quat = task._rover.get_world_poses()[1]
    assert float((quat.norm(dim=1) - 1).abs().max()) <= 1e-5
    env.close()
    return torch.stack(seen)


def test_the_task_sees_the_bogie_joints():
    """RoverTask at 64 envs on the synth scene for 20 steps: with suspension="bogie" the uprightness penalty is
    boogie_contraint_reward * (|j0| + |j1| + |j2|) of the joint state the step read, bit for bit, and not 0; with "plane" it is
    exactly 0 everywhere, as it has always been.  This test fails without the posture mode."""
    bogie = _task_run("bogie")
    assert bool((bogie != 0).any()) and float(bogie.abs().max()) <= 0.5 * 3 * 0.6
    plane = _task_run("plane")
    assert not bool((plane != 0).any())
