"""GPU: rover_motion_step (csrc/rover_motion.hip) against the numpy restatement of its definition (tests/motion_ref.py) on a ctx that
holds only a heightfield — a non-square one, poses outside the map on every side, tilted quaternions —, under a tolerance measured from
the restatement's own float32 rounding; sub-steps, the joint copy, strided commands, guard rows, graph replay, every refusal of the
C ABI, the turn-on-the-spot rule on the device, and VecEnv(sim="terrain") on a task.

The tolerance: for every compared quantity, d = max |float32 restatement - float64 restatement| over the inputs of this file; the kernel
must agree with the float64 restatement within 8 d (the device's sinf / cosf / atan2f / atanf are a few ulp where numpy's are within 1),
but never less than 4 float32 ulp of the quantity's largest magnitude.  An env one of whose wheel contacts lies within 1e-3 cell of a
rounding boundary of the height lookup (|coordinate| < 7 m: one ulp is below 5e-7 m = 1e-5 cell) is left out of the z / roll / pitch /
quaternion comparison only; at most 5 % of the envs may be."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N0, N1, HSCALE, VSCALE, SHIFT = 96, 80, 0.05, 0.7, (-1.3, 0.7)
KW = dict(dt=0.05, max_lin=1.3, max_ang=0.9, ride_height=0.3)
E_MAX = 257
NEAR = 1e-3                          # cells
MAX_EXCLUDED = 0.05
EPS32 = float(np.finfo(np.float32).eps)


def make_inputs(n, seed):
    rng = np.random.default_rng(seed)
    lo = np.array([SHIFT[0] - 0.5, SHIFT[1] - 0.5])
    hi = np.array([SHIFT[0] + N0 * HSCALE + 0.5, SHIFT[1] + N1 * HSCALE + 0.5])     # 0.5 m outside the map on every side: both clamps run
    pos = np.concatenate((rng.uniform(lo, hi, (n, 2)), rng.uniform(-1, 1, (n, 1))), 1).astype(np.float32)
    quat = rng.normal(size=(n, 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)          # any unit quaternion: tilted, either sign of w
    lin, ang = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    return pos, quat, lin, ang


HEIGHTS = np.random.default_rng(7).uniform(0.0, 1.0, (N0, N1)).astype(np.float32)
INPUTS = make_inputs(E_MAX, 0)
_ref_cache = {}


def reference(rcp, substeps=1):
    """The two restatements on INPUTS, the envs near a rounding boundary and the measured d per quantity — computed once per
    (cell_index_mode, substeps) and shared."""
    key = (rcp, substeps)
    if key not in _ref_cache:
        field = R.Field(HEIGHTS, HSCALE, VSCALE, SHIFT, rcp)
        r64 = R.step(field, *INPUTS, substeps=substeps, dtype=np.float64, **KW)
        r32 = R.step(field, *INPUTS, substeps=substeps, dtype=np.float32, **KW)
        near = R.boundary_distance(field, r64["contacts"]) < NEAR
        q64, q32 = quantities(r64["pos"], r64["quat"]), quantities(r32["pos"], r32["quat"])
        d = {k: deviation(k, q32[k], q64[k], near).max(initial=0.0) for k in q64}
        _ref_cache[key] = (r64, q64, near, d)
    return _ref_cache[key]


def quantities(pos, quat):
    pos, quat = np.asarray(pos, dtype=np.float64), np.asarray(quat, dtype=np.float64)
    eul = R.quat_to_eul(quat)
    return dict(x=pos[:, 0], y=pos[:, 1], z=pos[:, 2], roll=eul[:, 0], pitch=eul[:, 1], yaw=eul[:, 2], quat=quat)


TERRAIN_DEPENDENT = ("z", "roll", "pitch", "quat")


def deviation(name, got, want, near):
    """|got - want| per env over the envs the quantity is compared on: yaw up to its wrap, the quaternion up to its sign."""
    if name == "quat":
        dev = np.minimum(np.abs(got - want).max(1), np.abs(got + want).max(1))
    else:
        dev = np.abs(got - want)
        if name == "yaw":
            dev = np.minimum(dev, np.abs(dev - 2 * np.pi))
    return dev[~near] if name in TERRAIN_DEPENDENT else dev


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
    """INPUTS' first n envs on the GPU, in tensors ``pad`` rows longer (the extra rows are other envs' data)."""
    pos, quat, lin, ang = (torch.from_numpy(np.ascontiguousarray(a[:n + pad])).to(DEV) for a in inputs)
    return pos, quat, lin, ang


def run(eng, n, substeps=1, **kw):
    pos, quat, lin, ang = dev_inputs(n)
    eng.motion_step(pos, quat, lin, ang, substeps=substeps, **dict(KW, **kw))
    torch.cuda.synchronize()
    return pos, quat


@pytest.mark.parametrize("rcp", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_against_the_restatement(eng, n, rcp):
    eng.set_option("cell_index_mode", rcp)
    assert eng.info().cell_index_mode == rcp
    r64, q64, near, d = reference(rcp)
    assert near.mean() <= MAX_EXCLUDED, f"{near.mean():.3%} of the envs lie within {NEAR} cell of a rounding boundary"
    pos, quat = run(eng, n)
    got = quantities(pos.cpu().numpy(), quat.cpu().numpy())
    assert np.abs(np.linalg.norm(got["quat"], axis=1) - 1).max() <= 1e-6
    worst = {}
    for k in q64:
        tol = max(8.0 * d[k], 4.0 * EPS32 * float(np.abs(q64[k]).max()))
        dev = deviation(k, got[k], q64[k][:n], near[:n]).max(initial=0.0)
        worst[k] = (dev, d[k], tol)
    print(f"E = {n}, cell_index_mode {rcp}, {int(near[:n].sum())} envs near a boundary; quantity: kernel's worst deviation / measured d / tolerance")
    print("  " + "  ".join(f"{k} {dev:.3e}/{dk:.3e}/{tol:.3e}" for k, (dev, dk, tol) in worst.items()))
    for k, (dev, dk, tol) in worst.items():
        assert dev <= tol, f"{k}: the kernel deviates by {dev:.3e} from the float64 restatement, tolerance {tol:.3e} (d = {dk:.3e})"


def test_heights_are_read_with_the_right_index_order(eng):
    """On this non-square map a transposed lookup or swapped clamps give another height.  The kernel's z is compared with the
    restatement's above; here the restatement's own lookup is pinned against Engine.sample_height on the wheel contacts it lists."""
    r64, _, near, _ = reference(0)
    contacts = r64["contacts"][0].reshape(-1, 2).astype(np.float32)
    h = eng.sample_height(torch.from_numpy(contacts).to(DEV)).cpu().numpy()
    field = R.Field(HEIGHTS, HSCALE, VSCALE, SHIFT, 0)
    want = field.height(contacts[:, 0], contacts[:, 1], np.dtype(np.float32))
    assert np.array_equal(h, want)
    assert len(np.unique(h)) > 300                                 # the contacts spread over the map, clamped ones included


def test_substeps_fold_bit_for_bit(eng):
    one_pos, one_quat = dev_inputs(E_MAX)[:2]
    lin, ang = dev_inputs(E_MAX)[2:]
    for _ in range(3):
        eng.motion_step(one_pos, one_quat, lin, ang, substeps=1, **KW)
    pos, quat = run(eng, E_MAX, substeps=3)
    assert torch.equal(pos, one_pos) and torch.equal(quat, one_quat)
    start = torch.from_numpy(INPUTS[0]).to(DEV)
    assert not torch.equal(pos, start)
    # and three sub-steps against the restatement, under the three-step d
    r64, q64, near, d = reference(0, substeps=3)
    assert near.mean() <= MAX_EXCLUDED
    got = quantities(pos.cpu().numpy(), quat.cpu().numpy())
    for k in q64:
        tol = max(8.0 * d[k], 4.0 * EPS32 * float(np.abs(q64[k]).max()))
        dev = deviation(k, got[k], q64[k], near).max(initial=0.0)
        print(f"3 sub-steps: {k} {dev:.3e}/{d[k]:.3e}/{tol:.3e}")
        assert dev <= tol, (k, dev, tol)


@pytest.mark.parametrize("n", [1, 5, 64, 257, 300])
def test_joint_copy_is_exact_and_optional(eng, n):
    """All 13 columns of both targets reach the state, rows past E stay; without ``joints`` nothing is touched.  n = 5, 257, 300: 13 n
    is not a multiple of 4 (the 16-byte copy's tail); 257 and 300: a second workgroup."""
    g = torch.Generator().manual_seed(n)
    inputs = make_inputs(n, seed=n)
    pad = 3
    tp, tv, jp, jv = (torch.randn(n + pad, 13, generator=g).to(DEV) for _ in range(4))
    jp0, jv0 = jp.clone(), jv.clone()
    pos, quat, lin, ang = dev_inputs(n, inputs=inputs)
    eng.motion_step(pos, quat, lin, ang, **KW)
    assert torch.equal(jp, jp0) and torch.equal(jv, jv0)
    ref_pos, ref_quat = pos.clone(), quat.clone()
    pos, quat, lin, ang = dev_inputs(n, inputs=inputs)
    eng.motion_step(pos, quat, lin, ang, joints=(tp[:n], tv[:n], jp[:n], jv[:n]), **KW)
    assert torch.equal(jp[:n], tp[:n]) and torch.equal(jv[:n], tv[:n])
    assert torch.equal(jp[n:], jp0[n:]) and torch.equal(jv[n:], jv0[n:])
    assert torch.equal(pos, ref_pos) and torch.equal(quat, ref_quat)            # the pose does not depend on the joint copy
    # unaligned bases take the scalar copy: the same result
    flat = torch.zeros(4 * (n * 13 + 1), device=DEV)
    views = [flat[i * (n * 13 + 1) + 1:(i + 1) * (n * 13 + 1)].view(n, 13) for i in range(4)]
    views[0].copy_(tp[:n]), views[1].copy_(tv[:n])
    if any(v.data_ptr() % 16 for v in views):
        pos, quat, lin, ang = dev_inputs(n, inputs=inputs)
        eng.motion_step(pos, quat, lin, ang, joints=tuple(views), **KW)
        assert torch.equal(views[2], tp[:n]) and torch.equal(views[3], tv[:n]) and torch.equal(pos, ref_pos)


def test_commands_through_a_strided_column(eng):
    n = 130
    want_pos, want_quat = run(eng, n)
    pos, quat, lin, ang = dev_inputs(n)
    lin_hist, ang_hist = torch.full((n, 3), 9.0, device=DEV), torch.full((n, 3), -9.0, device=DEV)     # newest first, like Memory.tracker
    lin_hist[:, 0], ang_hist[:, 0] = lin, ang
    assert lin_hist[:, 0].stride(0) == 3
    eng.motion_step(pos, quat, lin_hist[:, 0], ang_hist[:, 0], **KW)
    assert torch.equal(pos, want_pos) and torch.equal(quat, want_quat)


def test_in_place_and_guard_rows(eng):
    n, pad = 70, 5
    want_pos, want_quat = run(eng, n)
    pos, quat, lin, ang = dev_inputs(n, pad)
    p0, q0 = pos.clone(), quat.clone()
    ptrs = (pos.data_ptr(), quat.data_ptr())
    eng.motion_step(pos[:n], quat[:n], lin[:n], ang[:n], **KW)
    assert (pos.data_ptr(), quat.data_ptr()) == ptrs
    assert torch.equal(pos[:n], want_pos) and torch.equal(quat[:n], want_quat)
    assert torch.equal(pos[n:], p0[n:]) and torch.equal(quat[n:], q0[n:])
    # a window in the middle: the rows before it stay too (its quaternion rows start 16-byte aligned, its position rows need not)
    pos, quat, lin, ang = dev_inputs(n, pad)
    eng.motion_step(pos[3:n], quat[3:n], lin[3:n], ang[3:n], **KW)
    assert torch.equal(pos[:3], p0[:3]) and torch.equal(quat[:3], q0[:3]) and torch.equal(pos[n:], p0[n:]) and torch.equal(quat[n:], q0[n:])
    assert torch.equal(pos[3:n], want_pos[3:]) and torch.equal(quat[3:n], want_quat[3:])
    assert eng.motion_step(pos[:0], quat[:0], lin[:0], ang[:0], **KW) is None      # E = 0: nothing happens
    assert torch.equal(pos[3:n], want_pos[3:])


def test_graph_replay_gives_the_eager_bits(eng):
    n = 257
    g = torch.Generator().manual_seed(5)
    tp, tv = torch.randn(n, 13, generator=g).to(DEV), torch.randn(n, 13, generator=g).to(DEV)
    jp, jv = torch.zeros(n, 13, device=DEV), torch.zeros(n, 13, device=DEV)
    pos, quat, lin, ang = dev_inputs(n)
    eng.motion_step(pos, quat, lin, ang, substeps=2, joints=(tp, tv, jp, jv), **KW)        # the eager call (and the warm-up)
    want_pos, want_quat = pos.clone(), quat.clone()
    start = dev_inputs(n)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.motion_step(pos, quat, lin, ang, substeps=2, joints=(tp, tv, jp, jv), **KW)
    for _ in range(2):
        pos.copy_(start[0]), quat.copy_(start[1]), jp.zero_(), jv.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pos, want_pos) and torch.equal(quat, want_quat) and torch.equal(jp, tp) and torch.equal(jv, tv)


def test_turn_on_the_spot_on_the_device(eng):
    """float32 ladders of v around 0.45 w: the rover moves exactly where the float32 quotient is above float32(0.45); w = 0 keeps v,
    v = w = 0 stands still.  max_lin = max_ang = 1 so that the commands are the velocities."""
    bound, vs, ws = np.float32(0.45), [], []
    for w in np.float32([0.3, -0.3, 1.0, -0.77]):
        v = np.float32(bound * np.abs(w))
        for _ in range(4):
            v = np.nextafter(v, np.float32(0))
        for _ in range(9):
            vs += [v, -v]
            ws += [w, w]
            v = np.nextafter(v, np.float32(1))
    vs, ws = np.float32(vs + [0.5, -0.5, 0.0]), np.float32(ws + [0.0, 0.0, 0.0])
    n = len(vs)
    pos0 = np.tile(np.float32([1.0, 2.0, 0.0]), (n, 1))
    quat0 = np.tile(np.float32([1, 0, 0, 0]), (n, 1))
    pos, quat, lin, ang = (torch.from_numpy(a).to(DEV) for a in (pos0, quat0, vs, ws))
    eng.motion_step(pos, quat, lin, ang, dt=0.05)
    moved = (pos[:, :2].cpu().numpy() != pos0[:, :2]).any(1)
    want = R.effective_speed(vs, ws) != 0
    assert np.array_equal(moved, want) and want[:-3].any() and not want[:-3].all()
    assert list(moved[-3:]) == [True, True, False]


def test_refusals_through_the_c_abi(eng):
    """Every refusal of rover_motion_step on a live ctx, with poisoned poses that no launch may touch; then the Python layer's own."""
    from isaac_rover_amd import _lib
    from isaac_rover_amd._lib import RoverError
    n = 8
    pos, quat, lin, ang = dev_inputs(n)
    jt = [torch.zeros(n, 13, device=DEV) for _ in range(4)]
    p0, q0 = pos.clone(), quat.clone()
    base = dict(pos3=pos.data_ptr(), quat4=quat.data_ptr(), lin=lin.data_ptr(), ang=ang.data_ptr(), cmd_stride=1)
    names = ("joint_pos_targets13", "joint_vel_targets13", "joint_pos13", "joint_vel13")

    def call(ctx, e=n, **kw):
        d = _lib.motion_desc(e, **dict(base, **kw))
        rc = ctx.lib.rover_motion_step(ctx._h, C.byref(d), None)
        return rc, ctx.lib.rover_last_error(ctx._h).decode()

    bad = [dict(e=-1), dict(substeps=0), dict(substeps=-2), dict(cmd_stride=0), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")),
           dict(pos3=None), dict(quat4=None), dict(lin=None), dict(ang=None)]
    bad += [{k: jt[i].data_ptr() for i, k in enumerate(names) if mask >> i & 1} for mask in range(1, 15)]
    for kw in bad:
        rc, msg = call(eng, **kw)
        assert rc == -1 and msg.startswith("motion_step:"), (kw, rc, msg)
    assert eng.lib.rover_motion_step(eng._h, None, None) == -1
    bare = _lib.Engine(8, device=0)                                # no heightfield: ROVER_E_STATE, also with E = 0
    try:
        for e in (n, 0):
            rc, msg = call(bare, e=e)
            assert rc == -2 and "rover_set_heightfield" in msg, (rc, msg)
        with pytest.raises(RoverError, match="rover_set_heightfield"):
            bare.motion_step(pos, quat, lin, ang, **KW)
    finally:
        bare.close()
    assert call(eng, e=0)[0] == 0                                  # E = 0 with a heightfield: ROVER_OK
    assert call(eng, e=0, pos3=None, quat4=None, lin=None, ang=None)[0] == 0
    torch.cuda.synchronize()
    assert torch.equal(pos, p0) and torch.equal(quat, q0) and not any(bool(t.any()) for t in jt)      # none of them launched
    # the binding's checks
    for kw in (dict(pos=pos.double()), dict(pos=pos.cpu()), dict(pos=pos[:, :2]), dict(quat=quat[:4]), dict(lin=lin[:4]), dict(ang=ang.double()),
               dict(lin=lin.cpu()), dict(lin=torch.zeros(n, 2, device=DEV)[:, 0]), dict(joints=(jt[0], jt[1], jt[2])),
               dict(joints=(jt[0], jt[1], jt[2], None)), dict(joints=(jt[0], jt[1], jt[2], jt[3][:4])), dict(dt=0.0), dict(substeps=0)):
        args = dict(pos=pos, quat=quat, lin=lin, ang=ang, dt=0.05)
        args.update(kw)
        with pytest.raises(RoverError):
            eng.motion_step(args.pop("pos"), args.pop("quat"), args.pop("lin"), args.pop("ang"), **args)
    torch.cuda.synchronize()
    assert torch.equal(pos, p0) and torch.equal(quat, q0)


def test_task_with_the_terrain_sim():
    """VecEnv(sim="terrain") on a task: after 20 steps of a fixed forward command some rover is tilted and the joint state equals the
    steering targets — both impossible with KinematicSim, which writes level quaternions and no joint state."""
    from isaac_rover_amd import synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.tasks.rover import RoverTask
    from isaac_rover_amd.vec_env import TerrainSim, VecEnv
    e = 64
    scene = synth.make_scene(n_cells=128, k=16, n_stones=10)
    env = VecEnv(headless=True, sim="terrain")
    task = RoverTask("Rover", SimConfig(num_envs=e, device=DEV), env, scene=scene, distribution=synth.ray_distribution("37"))
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(e, 3)
    spawn[:, 0:2] = 0.15 * 12.8 + 0.7 * 12.8 * torch.rand(e, 2, generator=g)
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    assert isinstance(env._world, TerrainSim)
    obs = env.reset()
    actions = torch.tensor([[0.8, 0.25]], device=DEV).repeat(e, 1)              # forward and a gentle left turn: |v / w| = 3.2
    for _ in range(20):
        obs, rew, done, info = env.step(actions)
    assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
    pos, quat = task._rover.get_world_poses()
    eul = task._engine.quat_to_euler(quat.contiguous())
    assert float(eul[:, :2].abs().max()) > 1e-3                                  # some rover is tilted
    assert float((quat.norm(dim=1) - 1).abs().max()) <= 1e-5
    assert torch.equal(task._rover.get_joint_positions(), task._rover._joint_pos_targets)
    assert torch.equal(task._rover.get_joint_velocities(), task._rover._joint_vel_targets)
    steer = task._rover.get_joint_positions()[:, task._rover.actuated_pos_indices]
    assert bool((steer != 0).any())                                            # and the steering joints did turn
    env.close()
