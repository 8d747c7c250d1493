"""GPU: rover_motion_step_drive (csrc/rover_motion.hip) against the numpy restatement of its definition (tests/drive_ref.py) on the
96 x 80 heightfield of tests/test_motion_gpu.py (at the bogie test's vertical scale, so that both postures are meaningful): pose and slip
under a tolerance measured from the restatement's own float32 rounding, the actuated joint columns bit for bit, both suspensions,
sub-steps, unaligned buffers, graph replay, NaN isolation, the command mode's pose on level ground, and VecEnv(drive="wheels") on a task.

The tolerance is test_motion_gpu's: for every compared quantity, d = max |float32 restatement - float64 restatement| over the inputs of
this file; the kernel must agree with the float64 restatement within 8 d, but never less than 4 float32 ulp of the quantity's largest
magnitude.  An env one of whose wheel contacts lies within 1e-3 cell of a rounding boundary of the height lookup is left out of the
z / roll / pitch / quaternion (and, with the bogie, passive joint) comparison only; at most 5 % of the envs may be.  The rate limiter is
adds and compares only, so the steering and drive columns are compared with the float32 restatement bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import drive_ref as D
import metrics_ref as A
import motion_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N0, N1, HSCALE, VSCALE, SHIFT = 96, 80, 0.05, 0.1, (-1.3, 0.7)
DT, RIDE = 0.05, 0.3
E_MAX = 333
NEAR, MAX_EXCLUDED = 1e-3, 0.05
EPS32 = float(np.finfo(np.float32).eps)
HEIGHTS = np.random.default_rng(7).uniform(0.0, 1.0, (N0, N1)).astype(np.float32)
# (steer_rate rad/s, wheel_accel rad/s^2, substeps): ideal actuators; slow ones, every state many sub-steps short of its target; a
# steering step of 0.3 rad, which some states reach within and others do not, with ideal wheel drives
RATES = {"ideal": (math.inf, math.inf, 1), "slow": (0.5, 4.0, 2), "mixed": (6.0, math.inf, 2)}
ACTUATED_POS, ACTUATED_VEL = list(D.STEERED), list(D.DRIVE_COLS)


def make_inputs(n, seed):
    """Poses as tests/test_motion_gpu.py draws them (0.5 m outside the map on every side, any unit quaternion); joint targets from
    Ackermann on random commands, with random passive columns so that their copy shows; joint states anywhere in their ranges."""
    rng = np.random.default_rng(seed)
    lo = np.array([SHIFT[0] - 0.5, SHIFT[1] - 0.5])
    hi = np.array([SHIFT[0] + N0 * HSCALE + 0.5, SHIFT[1] + N1 * HSCALE + 0.5])
    pos = np.concatenate((rng.uniform(lo, hi, (n, 2)), rng.uniform(-1, 1, (n, 1))), 1).astype(np.float32)
    quat = rng.normal(size=(n, 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
    steer, vel, _ = A.ackermann(rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32))
    pt, vt = rng.uniform(-0.2, 0.2, (n, 13)).astype(np.float32), rng.uniform(-0.2, 0.2, (n, 13)).astype(np.float32)
    for i in range(6):
        if D.STEER_COLS[i] is not None:
            pt[:, D.STEER_COLS[i]] = steer[:, i]
        vt[:, D.DRIVE_COLS[i]] = vel[:, i]
    jp, jv = rng.uniform(-1.5, 1.5, (n, 13)).astype(np.float32), rng.uniform(-5, 5, (n, 13)).astype(np.float32)
    return pos, quat, pt, vt, jp, jv


INPUTS = make_inputs(E_MAX, 5)            # the seed: the restatement alone leaves out at most 3.6 % of the envs in every configuration below
_ref_cache = {}


def kwargs(rates, suspension):
    steer_rate, accel, substeps = RATES[rates]
    return dict(dt=DT, ride_height=RIDE, substeps=substeps, steer_rate=steer_rate, wheel_accel=accel, suspension=suspension)


def quantities(out):
    pos, quat = np.asarray(out["pos"], dtype=np.float64), np.asarray(out["quat"], dtype=np.float64)
    eul = R.quat_to_eul(quat)
    q = dict(x=pos[:, 0], y=pos[:, 1], z=pos[:, 2], roll=eul[:, 0], pitch=eul[:, 1], yaw=eul[:, 2], quat=quat, slip=np.asarray(out["slip"], dtype=np.float64))
    if "bogie" in out:
        q["bogie"] = np.asarray(out["bogie"], dtype=np.float64)
    return q


TERRAIN_DEPENDENT = ("z", "roll", "pitch", "quat", "bogie")


def deviation(name, got, want, near):
    if name == "quat":
        dev = np.minimum(np.abs(got - want).max(1), np.abs(got + want).max(1))
    elif name == "bogie":
        dev = np.abs(got - want).max(1)
    else:
        dev = np.abs(got - want)
        if name == "yaw":
            dev = np.minimum(dev, np.abs(dev - 2 * np.pi))
    return dev[~near] if name in TERRAIN_DEPENDENT else dev


def restate(inputs, rates, suspension, rcp, dtype):
    field = R.Field(HEIGHTS, HSCALE, VSCALE, SHIFT, rcp)
    out = D.step(field, inputs[0], inputs[1], inputs[2:6], dtype=dtype, **kwargs(rates, suspension))
    if suspension == "bogie":
        out["bogie"] = out["joint_pos"][:, 0:3]
    return field, out


def reference(rates, suspension, rcp=0):
    """The two restatements on INPUTS, the envs near a rounding boundary and the measured d per quantity — once per configuration."""
    key = (rates, suspension, rcp)
    if key not in _ref_cache:
        field, r64 = restate(INPUTS, rates, suspension, rcp, np.float64)
        _, r32 = restate(INPUTS, rates, suspension, rcp, np.float32)
        near = R.boundary_distance(field, r64["contacts"]) < NEAR
        q64, q32 = quantities(r64), quantities(r32)
        d = {k: deviation(k, q32[k], q64[k], near).max(initial=0.0) for k in q64}
        _ref_cache[key] = (r64, r32, q64, near, d)
    return _ref_cache[key]


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


def dev_inputs(n, inputs=INPUTS):
    return [torch.from_numpy(np.ascontiguousarray(a[:n])).to(DEV) for a in inputs]


def run(eng, n, rates, suspension, inputs=INPUTS, slip=True, **over):
    """The kernel on the first n envs -> (pos, quat, joint_pos, joint_vel, slip), on the device."""
    pos, quat, pt, vt, jp, jv = dev_inputs(n, inputs)
    sl = torch.full((n,), -1.0, device=DEV) if slip else None
    eng.motion_step(pos, quat, None, None, joints=(pt, vt, jp, jv), drive="wheels", slip=sl, **dict(kwargs(rates, suspension), **over))
    torch.cuda.synchronize()
    return pos, quat, jp, jv, sl


def check(got, n, ref, label):
    """Pose, slip and (bogie) passive joints against the float64 restatement under the measured tolerance; the joint columns bit for bit."""
    r64, r32, q64, near, d = ref
    assert near.mean() <= MAX_EXCLUDED, f"{near.mean():.3%} of the envs lie within {NEAR} cell of a rounding boundary"
    pos, quat, jp, jv, sl = (t.cpu().numpy() for t in got)
    out = dict(pos=pos, quat=quat, slip=sl)
    if "bogie" in q64:
        out["bogie"] = jp[:, 0:3]
    q = quantities(out)
    assert np.abs(np.linalg.norm(q["quat"], axis=1) - 1).max() <= 1e-6
    worst = {}
    for k in q64:
        tol = max(8.0 * d[k], 4.0 * EPS32 * float(np.abs(q64[k]).max()))
        worst[k] = (deviation(k, q[k], q64[k][:n], near[:n]).max(initial=0.0), d[k], tol)
    print(f"{label}, E = {n}, {int(near[:n].sum())} envs near a boundary; quantity: kernel's worst deviation / measured d / tolerance")
    print("  " + "  ".join(f"{k} {dev:.3e}/{dk:.3e}/{tol:.3e}" for k, (dev, dk, tol) in worst.items()))
    for k, (dev, dk, tol) in worst.items():
        assert dev <= tol, f"{k}: the kernel deviates by {dev:.3e} from the float64 restatement, tolerance {tol:.3e} (d = {dk:.3e})"
    # the actuated columns: the float32 restatement's bits; every other column of 3-12 (and 0-2 in the plane mode) the targets' bits
    want_p, want_v = r32["joint_pos"][:n], r32["joint_vel"][:n]
    assert np.array_equal(jp[:, ACTUATED_POS].view(np.uint32), want_p[:, ACTUATED_POS].view(np.uint32))
    assert np.array_equal(jv[:, ACTUATED_VEL].view(np.uint32), want_v[:, ACTUATED_VEL].view(np.uint32))
    first = 3 if "bogie" in q64 else 0
    assert np.array_equal(jp[:, first:].view(np.uint32), want_p[:, first:].view(np.uint32))
    assert np.array_equal(jv.view(np.uint32), want_v.view(np.uint32))
    assert np.array_equal(jv[:, 0:3], INPUTS[3][:n, 0:3]) and np.array_equal(jp[:, [3, 5, 9]], INPUTS[2][:n][:, [3, 5, 9]])


@pytest.mark.parametrize("rates", list(RATES))
@pytest.mark.parametrize("suspension", ["plane", "bogie"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 333])
def test_against_the_restatement(eng, n, suspension, rates):
    ref = reference(rates, suspension)
    got = run(eng, n, rates, suspension)
    check(got, n, ref, f"{suspension}, {rates}")
    r32 = ref[1]
    if rates == "slow":             # many sub-steps short: hardly a state is at its target yet, and the bogie's joints are live meanwhile
        assert np.mean(r32["joint_pos"][:, ACTUATED_POS] == INPUTS[2][:, ACTUATED_POS]) < 0.15
        assert np.mean(r32["joint_vel"][:, ACTUATED_VEL] == INPUTS[3][:, ACTUATED_VEL]) < 0.15
        if suspension == "bogie":
            assert np.abs(r32["joint_pos"][:, 0:3]).max() > 0.05
    if rates == "mixed":
        landed = r32["joint_pos"][:, ACTUATED_POS] == INPUTS[2][:, ACTUATED_POS]
        assert 0.1 < landed.mean() < 0.9
    if rates == "ideal":
        assert np.array_equal(r32["joint_pos"][:, ACTUATED_POS], INPUTS[2][:, ACTUATED_POS])


@pytest.mark.parametrize("suspension", ["plane", "bogie"])
def test_the_reciprocal_cell_index_mode(eng, suspension):
    eng.set_option("cell_index_mode", 1)
    assert eng.info().cell_index_mode == 1
    check(run(eng, E_MAX, "mixed", suspension), E_MAX, reference("mixed", suspension, rcp=1), f"{suspension}, cell_index_mode 1")


@pytest.mark.parametrize("suspension", ["plane", "bogie"])
def test_substeps_fold_bit_for_bit(eng, suspension):
    """substeps = 4 gives the bits of four calls: pose, joint state and slip (the last sub-step's)."""
    n = E_MAX
    pos, quat, pt, vt, jp, jv = dev_inputs(n)
    sl = torch.zeros(n, device=DEV)
    kw = dict(kwargs("slow", suspension), substeps=1)
    for _ in range(4):
        eng.motion_step(pos, quat, None, None, joints=(pt, vt, jp, jv), drive="wheels", slip=sl, **kw)
    got = run(eng, n, "slow", suspension, substeps=4)
    for a, b in zip(got, (pos, quat, jp, jv, sl)):
        assert torch.equal(a, b)
    assert not torch.equal(pos, torch.from_numpy(INPUTS[0]).to(DEV)) and float(sl.max()) > 0


@pytest.mark.parametrize("suspension", ["plane", "bogie"])
@pytest.mark.parametrize("n", [5, 257, 333])
def test_unaligned_buffers_give_the_same_bits(eng, n, suspension):
    """Joint arrays whose bases are offset by one float take the scalar staging path; rows past E stay.  13 n is no multiple of 4 at
    these n: the vector path's tail runs too."""
    pad = 3
    want = run(eng, n, "mixed", suspension)
    guard = lambda t: torch.cat((t, torch.full((pad,) + tuple(t.shape[1:]), 7.0, device=DEV)))         # rows of other envs behind the n
    pos, quat, pt, vt, jp, jv = (guard(t) for t in dev_inputs(n))
    slot = -(-(n + pad) * 13 // 4) * 4 + 4
    flat = torch.zeros(4 * slot, device=DEV)
    views = [flat[i * slot + 1:][:(n + pad) * 13].view(n + pad, 13) for i in range(4)]
    assert all(v.data_ptr() % 16 == 4 for v in views)
    for v, src in zip(views, (pt, vt, jp, jv)):
        v.copy_(src)
    sl = torch.zeros(n, device=DEV)
    eng.motion_step(pos[:n], quat[:n], None, None, joints=tuple(v[:n] for v in views), drive="wheels", slip=sl, **kwargs("mixed", suspension))
    assert torch.equal(pos[:n], want[0]) and torch.equal(quat[:n], want[1]) and torch.equal(views[2][:n], want[2]) and torch.equal(views[3][:n], want[3])
    assert torch.equal(sl, want[4])
    assert torch.equal(views[2][n:], jp[n:]) and torch.equal(views[3][n:], jv[n:]) and torch.equal(views[0], pt) and torch.equal(views[1], vt)
    assert bool((pos[n:] == 7.0).all()) and bool((quat[n:] == 7.0).all())
    # aligned arrays with guard rows: the vector path leaves the rows past E alone as well
    pos, quat, pt, vt, jp, jv = (guard(t) for t in dev_inputs(n))
    eng.motion_step(pos[:n], quat[:n], None, None, joints=(pt[:n], vt[:n], jp[:n], jv[:n]), drive="wheels", **kwargs("mixed", suspension))
    assert torch.equal(jp[:n], want[2]) and torch.equal(jv[:n], want[3]) and bool((jp[n:] == 7.0).all()) and bool((jv[n:] == 7.0).all())
    assert torch.equal(pos[:n], want[0]) and bool((pos[n:] == 7.0).all())


def test_graph_replay_gives_the_eager_bits(eng):
    n = 257
    want = run(eng, n, "slow", "bogie")
    start = dev_inputs(n)
    pos, quat, pt, vt, jp, jv = dev_inputs(n)
    sl = torch.zeros(n, device=DEV)
    kw = kwargs("slow", "bogie")
    eng.motion_step(pos, quat, None, None, joints=(pt, vt, jp, jv), drive="wheels", slip=sl, **kw)          # warm-up
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.motion_step(pos, quat, None, None, joints=(pt, vt, jp, jv), drive="wheels", slip=sl, **kw)
    for _ in range(2):
        pos.copy_(start[0]), quat.copy_(start[1]), jp.copy_(start[4]), jv.copy_(start[5]), sl.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(want, (pos, quat, jp, jv, sl)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("suspension", ["plane", "bogie"])
def test_a_nan_target_stays_in_its_env(eng, suspension):
    """NaN steering and speed targets in envs 3, 255 and 256: every other env keeps its bits; the three envs' poses are not finite,
    with finite rates as with ideal ones."""
    n, bad = 300, [3, 255, 256]
    for rates in ("ideal", "slow"):
        want = run(eng, n, rates, suspension)
        inputs = [a.copy() for a in INPUTS]
        inputs[2][bad[0], 4] = np.nan
        inputs[3][bad[1], 10] = np.nan
        inputs[2][bad[2], 7], inputs[3][bad[2], 3] = np.nan, np.nan
        got = run(eng, n, rates, suspension, inputs=inputs)
        keep = np.ones(n, dtype=bool)
        keep[bad] = False
        keep = torch.from_numpy(keep).to(DEV)
        for a, b in zip(got, want):
            assert torch.equal(a[keep], b[keep])
        assert not bool(torch.isfinite(got[0][~keep, 0:2]).any()) and not bool(torch.isfinite(got[4][~keep]).any())


def test_slip_is_optional(eng):
    want = run(eng, 257, "mixed", "plane")
    got = run(eng, 257, "mixed", "plane", slip=False)
    assert got[4] is None and all(torch.equal(a, b) for a, b in zip(got[:4], want[:4]))
    assert float(want[4].min()) >= 0 and float(want[4].max()) > 0.01


def test_level_ground_ideal_actuators_forward_commands_match_the_command_mode(eng):
    """On a constant heightfield, with ideal actuators and forward commands off the turn-on-the-spot rule, the wheels realise the
    commanded twist: the drive mode's pose agrees with rover_motion_step's within the two restatements' own difference (float64, on the
    same inputs) plus each kernel's tolerance against its restatement, measured as everywhere in this file."""
    from isaac_rover_amd import _lib
    n = 257
    rng = np.random.default_rng(4)
    ang = rng.uniform(-1, 1, n).astype(np.float32)
    lin = (np.abs(ang) * rng.uniform(0.5, 1.0, n) + 0.01).astype(np.float32)               # forward, |v / w| >= 0.5
    steer, vel, br = A.ackermann(lin, ang)
    assert not br["far"].any() and br["keep"].all()
    pos, quat = INPUTS[0][:n], INPUTS[1][:n]
    pt, vt = np.zeros((n, 13), dtype=np.float32), np.zeros((n, 13), dtype=np.float32)
    for i in range(6):
        if D.STEER_COLS[i] is not None:
            pt[:, D.STEER_COLS[i]] = steer[:, i]
        vt[:, D.DRIVE_COLS[i]] = vel[:, i]
    field = R.Field(np.full((N0, N1), 0.37, dtype=np.float32), HSCALE, 1.0, SHIFT)
    zero = np.zeros((n, 13), dtype=np.float32)
    ref = {}
    for dtype in (np.float64, np.float32):
        cmd = R.step(field, pos, quat, lin, ang, dt=DT, substeps=2, ride_height=RIDE, dtype=dtype)
        drv = D.step(field, pos, quat, (pt, vt, zero, zero), dt=DT, substeps=2, ride_height=RIDE, dtype=dtype)
        ref[dtype] = (cmd, drv)
    flat = _lib.Engine(8, device=0)
    try:
        flat.set_heightfield(field.hm, HSCALE, 1.0, SHIFT)
        tp, tq, tl, ta = (torch.from_numpy(a).to(DEV) for a in (pos.copy(), quat.copy(), lin, ang))
        flat.motion_step(tp, tq, tl, ta, dt=DT, substeps=2, ride_height=RIDE)
        dp, dq = torch.from_numpy(pos.copy()).to(DEV), torch.from_numpy(quat.copy()).to(DEV)
        sl = torch.zeros(n, device=DEV)
        joints = tuple(torch.from_numpy(a.copy()).to(DEV) for a in (pt, vt, zero, zero))
        flat.motion_step(dp, dq, None, None, dt=DT, substeps=2, ride_height=RIDE, joints=joints, drive="wheels", slip=sl)
        torch.cuda.synchronize()
    finally:
        flat.close()
    for name, got_c, got_d, k in (("pos", tp, dp, "pos"), ("quat", tq, dq, "quat")):
        c64, d64 = ref[np.float64][0][k], ref[np.float64][1][k]
        own = np.abs(c64 - d64).max()
        tol_c = max(8.0 * np.abs(ref[np.float32][0][k] - c64).max(), 4.0 * EPS32 * np.abs(c64).max())
        tol_d = max(8.0 * np.abs(ref[np.float32][1][k] - d64).max(), 4.0 * EPS32 * np.abs(d64).max())
        diff = float((got_c - got_d).abs().max())
        print(f"{name}: kernels differ by {diff:.3e}; the restatements by {own:.3e}; tolerances {tol_c:.3e} + {tol_d:.3e}")
        assert diff <= own + tol_c + tol_d
    assert float((dp - torch.from_numpy(pos).to(DEV)).abs().max()) > 0.05 and float(sl.max()) <= 1e-5


def test_refusals_on_a_live_ctx(eng):
    from isaac_rover_amd import _lib
    from isaac_rover_amd._lib import RoverError
    n = 8
    pos, quat, pt, vt, jp, jv = dev_inputs(n)
    keep = [t.clone() for t in (pos, quat, jp, jv)]
    joints = dict(joint_pos_targets13=pt.data_ptr(), joint_vel_targets13=vt.data_ptr(), joint_pos13=jp.data_ptr(), joint_vel13=jv.data_ptr())

    def call(ctx, e=n, params=None, **kw):
        d = _lib.motion_desc(e, **dict(dict(joints, pos3=pos.data_ptr(), quat4=quat.data_ptr(), lin=None, ang=None, cmd_stride=0), **kw))
        p = _lib.DriveParams(0.2, math.inf, math.inf, None) if params is None else params
        rc = ctx.lib.rover_motion_step_drive(ctx._h, C.byref(d), C.byref(p), None, None)
        return rc, ctx.lib.rover_last_error(ctx._h).decode()

    for kw in (dict(e=-1), dict(substeps=0), dict(dt=0.0), dict(pos3=None), dict(joint_pos13=None), dict(params=_lib.DriveParams(0.0, 1.0, 1.0, None)),
               dict(params=_lib.DriveParams(0.2, float("nan"), 1.0, None)), dict(params=_lib.DriveParams(0.2, 1.0, -1.0, None))):
        rc, msg = call(eng, **kw)
        assert rc == -1 and msg.startswith("motion_step_drive:"), (kw, rc, msg)
    bare = _lib.Engine(8, device=0)                                # no heightfield: ROVER_E_STATE, also with E = 0
    try:
        for e in (n, 0):
            rc, msg = call(bare, e=e)
            assert rc == -2 and "rover_set_heightfield" in msg, (rc, msg)
    finally:
        bare.close()
    assert call(eng, e=0)[0] == 0 and call(eng, e=0, pos3=None, quat4=None, **{k: None for k in joints})[0] == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (pos, quat, jp, jv)))                  # none of them launched
    for kw in (dict(joints=None), dict(drive="tracks"), dict(slip=torch.zeros(n - 1, device=DEV)), dict(slip=torch.zeros(n, device=DEV).double()),
               dict(wheel_radius=0.0), dict(steer_rate=0.0), dict(joints=(pt, vt, jp))):
        args = dict(dt=DT, joints=(pt, vt, jp, jv), drive="wheels")
        args.update(kw)
        with pytest.raises(RoverError):
            eng.motion_step(pos, quat, None, None, **args)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (pos, quat, jp, jv)))


def test_a_task_on_its_wheels():
    """VecEnv(sim="terrain", drive="wheels") on a task at 64 envs for 30 steps with slow actuators, eight envs timing out on the way:
    finite poses and observations; an env reset by the step's pre_physics_step starts from a zero joint state, so what the step leaves
    in its steering and drive columns is the rate limiter's fold from 0 towards its targets, bit for bit; slip shows while the steering
    lags.  drive="command" on the same task state gives the bits of rover_motion_step called through the C ABI directly."""
    from isaac_rover_amd import _lib, synth
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.tasks.rover import RoverTask
    from isaac_rover_amd.vec_env import TerrainSim, VecEnv
    e, steer_rate, accel = 64, 0.8, 6.0
    scene = synth.make_scene(n_cells=128, k=16, n_stones=10)
    env = VecEnv(headless=True, sim="terrain", drive="wheels", steer_rate=steer_rate, wheel_accel=accel)
    task = RoverTask("Rover", SimConfig(num_envs=e, device=DEV), env, scene=scene, distribution=synth.ray_distribution("37"))
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(e, 3)
    spawn[:, 0:2] = 0.15 * 12.8 + 0.7 * 12.8 * torch.rand(e, 2, generator=g)
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    world = env._world
    assert isinstance(world, TerrainSim) and (world.drive, world.steer_rate, world.wheel_accel) == ("wheels", steer_rate, accel)
    env.reset()
    task.progress_buf[:8] = task.max_episode_length - 6                       # these time out within the run
    actions = torch.tensor([[0.8, 0.25]], device=DEV).repeat(e, 1)
    actions[e // 2:] = torch.tensor([-0.6, 0.5], device=DEV)                    # half of them in reverse
    n_sub = task.control_frequency_inv
    step_s, step_w = np.float32(steer_rate) * np.float32(0.05), np.float32(accel) * np.float32(0.05)
    prev_done, seen_resets, slipped = torch.zeros(e, dtype=torch.bool, device=DEV), 0, 0.0
    for _ in range(30):
        obs, rew, done, info = env.step(actions)
        assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
        pos, quat = task._rover.get_world_poses()
        assert bool(torch.isfinite(pos).all()) and float((quat.norm(dim=1) - 1).abs().max()) <= 1e-5
        slipped = max(slipped, float(world.last_slip.max()))
        ids = torch.nonzero(prev_done).flatten().cpu().numpy()
        if len(ids):                                # reset at the start of this step: from rest, n_sub sub-steps towards the targets
            seen_resets += len(ids)
            jp, jv = task._rover.get_joint_positions().cpu().numpy(), task._rover.get_joint_velocities().cpu().numpy()
            pt, vt = task._rover._joint_pos_targets.cpu().numpy(), task._rover._joint_vel_targets.cpu().numpy()
            for cols, state, target, step in ((ACTUATED_POS, jp, pt, step_s), (ACTUATED_VEL, jv, vt, step_w)):
                want = np.zeros((len(ids), len(cols)), dtype=np.float32)
                for _ in range(n_sub):
                    want = D.rate_limit(want, target[ids][:, cols], step)
                assert want.dtype == np.float32 and np.array_equal(state[ids][:, cols], want)
                assert np.abs(state[ids][:, cols]).max() <= n_sub * float(step) * (1 + 1e-6)
        prev_done = done.bool().clone()
    assert seen_resets >= 8 and slipped > 1e-3
    # drive="command" is the parent's call: Engine.motion_step without the new arguments against rover_motion_step itself
    r = task._rover
    lin, ang = task.linear_velocity.get_state(0), task.angular_velocity.get_state(0)
    pos, quat = (t.clone() for t in r.get_world_poses())
    joints = (r._joint_pos_targets, r._joint_vel_targets, r.get_joint_positions().clone(), r.get_joint_velocities().clone())
    task._engine.motion_step(pos, quat, lin, ang, dt=0.05, substeps=n_sub, joints=joints, drive="command", wheel_radius=0.1, steer_rate=1.0)
    pos2, quat2 = (t.clone() for t in r.get_world_poses())
    jp2, jv2 = torch.zeros_like(joints[2]), torch.zeros_like(joints[3])
    desc = _lib.motion_desc(e, pos2.data_ptr(), quat2.data_ptr(), lin.data_ptr(), ang.data_ptr(), lin.stride(0), n_sub, 0.05, 1.0, 1.0, 0.3,
                            joints[0].data_ptr(), joints[1].data_ptr(), jp2.data_ptr(), jv2.data_ptr())
    assert task._engine.lib.rover_motion_step(task._engine._h, C.byref(desc), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(pos, pos2) and torch.equal(quat, quat2) and torch.equal(joints[2], jp2) and torch.equal(joints[3], jv2)
    assert torch.equal(jp2, joints[0]) and not torch.equal(pos, r.get_world_poses()[0])
    env.close()
