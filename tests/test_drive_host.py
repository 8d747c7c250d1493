"""CPU: the wheel-level drive mode of the motion model as DEFINED (tests/drive_ref.py; include/rover_step.h, rover_motion_step_drive;
DESIGN.md §4.24) — the constant of the twist fit against the library's host entry, every refusal that needs no device, the closed loop
Ackermann -> wheels -> body twist, the rate limiter's exact landing, the wrong variants the restatement tells apart, and the ``drive``
switch.  No GPU."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import drive_ref as D
import metrics_ref as A
import motion_ref as R

EPS32 = float(np.finfo(np.float32).eps)
DT = 0.05


def test_symbols_declared_and_exported():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for name in ("rover_motion_step_drive", "rover_motion_drive_fit"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert [f for f, _ in _lib.DriveParams._fields_] == ["wheel_radius", "steer_rate", "wheel_accel", "slip"] and C.sizeof(_lib.DriveParams) == 24
    assert _lib.DRIVES == ("command", "wheels")


def test_the_fit_is_the_pseudo_inverse_of_the_rigid_motion_matrix():
    """rover_motion_drive_fit against numpy.linalg.pinv of M (rows (1, 0, -b_i), (0, 1, a_i)), rounded to float32: bit for bit, held the
    way test_motion_host holds rover_motion_plane_fit — in the 30 entries whose exact value is not 0.  sum b_i = 0 makes vx the mean of
    the x components, so the six entries pairing vx with a y component are exactly 0; an SVD may leave noise of 1e-17 there whose bits
    no library can be held to, so, as test_bogie_host does, all 36 entries are held to something stronger: each is the float32 nearest
    to the exact rational (M^T M)^-1 M^T, and the zeros are +0.  P M = I to 1e-6: |M| <= 1 and |P| < 0.27, so float32 rounding of P
    moves an entry of P M by at most 12 * 0.27 * 2^-24 = 2e-7."""
    from isaac_rover_amd import _lib
    m = D.rigid_matrix()
    assert m.shape == (12, 3)
    assert np.array_equal(m[0::2], [[1.0, 0.0, r] for r, _ in R.WHEELS]) and np.array_equal(m[1::2], [[0.0, 1.0, f] for _, f in R.WHEELS])
    got = _lib.motion_drive_fit()
    assert got.dtype == np.float32 and got.shape == (3, 12)
    fm = [[Fraction(float(v)) for v in row] for row in m]
    g = [[sum(fm[j][r] * fm[j][c] for j in range(12)) for c in range(3)] for r in range(3)]
    det = sum(g[0][c] * (g[1][(c + 1) % 3] * g[2][(c + 2) % 3] - g[1][(c + 2) % 3] * g[2][(c + 1) % 3]) for c in range(3))
    inv = [[(g[(c + 1) % 3][(r + 1) % 3] * g[(c + 2) % 3][(r + 2) % 3] - g[(c + 1) % 3][(r + 2) % 3] * g[(c + 2) % 3][(r + 1) % 3]) / det
            for c in range(3)] for r in range(3)]
    exact = [[sum(inv[r][c] * fm[j][c] for c in range(3)) for j in range(12)] for r in range(3)]
    assert all(sum(exact[r][j] * fm[j][c] for j in range(12)) == (r == c) for r in range(3) for c in range(3))      # it IS a left inverse
    zeros = [(r, j) for r in range(3) for j in range(12) if exact[r][j] == 0]
    assert zeros == [(0, j) for j in range(1, 12, 2)]
    want = np.linalg.pinv(m)
    for r in range(3):
        for j in range(12):
            v = got[r, j]
            if (r, j) in zeros:
                assert v.view(np.uint32) == 0 and abs(want[r, j]) < 1e-15, (r, j)
                continue
            assert v.view(np.uint32) == want[r, j].astype(np.float32).view(np.uint32), (r, j, v, want[r, j])
            err = abs(Fraction(float(v)) - exact[r][j])
            for other in (np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))):
                assert err <= abs(Fraction(float(other)) - exact[r][j]), (r, j)
    assert np.array_equal(got, D.drive_fit())
    assert np.abs(got.astype(np.float64) @ m - np.eye(3)).max() <= 1e-6
    assert 1.86 < np.linalg.cond(m) < 1.88
    lib = _lib.load()
    assert lib.rover_motion_drive_fit(None) == -1 and b"motion_drive_fit" in lib.rover_last_error(None)


def test_descriptor_and_parameter_refusals_need_no_device():
    """Every ROVER_E_INVALID of rover_motion_step_drive is decided before the ctx is looked at: the refusals of the other two modes that
    still apply (lin, ang and cmd_stride are not read here: NULL and 0 pass), a missing joint quadruple, NULL or bad drive parameters,
    bad bogie parameters — each reported by name with a NULL ctx."""
    from isaac_rover_amd import _lib
    lib = _lib.load()
    names = ("joint_pos_targets13", "joint_vel_targets13", "joint_pos13", "joint_vel13")
    joints = {n: 16 for n in names}
    inf, nan = math.inf, math.nan

    def desc(e=4, **kw):
        return _lib.motion_desc(e, **dict(dict(joints, lin=None, ang=None, cmd_stride=0, max_lin=0.0, max_ang=0.0), **kw))

    def params(radius=0.2, steer=inf, accel=inf, slip=None):
        return _lib.DriveParams(radius, steer, accel, slip)

    def call(d, p, b=None):
        rc = lib.rover_motion_step_drive(None, None if d is None else C.byref(d), None if p is None else C.byref(p), None if b is None else C.byref(b), None)
        return rc, lib.rover_last_error(None).decode()

    ok, bogie = params(), _lib.BogieParams
    bad = [("null descriptor", None, ok, None, "null descriptor"), ("E < 0", desc(-1), ok, None, "negative"), ("substeps 0", desc(substeps=0), ok, None, "substeps"),
           ("substeps -2", desc(substeps=-2), ok, None, "substeps"), ("dt 0", desc(dt=0.0), ok, None, "dt"), ("dt < 0", desc(dt=-0.05), ok, None, "dt"),
           ("dt nan", desc(dt=nan), ok, None, "dt"), ("dt inf", desc(dt=inf), ok, None, "dt"), ("no pos", desc(pos3=None), ok, None, "pos3"),
           ("no quat", desc(quat4=None), ok, None, "quat4")]
    for mask in range(1, 15):
        bad.append((f"joints {mask:04b}", desc(**{n: (16 if mask >> i & 1 else None) for i, n in enumerate(names)}), ok, None, "go together"))
    bad += [("no joints", desc(**{n: None for n in names}), ok, None, "must be given"), ("null params", desc(), None, None, "null parameters"),
            ("radius 0", desc(), params(radius=0.0), None, "wheel_radius"), ("radius < 0", desc(), params(radius=-0.1), None, "wheel_radius"),
            ("radius nan", desc(), params(radius=nan), None, "wheel_radius"), ("radius inf", desc(), params(radius=inf), None, "wheel_radius"),
            ("steer 0", desc(), params(steer=0.0), None, "steer_rate"), ("steer < 0", desc(), params(steer=-1.0), None, "steer_rate"),
            ("steer nan", desc(), params(steer=nan), None, "steer_rate"), ("steer -inf", desc(), params(steer=-inf), None, "steer_rate"),
            ("accel 0", desc(), params(accel=0.0), None, "wheel_accel"), ("accel < 0", desc(), params(accel=-1.0), None, "wheel_accel"),
            ("accel nan", desc(), params(accel=nan), None, "wheel_accel"),
            ("iters 0", desc(), ok, bogie(0, 0.6), "iters"), ("iters 9", desc(), ok, bogie(9, 0.6), "iters"), ("max_bogie 0", desc(), ok, bogie(4, 0.0), "max_bogie"),
            ("max_bogie nan", desc(), ok, bogie(4, nan), "max_bogie"), ("max_bogie inf", desc(), ok, bogie(4, inf), "max_bogie"),
            ("E 0, radius 0", desc(0), params(radius=0.0), None, "wheel_radius"), ("E 0, null params", desc(0), None, None, "null parameters")]
    for what, d, p, b, word in bad:
        rc, msg = call(d, p, b)
        assert rc == -1 and msg.startswith("motion_step_drive:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    good = [(desc(), ok, None), (desc(0), ok, None), (desc(0, **{n: None for n in names}), ok, None), (desc(), params(0.1, 1e-3, 1e9, 64), None),
            (desc(), ok, bogie(1, 1e-3)), (desc(), ok, bogie(8, 3.0)), (desc(lin=16, ang=16, cmd_stride=3, max_lin=1.0), ok, None)]
    for d, p, b in good:
        assert call(d, p, b) == (-1, "motion_step_drive: null ctx")


# ---- closing the loop: Ackermann's targets through the drive model give back the command ----------------------------------------------

def commands(n=4000, seed=11):
    rng = np.random.default_rng(seed)
    lin, ang = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    lin[:8] = (0.0, 0.5, -0.5, 0.0, 0.0, 0.7, -0.7, 1.0)
    ang[:8] = (0.0, 0.0, 0.0, 0.6, -0.6, 1e-4, -2e-4, 1.0)           # both 0, ang = 0, lin = 0, and two rows on the go-straight branch
    return lin, ang


def targets_of(lin, ang):
    """metrics_ref's Ackermann in the reference's float32 -> (joint_pos_targets, joint_vel_targets) [n, 13] as pre_physics_step writes
    them, the branch record, and the speed Ackermann kept (lin zeroed on the spot)."""
    steer, vel, br = A.ackermann(lin, ang)
    pt, vt = np.zeros((len(lin), 13), dtype=np.float32), np.zeros((len(lin), 13), dtype=np.float32)
    for i in range(6):
        if D.STEER_COLS[i] is not None:
            pt[:, D.STEER_COLS[i]] = steer[:, i]
        vt[:, D.DRIVE_COLS[i]] = vel[:, i]
    v_eff = np.where(br["px"] != 0, lin, np.float32(0))
    return pt, vt, br, v_eff


def run_twist(pt, vt, dtype, **kw):
    n = len(pt)
    pos, quat = np.zeros((n, 3), dtype=np.float32), np.tile(np.float32([1, 0, 0, 0]), (n, 1))
    zero = np.zeros((n, 13), dtype=np.float32)
    return D.step(None, pos, quat, (pt, vt, zero, zero), dt=DT, dtype=dtype, **kw)


def test_ackermanns_targets_give_back_the_command():
    """4 000 seeded commands in [-1, 1]^2 (with lin = 0, ang = 0 and both) -> Ackermann (float32, as the reference computes it) -> the
    float64 restatement with +inf rates and wheel_radius = 0.2, from rest.  The fitted twist is (v_eff, 0, w) for v >= 0 and on the spot,
    and (v, 0, -w) in reverse: Ackermann puts the turning point at copysign(|v / w|, -w) whatever the sign of v, the car-like
    convention, so a reversing rover yaws against the commanded w.  Slip is 0.
    Tolerance, per quantity: 8 x the largest |float32 restatement - float64 restatement| on these inputs, never below 4 float32 ulp
    of the quantity's largest magnitude — the margin of the motion tests; nothing here comes from a kernel.
    Rows on Ackermann's go-straight branch (a wheel farther than 1000 m from the turning point: its speed is set to lin while its tiny
    steering angle stays) are held to vx = v — within the tolerance plus |v| d^2 / 2 = 1.1e-7 |v| for the cosine of an angle
    d <= 0.46 / 999 — and to w within 2.5e-3 |v|, which follows from |w| < |v| / 999 on that branch; their slip, the wheels' disagreement
    by that angle, within 2.5e-3 |v| likewise."""
    lin, ang = commands()
    pt, vt, br, v_eff = targets_of(lin, ang)
    r64, r32 = run_twist(pt, vt, np.float64), run_twist(pt, vt, np.float32)
    straight = br["far"].any(1)
    spot = (v_eff == 0)
    assert len(lin) >= 2000 and straight.sum() >= 2 and spot.sum() > 100 and (lin < 0).sum() > 1000
    v, w = v_eff.astype(np.float64), ang.astype(np.float64)
    want = np.stack((v, np.zeros_like(v), np.where(v < 0, -w, w)), 1)
    tol = {}
    for k, name in enumerate(("vx", "vy", "w")):
        d = np.abs(r32["twist"][:, k].astype(np.float64) - r64["twist"][:, k]).max()
        tol[name] = max(8.0 * d, 4.0 * EPS32 * np.abs(want[:, k]).max())
    d_slip = np.abs(r32["slip"].astype(np.float64) - r64["slip"]).max()
    speed = np.abs(vt).max() * D.WHEEL_RADIUS
    tol["slip"] = max(8.0 * d_slip, 4.0 * EPS32 * speed)
    err = np.abs(r64["twist"] - want)
    print("tolerances:", tol, "worst twist error off the go-straight branch:", err[~straight].max(0), "with every row counted:", err.max(),
          "worst slip:", r64["slip"][~straight].max(), "rows on the go-straight branch:", int(straight.sum()))
    for k, name in enumerate(("vx", "vy", "w")):
        assert err[~straight, k].max() <= tol[name], (name, err[~straight, k].max(), tol[name])
    assert r64["slip"][~straight].max() <= tol["slip"], (r64["slip"][~straight].max(), tol["slip"])
    av = np.abs(lin[straight].astype(np.float64))
    assert np.all(err[straight, 0] <= tol["vx"] + 1.1e-7 * av)
    assert np.all(err[straight, 2] <= 2.5e-3 * av) and np.all(r64["slip"][straight] <= 2.5e-3 * av + tol["slip"])
    # the yaw the model integrates is the fitted w: in reverse, the opposite of the command
    rev = (v < 0) & ~straight
    assert np.abs(r64["yaw"][rev] + w[rev] * np.float64(np.float32(DT))).max() <= 1e-6 and np.abs(w[rev]).max() > 0.9
    # wheel_radius = 0.1, the asset's physical radius, halves every speed
    half = run_twist(pt, vt, np.float64, wheel_radius=0.1)
    assert np.abs(half["twist"] - 0.5 * r64["twist"]).max() <= 1e-7


def test_the_restatement_tells_wrong_variants_apart():
    lin, ang = commands()
    pt, vt, br, v_eff = targets_of(lin, ang)
    straight = br["far"].any(1)
    right64, right32 = run_twist(pt, vt, np.float64), run_twist(pt, vt, np.float32)
    gap = np.abs(right32["pos"].astype(np.float64) - right64["pos"]).max()
    gap_yaw = np.abs(right32["yaw"].astype(np.float64) - right64["yaw"]).max()
    # yaw from the commanded w: wrong in reverse by 2 w dt
    wrong = run_twist(pt, vt, np.float64, wrong="yaw_from_command", w_cmd=ang)
    rev = (v_eff < 0) & ~straight
    assert np.abs(wrong["yaw"] - right64["yaw"])[rev].max() > 1000 * max(gap_yaw, EPS32) and np.abs(wrong["yaw"] - right64["yaw"])[~rev & ~straight].max() <= 8 * gap_yaw + 4 * EPS32
    # RL read as -j7: the rear-left wheel fights the turn
    wrong = run_twist(pt, vt, np.float64, wrong="rl_sign")
    turning = (np.abs(pt[:, 7]) > 0.1) & (v_eff != 0)
    assert turning.sum() > 500 and np.abs(wrong["twist"] - right64["twist"])[turning].max(1).min() > 1e-3
    assert wrong["slip"][turning].min() > 1e-3 and np.abs(wrong["pos"] - right64["pos"]).max() > 1000 * gap
    # P summed from the last column downwards: float32 sees it (float64 agrees to rounding)
    wrong32 = run_twist(pt, vt, np.float32, wrong="sum_order")
    assert not np.array_equal(wrong32["twist"], right32["twist"])
    assert np.abs(run_twist(pt, vt, np.float64, wrong="sum_order")["twist"] - right64["twist"]).max() <= 1e-14
    # rule 1 as a clipped step: state + (target - state) is not the target in float32 where the difference is inexact, that is
    # when a state jumps across 0 or by more than its own size — one sub-step that is longer than the whole way
    n = len(pt)
    rng = np.random.default_rng(2)
    jp = np.zeros((n, 13), dtype=np.float32)
    jp[:, D.STEERED] = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
    pos, quat = np.zeros((n, 3), dtype=np.float32), np.tile(np.float32([1, 0, 0, 0]), (n, 1))
    kw = dict(dt=DT, substeps=1, steer_rate=80.0, dtype=np.float32)             # 4 rad per sub-step: it lands
    right = D.step(None, pos, quat, (pt, vt, jp, np.zeros_like(jp)), **kw)
    wrong = D.step(None, pos, quat, (pt, vt, jp, np.zeros_like(jp)), wrong="no_landing", **kw)
    assert np.array_equal(right["joint_pos"][:, D.STEERED], pt[:, D.STEERED])
    off = (wrong["joint_pos"][:, D.STEERED] != pt[:, D.STEERED]).any(1)
    assert off.sum() > n // 20, off.sum()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_state_reaches_its_target_in_ceil_steps_and_stays(dtype):
    """With finite rates a state takes ceil(|target - state| / step) sub-steps to reach its target, moves by exactly one step until
    then without ever passing it, equals it bit for bit from then on, and a call with `substeps` = n is n calls."""
    rng = np.random.default_rng(9)
    n, steer_rate, accel = 300, 0.9, 35.0
    k = np.dtype(dtype).type
    pt, vt, jp, jv = (np.zeros((n, 13), dtype=np.float32) for _ in range(4))
    pt[:, D.STEERED], jp[:, D.STEERED] = rng.uniform(-1.5, 1.5, (n, 4)), rng.uniform(-1.5, 1.5, (n, 4))
    vt[:, D.DRIVE_COLS], jv[:, D.DRIVE_COLS] = rng.uniform(-9, 9, (n, 6)), rng.uniform(-9, 9, (n, 6))
    jp[:5, D.STEERED], jv[:5, D.DRIVE_COLS] = pt[:5, D.STEERED], vt[:5, D.DRIVE_COLS]            # already there: 0 steps
    pt[:, 0:3], vt[:, 0:3] = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))              # passive columns: copied
    step_s, step_w = k(np.float32(steer_rate)) * k(np.float32(DT)), k(np.float32(accel)) * k(np.float32(DT))
    cols = [("joint_pos", c, pt, jp, step_s) for c in D.STEERED] + [("joint_vel", c, vt, jv, step_w) for c in D.DRIVE_COLS]
    ratio = np.stack([np.abs(t[:, c].astype(np.float64) - s[:, c]) / float(st) for _, c, t, s, st in cols], 1)
    assert np.abs(ratio - np.rint(ratio))[ratio > 0].min() > 1e-4            # no ratio sits on an integer: ceil is safe from rounding
    need = np.ceil(ratio).astype(int)
    total = int(need.max()) + 2
    assert 20 < total < 120
    pos, quat = np.zeros((n, 3), dtype=np.float32), np.tile(np.float32([1, 0, 0, 0]), (n, 1))
    kw = dict(dt=DT, steer_rate=steer_rate, wheel_accel=accel, dtype=dtype)
    fold = lambda it: D.step(None, pos, quat, (pt, vt, jp, jv), substeps=it, **kw)
    prev = dict(joint_pos=jp.astype(dtype), joint_vel=jv.astype(dtype))
    chain = dict(prev, pos=pos, quat=quat)                  # float32 only: `it` calls of one sub-step each
    for it in range(1, total + 1):
        out = fold(it)
        for j, (key, c, t, s, st) in enumerate(cols):
            now, before, tgt = out[key][:, c], prev[key][:, c], t[:, c].astype(dtype)
            landed = need[:, j] <= it
            assert np.array_equal(now[landed], tgt[landed])
            moving = ~landed
            assert np.all(np.abs(tgt[moving] - now[moving]) < np.abs(tgt[moving] - before[moving]))
            assert np.all(np.sign(tgt[moving] - now[moving]) == np.sign(tgt[moving] - before[moving]))              # never past the target
            assert np.array_equal(now[moving], before[moving] + np.copysign(st, tgt[moving] - before[moving]))
        assert np.array_equal(out["joint_pos"][:, 0:3], pt[:, 0:3].astype(dtype)) and np.array_equal(out["joint_vel"][:, 0:3], vt[:, 0:3].astype(dtype))
        prev = out
        if dtype is np.float32:                             # the float32 state survives the hand-over between calls exactly
            chain = D.step(None, chain["pos"], chain["quat"], (pt, vt, chain["joint_pos"], chain["joint_vel"]), **kw)
            for key in ("pos", "quat", "joint_pos", "joint_vel", "slip"):
                assert np.array_equal(chain[key], out[key]), (it, key)
    # Ackermann's targets from rest, ideal wheel drives: while the steering lags the wheels disagree and the slip is positive; once it has
    # landed they agree with one rigid motion again
    lin, ang = commands(n)
    apt, avt, br, v_eff = targets_of(lin, ang)
    lag = (np.abs(apt[:, D.STEERED]).max(1) > 0.2) & (np.abs(avt).max(1) > 0.5)
    zero = np.zeros_like(apt)
    first = D.step(None, pos, quat, (apt, avt, zero, zero), dt=DT, steer_rate=steer_rate, dtype=dtype)
    assert lag.sum() > 60 and first["slip"][lag].min() > 1e-3
    last = D.step(None, pos, quat, (apt, avt, zero, zero), dt=DT, substeps=40, steer_rate=steer_rate, dtype=dtype)
    assert np.array_equal(last["joint_pos"], apt.astype(dtype)) and last["slip"][~br["far"].any(1)].max() <= 1e-5


def test_the_drive_switch():
    from isaac_rover_amd import _lib, vec_env

    class Task:
        num_envs, observation_space, action_space = 3, None, None

        def set_up_scene(self, spawn_positions=None):
            pass

        def post_reset(self):
            pass

    assert vec_env.DRIVES == ("command", "wheels") == _lib.DRIVES
    with pytest.raises(ValueError, match="needs sim='terrain'"):
        vec_env.VecEnv(sim="kinematic", drive="wheels")
    with pytest.raises(ValueError, match="needs sim='terrain'"):
        vec_env.VecEnv(drive="wheels")
    with pytest.raises(TypeError):
        vec_env.KinematicSim(Task(), drive="wheels")
    for bad in ("wheel", "", None, "Wheels"):
        with pytest.raises(ValueError, match="drive must be one of"):
            vec_env.VecEnv(sim="terrain", drive=bad)
        with pytest.raises(ValueError, match="drive must be one of"):
            vec_env.TerrainSim(Task(), drive=bad)
    for kw, cls, want in (({}, vec_env.KinematicSim, None), ({"sim": "kinematic", "drive": "command"}, vec_env.KinematicSim, None),
                          ({"sim": "terrain"}, vec_env.TerrainSim, ("command", "plane")), ({"sim": "terrain", "drive": "command"}, vec_env.TerrainSim, ("command", "plane")),
                          ({"sim": "terrain", "drive": "wheels"}, vec_env.TerrainSim, ("wheels", "plane")),
                          ({"sim": "terrain", "drive": "wheels", "suspension": "bogie"}, vec_env.TerrainSim, ("wheels", "bogie"))):
        env = vec_env.VecEnv(headless=True, **kw)
        env.set_task(Task(), sim_params={"dt": 0.02})
        assert type(env._world) is cls and env._world.dt == 0.02
        assert (want is None) or (env._world.drive, env._world.suspension) == want
    env = vec_env.VecEnv(sim="terrain", drive="wheels", wheel_radius=0.1, steer_rate=1.5, wheel_accel=20.0)
    env.set_task(Task())
    w = env._world
    assert (w.drive, w.wheel_radius, w.steer_rate, w.wheel_accel) == ("wheels", 0.1, 1.5, 20.0)
    w = vec_env.TerrainSim(Task())
    assert (w.drive, w.wheel_radius, w.steer_rate, w.wheel_accel) == ("command", 0.2, math.inf, math.inf)
