"""The per-environment step decisions restated in plain numpy float32, one rounding per operation, in the reference's order:
check_collision (rover.py:663-672), calculate_metrics (rover.py:460-531), is_done (rover.py:610-647), and Ackermann
(tasks/utils/kinematics.py:13-67).  Written from the reference's Python and SURVEY.md, not from the kernels: it is the yardstick for
metrics_done_kernel / obs_metrics_kernel / ackermann_kernel / pre_physics_kernel, whose every operation is one IEEE float32 operation.
tests/test_metrics_host.py pins it to the reference's own outputs (every step_*_fp32 golden) and, bit for bit, to the CPU oracle.

The restatement takes what the decision code itself reads — the step's state AND the heading difference and the 26 rock-ray distances
of the earlier stages — so a comparison feeds it the device's (or the reference's) own heading and distances: the pose trigonometry
and the ray cast have tests of their own and stay out of this one.

``threshold_table`` is the batch such a comparison runs: make_states rows overwritten with ulp ladders round every threshold of the
decision code, and ``coverage`` asserts, from the restatement's outputs, that each side of each threshold is populated."""
import dataclasses

import numpy as np

F = np.float32
I64 = np.int64

# the constants as the reference writes them: Python doubles, rounded to f32 where ATen meets an f32 tensor
C_089 = F(0.33 * 0.33)          # rover.py:505
C_103 = F(1.03)                 # :506
C_3000 = F(3000)                # :522
C_300 = F(300)                  # :519
TILT = F(0.78 * 1.5)            # :615-616
TD_GOAL, TD_AREA, TD_FAR = F(0.18), F(9.5), F(11)   # :506,619 / :622 / :618
HEADING_GATE, HEADING_GAIN, MOTION_GATE = F(2.0), F(0.3), F(0.05)     # :495 / :495 / :498-499
THREE = F(3)

EXTRAS = ("pos_reward", "collision_penalty", "uprightness_penalty", "heading_contraint_penalty", "motion_contraint_penalty",
          "goal_angle_penalty", "torque_penalty_driving", "torque_penalty_steering")
FLOAT_OUTPUTS = ("rew",) + tuple("extras_" + k for k in EXTRAS if k != "collision_penalty")
INT_OUTPUTS = ("rock_collision", "reset", "progress", "extras_collision_penalty", "eval_code", "eval_step")

DEFAULT_REWARDS = dict(pos_reward=1.0, heading_contraint_reward=0.05, motion_contraint_reward=-0.01, goal_angle_reward=0.3,
                       boogie_contraint_reward=0.5)                         # cfg/task/Rover.yaml
REWARDS_A = dict(pos_reward=1.7, heading_contraint_reward=0.11, motion_contraint_reward=-0.03, goal_angle_reward=0.45,
                 boogie_contraint_reward=0.7)                               # five distinct non-default scales: a swap shows

WRONG_VARIANTS = ("goal_lt", "tilt_gt", "motion_sum_first", "pos_scale_one", "timeout_before_increment")


@dataclasses.dataclass
class Config:
    level: int = 2
    max_episode_length: int = 3000
    num_envs_global: int = 0            # 0: the batch's own size (rover.py:517 `self.num_envs`)
    rewards: dict = None
    wheel_thr: float = 0.8              # rover.py:667
    body_thr: float = 0.45              # :668
    increment: bool = True              # rl_task.py:250 progress_buf += 1
    collision: bool = True              # the check_collision stage runs (part of get_observations)
    metrics: bool = True
    done: bool = True
    evaluation: bool = False            # rover.py:122: is_evaluation

    def scales(self):
        rw = dict(DEFAULT_REWARDS)
        rw.update(self.rewards or {})
        return {k: F(v) for k, v in rw.items()}


def _f(a):
    return np.ascontiguousarray(np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a), dtype=F)


def _i(a):
    return np.ascontiguousarray(np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a), dtype=I64)


def restate(st, heading_diff, wheel_dist, body_dist, cfg, rock_collision_in=None, eval_code_in=None, eval_step_in=None, wrong=None):
    """One post_physics_step's decisions.  ``st``: pos, target, joints, lin_hist, ang_hist, euler_pre, progress (the PRE-increment
    progress).  ``wrong``: one of WRONG_VARIANTS, a deliberately broken restatement (the host test shows the table tells them apart).
    Returns a dict: rew, extras_*, rock_collision, reset, progress, eval_code, eval_step, plus the deciding values the coverage check
    reads (td, min_wheel, min_body, dl, da, cause)."""
    assert wrong is None or wrong in WRONG_VARIANTS
    pos, target, joints = _f(st["pos"]), _f(st["target"]), _f(st["joints"])
    lin_hist, ang_hist, euler_pre = _f(st["lin_hist"]), _f(st["ang_hist"]), _f(st["euler_pre"])
    e = pos.shape[0]
    progress_in = _i(st["progress"])
    hd, wd, bd = _f(heading_diff), _f(wheel_dist), _f(body_dist)
    sc = cfg.scales()
    n_global = cfg.num_envs_global or e
    max_len = int(cfg.max_episode_length)
    code0 = np.zeros(e, I64) if eval_code_in is None else _i(eval_code_in)
    step0 = np.zeros(e, I64) if eval_step_in is None else _i(eval_step_in)
    code = code0.copy()
    out = {}

    progress = progress_in + 1 if cfg.increment else progress_in.copy()      # rl_task.py:250, before get_observations
    # ---- check_collision, rover.py:663-672: called at level >= 2 only (:292); below that the stage reports "no collision"
    mw, mb = wd.min(axis=1), bd.min(axis=1)
    if cfg.collision:
        coll = np.zeros(e, I64)
        if cfg.level >= 2:
            coll = np.where(np.abs(mw) < F(cfg.wheel_thr), 1, 0).astype(I64)
            coll = np.where(np.abs(mb) < F(cfg.body_thr), 1, coll)
            if cfg.evaluation:
                code = np.where(code == 0, coll, code)                          # :671
    else:
        coll = np.zeros(e, I64) if rock_collision_in is None else _i(rock_collision_in)
    out["rock_collision"] = coll.copy()

    dx, dy = target[:, 0] - pos[:, 0], target[:, 1] - pos[:, 1]
    td = np.sqrt(dx * dx + dy * dy)                                              # :482 / :617
    goal = (td < TD_GOAL) if wrong == "goal_lt" else (td <= TD_GOAL)
    hits = (coll == 1) if cfg.level >= 2 else np.zeros(e, bool)                 # :514 / :645: rock_collison is read at level >= 2 only

    lin, lin_prev, ang, ang_prev = lin_hist[:, 0], lin_hist[:, 1], ang_hist[:, 0], ang_hist[:, 1]
    dl = np.abs(lin * THREE - THREE * lin_prev)                                  # :498
    da = np.abs(ang * THREE - THREE * ang_prev)                                  # :499
    if cfg.metrics:
        zero = F(0)
        heading_pen = np.where(lin < 0, F(-1), zero) * sc["heading_contraint_reward"]                      # :486
        boogie = (np.abs(joints[:, 0]) + np.abs(joints[:, 1]) + np.abs(joints[:, 2])) * sc["boogie_contraint_reward"]   # :492
        goal_pen = np.where(np.abs(hd) > HEADING_GATE, -np.abs(hd * HEADING_GAIN * sc["goal_angle_reward"]), zero)       # :495
        p1 = np.where(dl > MOTION_GATE, dl * dl, zero)
        p2 = np.where(da > MOTION_GATE, da * da, zero)
        if wrong == "motion_sum_first":
            motion = (p1 * p1 + p2 * p2) * sc["motion_contraint_reward"]
        else:
            motion = (p1 * p1) * sc["motion_contraint_reward"]                                              # :500
            motion = motion + (p2 * p2) * sc["motion_contraint_reward"]                                     # :502
        pos_scale = F(1.0) if wrong == "pos_scale_one" else sc["pos_reward"]
        pos_rew = (F(1.0) / (F(1.0) + (C_089 * td) * td)) * pos_scale                                       # :505
        pos_rew = np.where(goal, C_103 * (max_len - progress).astype(F), pos_rew)                          # :506
        reward = pos_rew + heading_pen + motion + goal_pen                                                  # :512
        tracker = np.where(hits, n_global, 0).astype(I64)                                                   # :517
        reward = np.where(hits, reward - C_300, reward)                                                     # :519
        reward = reward / C_3000                                                                            # :522
        for k, v in (("rew", reward), ("extras_pos_reward", pos_rew), ("extras_uprightness_penalty", boogie),
                     ("extras_heading_contraint_penalty", heading_pen), ("extras_motion_contraint_penalty", motion),
                     ("extras_goal_angle_penalty", goal_pen), ("extras_torque_penalty_driving", lin),
                     ("extras_torque_penalty_steering", ang)):
            out[k] = np.ascontiguousarray(v, dtype=F)
            assert np.asarray(v).dtype == F, k                  # an accidental float64 promotion would hide a double rounding
        out["extras_collision_penalty"] = tracker

    timeout = (progress_in if wrong == "timeout_before_increment" else progress) >= max_len                # :614
    roll, pitch = np.abs(euler_pre[:, 0]), np.abs(euler_pre[:, 1])
    tilt_r = (roll > TILT) if wrong == "tilt_gt" else (roll >= TILT)                                       # :615
    tilt_p = (pitch > TILT) if wrong == "tilt_gt" else (pitch >= TILT)                                     # :616
    far = td >= TD_FAR                                                                                      # :618
    if cfg.done:
        reset = timeout | tilt_r | tilt_p | far | goal | hits                                               # :614-619,645-646
        out["reset"] = reset.astype(I64)
        if cfg.evaluation:                                                                                  # :620-632
            code = np.where((code == 0) & (td >= TD_AREA), 1, code)
            code = np.where((code == 0) & goal, 2, code)
            code = np.where((code == 0) & timeout, 3, code)
    out["progress"] = progress
    out["eval_code"] = code
    out["eval_step"] = np.where(code != code0, progress, step0)
    out.update(td=td, min_wheel=mw, min_body=mb, dl=dl, da=da, heading=hd,
               cause=(timeout * 1 + tilt_r * 2 + tilt_p * 4 + far * 8 + goal * 16 + hits * 32).astype(I64))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Ackermann, kinematics.py:13-67
# ---------------------------------------------------------------------------------------------------------------------------------
WHEELS = np.array([[-0.385, 0.438], [0.385, 0.438], [-0.447, 0.0], [0.447, 0.0], [-0.385, -0.411], [0.385, -0.411]], dtype=F)   # :20-25
SIDE = np.array([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0], dtype=F)                                                                      # :46
BOUND, FAR_DIST, DIAMETER = F(0.45), F(1000), F(0.2)
WRAP_LO, WRAP_HI, PI32 = F(-3.14 / 2), F(3.14 / 2), F(np.pi)


def ackermann(lin, ang, dtype=F, branches=None):
    """-> (steer [n, 6], vel [n, 6], branches).  dtype float32: the reference's arithmetic, one rounding per operation.  dtype float64 with
    ``branches`` of the float32 run: the same formulas in double on the float32 run's decisions (Px zeroed or not, dist > 1000, wrap
    taken or not) — the value a float32 library routine is measured against."""
    lin, ang = _f(lin).astype(dtype), _f(ang).astype(dtype)
    wl, side = WHEELS.astype(dtype), SIDE.astype(dtype)
    zero = dtype(0)
    with np.errstate(all="ignore"):
        px = np.copysign(lin / ang, -ang)                                        # :34-35
        keep = (np.abs(px) > dtype(BOUND)) if branches is None else branches["keep"]
        px = np.where(keep, px, zero)                                            # :38
        lin = np.where(px != 0, lin, zero)                                       # :39
        ddx, ddy = px[:, None] - wl[None, :, 0], zero - wl[None, :, 1]
        dist = np.sqrt(ddx * ddx + ddy * ddy)                                    # :43
        av = np.where((lin != 0)[:, None], np.copysign(ang, lin)[:, None], ang[:, None] * side[None, :])     # :49-52
        mv = dist * av                                                           # :55
        far = (dist > dtype(FAR_DIST)) if branches is None else branches["far"]
        mv = np.where(far, lin[:, None], mv)                                     # :58
        vel = mv / dtype(DIAMETER)                                               # :61
        sa = np.arctan2(np.broadcast_to(wl[None, :, 1], ddx.shape), wl[None, :, 0] - px[:, None])     # :63
        lo = (sa < dtype(WRAP_LO)) if branches is None else branches["lo"]
        sa = np.where(lo, sa + dtype(PI32), sa)                                  # :64
        hi = (sa > dtype(WRAP_HI)) if branches is None else branches["hi"]
        sa = np.where(hi, sa - dtype(PI32), sa)                                  # :65
    assert sa.dtype == dtype and vel.dtype == dtype
    return sa, vel, dict(keep=keep, far=far, lo=lo, hi=hi, px=px, dist=dist)


def ulp_steps(x, k):
    """float32 x moved by k units in the last place (k < 0: towards -inf)."""
    x = F(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def ladder(x, n=4):
    """x - n ulp ... x + n ulp, x itself in the middle."""
    return np.array([ulp_steps(x, k) for k in range(-n, n + 1)], dtype=F)


def ulp_diff(got, want64):
    """|got - want| in units of the float32 ulp of want (got float32, want float64)."""
    want64 = np.asarray(want64, np.float64)
    w32 = want64.astype(F)
    ulp = np.abs(np.nextafter(np.abs(w32), F(np.inf)) - np.abs(w32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / ulp


def steer_ulp(got, want64, unwrapped64):
    """|got - want| in float32 ulp of the UNWRAPPED angle: the wrap adds ±float32(pi) to an angle within a factor 2 of it, which is
    exact, so the error of a wrapped angle is atan2's, and near zero after the wrap it is no relative error of the result."""
    ulp = np.spacing(np.abs(np.asarray(unwrapped64)).astype(F)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64)) / ulp


def ackermann_table():
    """(lin, ang) float32: ±4 ulp ladders of lin / ang round ±0.45, zero rows, turning points on both sides of dist > 1000, and turning
    points that put each wheel's atan2 next to ±float32(3.14 / 2), plus 64 random pairs."""
    lin, ang = [], []

    def add(l, a):
        lin.append(F(l)), ang.append(F(a))

    for a in (F(1.0), F(-1.0), F(0.75), F(-3.0)):               # lin / ang: a = ±1 makes the quotient the ladder value itself
        for s in (1, -1):
            for v in ladder(BOUND):
                add(F(s) * v * a, a)
    for l in (0.5, -0.5):
        for a in (0.0, -0.0):
            add(l, a)                                            # lin / ±0 = ±inf: dist > 1000, straight
    for a in (0.7, -0.7):
        for l in (0.0, -0.0):
            add(l, a)                                            # turn on the spot
    add(0.0, 0.0), add(-0.0, 0.0), add(0.0, -0.0)                # 0 / 0 = NaN: |NaN| > 0.45 is false
    for r in (990.0, 999.0, 999.5, 1000.0, 1000.3, 1000.5, 1001.0, 1010.0):      # dist = hypot(Px - wx, wy) round 1000
        for s in (1, -1):
            add(s * r * 1e-3, 1e-3), add(s * r * 2e-3, -2e-3)
    # atan2(wy, wx - Px) reaches ±3.14 / 2 only at |wx - Px| < 4e-4, i.e. |Px| ~ 0.385 — a turning point :38 has already zeroed.  The
    # nearest a kept Px brings a wheel is atan2(0.438, ∓0.065) = 1.42 / 1.72 (the 0.45 ladders above); these rows put every wheel on
    # either side of both wrap thresholds at a distance
    for p in (0.46, 0.5, 0.7, 1.0, 3.0, 40.0):
        for s in (1, -1):
            add(-s * p, 1.0), add(s * p * 0.5, 0.5)              # Px = copysign(lin / ang, -ang)
    rng = np.random.default_rng(12)
    for l, a in zip(rng.uniform(-1, 1, 64), rng.uniform(-1, 1, 64)):
        add(l, a)
    return np.array(lin, F), np.array(ang, F)


# ---------------------------------------------------------------------------------------------------------------------------------
# the threshold table
# ---------------------------------------------------------------------------------------------------------------------------------
TABLE_ENVS = 384
_scene = {}


def table_scene():
    """The 128-cell, K = 24, 48-stone synthetic scene and the 9-ray distribution (built once per process)."""
    if not _scene:
        from isaac_rover_amd import synth
        _scene["s"] = (synth.make_scene(n_cells=128, k=24, n_stones=48), synth.ray_distribution("9"))
    return _scene["s"]


def threshold_table(num_envs=TABLE_ENVS, max_episode_length=3000):
    """-> (st, groups): make_states(seed 77) with the first rows overwritten; ``groups`` names the row ranges.  The hand-placed rows
    come first, so a table cut to fewer envs keeps them; a larger one is padded with further random rows."""
    import torch
    from isaac_rover_amd import synth
    scene, _ = table_scene()
    st = synth.make_states(max(num_envs, 320), 12.8, seed=77)
    st = {k: v.clone() for k, v in st.items()}
    st["progress"] = st["progress"] % (max_episode_length + 1)
    m = int(max_episode_length)
    groups, cur = {}, [0]

    def rows(name, n):
        a = cur[0]
        cur[0] += n
        groups[name] = (a, a + n)
        return range(a, a + n)

    def calm(e):                    # a row no done condition holds for, unless the group sets one: early, upright, 3 m above any stone
        st["progress"][e] = min(5, max(m - 3, 0))
        st["euler_pre"][e, 0:2] = 0.0
        st["pos"][e, 2] = 4.0

    def place_target(e, px, py, tx):
        st["pos"][e, 0], st["pos"][e, 1] = float(px), float(py)
        st["target"][e, 0], st["target"][e, 1] = float(tx), float(py)       # the rover's own y: td = |tx - px|

    # td: pos x = 0 under the 0.18 ladder (tx - 0 is exact), pos x = 4 under 9.5 and 11 (13.5, 15 and their ulp neighbours minus 4 are exact)
    for name, c, px in (("td_goal", TD_GOAL, 0.0), ("td_area", TD_AREA, 4.0), ("td_far", TD_FAR, 4.0)):
        for e, v in zip(rows(name, 9), ladder(F(c) + F(px))):
            calm(e)
            place_target(e, px, 4.0, v)
    for e, (px, tx) in zip(rows("td_exact", 4), ((4.0, 13.5), (4.0, 15.0), (13.5, 4.0), (15.0, 4.0))):
        calm(e)
        place_target(e, px, 4.0, tx)
    for axis, name in ((0, "roll"), (1, "pitch")):
        for e, (s, v) in zip(rows(name, 18), [(s, v) for s in (1.0, -1.0) for v in ladder(TILT)]):
            calm(e)
            st["euler_pre"][e, axis] = float(F(s) * v)
    for e, p in zip(rows("progress", 9), [m - 2, m - 1, m] * 3):
        calm(e)
        st["progress"][e] = p
    gate = F(MOTION_GATE / THREE)
    for hist, name in (("lin_hist", "lin_gate"), ("ang_hist", "ang_gate")):
        for e, (s, v) in zip(rows(name, 18), [(s, v) for s in (1.0, -1.0) for v in ladder(gate)]):
            calm(e)
            st[hist][e, 1] = 0.0
            st[hist][e, 0] = float(F(s) * v)
    tiny = float(np.finfo(F).tiny)
    for e, (l, j) in zip(rows("small", 6), ((-0.0, (0.2, -0.3, 0.1)), (0.0, (-0.2, -0.3, -0.1)), (-tiny, (-0.0, 0.25, -0.5)),
                                            (tiny, (0.4, 0.0, -0.0)), (-0.0, (-0.7, 0.6, 0.5)), (-tiny, (0.01, -0.02, 0.03)))):
        calm(e)
        st["lin_hist"][e, 0] = l
        st["joints"][e, 0:3] = torch.tensor(j)
    # heading: yaw 0, level pose, target at angle ±(1.65 .. 2.45) from the rover's x axis
    angles = [s * (1.65 + 0.1 * k) for s in (1.0, -1.0) for k in range(9)]
    for e, th in zip(rows("heading", 18), angles):
        calm(e)
        st["quat"][e] = torch.tensor([1.0, 0.0, 0.0, 0.0])
        st["target"][e, 0] = st["pos"][e, 0] + 8.0 * float(np.cos(th))
        st["target"][e, 1] = st["pos"][e, 1] + 8.0 * float(np.sin(th))
    # collisions: over the largest stones well inside the map, level pose, a sweep of heights through the wheel threshold
    info = synth.read_stone_info_array(scene.stone_info_raw)
    inside = [i for i in np.argsort(-info[:, 6]) if 2.0 < info[i, 0] < 10.8 and 2.0 < info[i, 1] < 10.8][:4]

    def hang(e, stone, h, roll=0.0, dx=0.0):
        calm(e)
        x, y = float(info[stone, 0]) + dx, float(info[stone, 1])
        st["pos"][e, 0], st["pos"][e, 1] = x, y
        st["pos"][e, 2] = float(synth.surface_height(np.float64(x / 0.1), np.float64(y / 0.1))) + h
        st["quat"][e] = synth.quat_from_euler(torch.tensor([roll]), torch.tensor([0.0]), torch.tensor([0.0]))[0]
        st["joints"][e] = 0.0
        st["target"][e, 0], st["target"][e, 1] = x + 5.0, y + 5.0

    heights = np.linspace(0.3, 1.5, 13)
    for e, (s, h) in zip(rows("hang", 52), [(s, h) for s in inside for h in heights]):
        hang(e, s, float(h))
    for e, (s, h) in zip(rows("sunk", 8), [(s, h) for s in inside[:2] for h in (-1.5, -1.0, -0.5, -0.2)]):
        hang(e, s, h)
    # on its side (roll ±1.45), the front body ray over the stone's centre: the body ray points at the ground, the wheel rays sideways
    body_h = np.linspace(0.15, 0.95, 9)
    for e, (s, r, h) in zip(rows("side", 36), [(s, r, h) for s in inside[:2] for r in (1.45, -1.45) for h in body_h]):
        hang(e, s, float(h), roll=r, dx=-0.34)
    # coinciding conditions
    e0 = list(rows("both", 10))
    for e in e0:
        calm(e)
    for e, p in ((e0[0], m - 1), (e0[1], m)):                    # goal reached and timed out (with / without the increment)
        place_target(e, 0.0, 5.0, 0.1)
        st["progress"][e] = p
    hang(e0[2], inside[0], 0.4)                                  # collision and out of area (td >= 9.5, < 11)
    st["target"][e0[2], 0:2] = st["pos"][e0[2], 0:2] + torch.tensor([10.0, 0.0])
    hang(e0[3], inside[0], 0.4)                                  # collision and td >= 11
    st["target"][e0[3], 0:2] = st["pos"][e0[3], 0:2] + torch.tensor([12.0, 0.0])
    hang(e0[4], inside[1], 0.4)                                  # collision and goal reached
    st["target"][e0[4], 0:2] = st["pos"][e0[4], 0:2] + torch.tensor([0.1, 0.0])
    for e, p in ((e0[5], m - 1), (e0[6], m)):                    # out of area and timed out
        place_target(e, 4.0, 6.0, 14.0)
        st["progress"][e] = p
    st["euler_pre"][e0[7], 0], st["euler_pre"][e0[7], 1] = 1.3, -1.3         # both tilts
    place_target(e0[8], 4.0, 7.0, 16.0)                          # td >= 11 and roll
    st["euler_pre"][e0[8], 0] = -1.2
    hang(e0[9], inside[1], 0.4)                                  # collision and pitch and timeout
    st["euler_pre"][e0[9], 1] = 1.2
    st["progress"][e0[9]] = m
    assert cur[0] <= 320, cur[0]
    st = {k: v[:num_envs].contiguous() for k, v in st.items()}
    return st, groups


def _both_sides(name, below, counts, need=2):
    lo, hi = int(np.count_nonzero(below)), int(np.count_nonzero(~below))
    counts[name] = (lo, hi)
    assert lo >= need and hi >= need, f"threshold table: {name}: {lo} rows on one side, {hi} on the other (need {need} each)"


def coverage(res, cfg, exact=True):
    """Asserts, from a restatement result on the table, that both sides of every threshold are populated, every evaluation code and
    every done cause occurs (alone and combined).  ``exact``: the full table (not a cut one) also holds the exact-threshold rows.
    -> counts per threshold: (rows on the true side, rows on the false side)."""
    c = {}
    td, m = res["td"], int(cfg.max_episode_length)
    _both_sides("td <= 0.18", td <= TD_GOAL, c)
    _both_sides("td >= 9.5", td >= TD_AREA, c)
    _both_sides("td >= 11", td >= TD_FAR, c)
    if exact:
        for v in (TD_GOAL, TD_AREA, TD_FAR):
            assert np.count_nonzero(td == v) >= 1, f"threshold table: no row with td == {v!r}"
            assert np.count_nonzero(td == ulp_steps(v, 1)) and np.count_nonzero(td == ulp_steps(v, -1)), f"no td 1 ulp from {v!r}"
    _both_sides("lin < 0", res["extras_torque_penalty_driving"] < 0, c)
    _both_sides("dl > 0.05", res["dl"] > MOTION_GATE, c)
    _both_sides("da > 0.05", res["da"] > MOTION_GATE, c)
    hd = res["heading"]
    # each sign on its own subset: "both sides" then means beyond and within the gate AMONG the rows of that sign (a table with no
    # row of one sign fails the need=2 count of that line)
    _both_sides("hd > 2", hd[hd > 0] > HEADING_GATE, c)
    _both_sides("hd < -2", hd[hd < 0] < -HEADING_GATE, c)
    _both_sides("progress >= max", res["progress"] >= m, c)
    cause = res["cause"]
    _both_sides("|roll| >= tilt", (cause & 2) != 0, c)
    _both_sides("|pitch| >= tilt", (cause & 4) != 0, c)
    _both_sides("|min wheel| < thr", np.abs(res["min_wheel"]) < F(cfg.wheel_thr), c)
    _both_sides("|min body| < thr", np.abs(res["min_body"]) < F(cfg.body_thr), c)
    if cfg.level >= 2:
        _both_sides("rock_collision", res["rock_collision"] == 1, c)
        # rows the body test alone decides: wheels clear, body within its threshold
        alone = (np.abs(res["min_wheel"]) >= F(cfg.wheel_thr)) & (np.abs(res["min_body"]) < F(cfg.body_thr))
        c["body alone"] = (int(alone.sum()), int((~alone).sum()))
        assert alone.sum() >= 2, "threshold table: no row where only the body rays collide"
    causes = [1, 2, 4, 8, 16] + ([32] if cfg.level >= 2 else [])
    for bit in causes:
        n_alone, n_comb = int(np.count_nonzero(cause == bit)), int(np.count_nonzero(((cause & bit) != 0) & (cause != bit)))
        c["cause %d" % bit] = (n_alone, n_comb)
        assert n_alone >= 1 and n_comb >= 1, f"threshold table: done cause {bit}: {n_alone} rows alone, {n_comb} combined"
    if cfg.evaluation:
        codes = np.bincount(res["eval_code"], minlength=4)
        c["eval codes"] = tuple(int(x) for x in codes)
        assert (codes[:4] > 0).all(), f"threshold table: evaluation codes {codes.tolist()}"
    return c


def compare_bits(got, want, label, float_keys=FLOAT_OUTPUTS, int_keys=INT_OUTPUTS):
    """Float outputs equal as int32 views, integer outputs equal; names the first differing row and term."""
    for k in tuple(float_keys) + tuple(int_keys):
        assert k in got and k in want, f"{label}: output {k!r} is missing on {'the tested' if k not in got else 'the expected'} side"
    for k in float_keys:
        a, b = np.ascontiguousarray(got[k], dtype=F).view(np.int32), np.ascontiguousarray(want[k], dtype=F).view(np.int32)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (f"{label}: {k} differs in {len(bad)} rows, first row {bad[0]}: got {got[k][bad[0]]!r} "
                               f"({a[bad[0]]:#x}) want {want[k][bad[0]]!r} ({b[bad[0]]:#x})")
    for k in int_keys:
        a, b = np.asarray(got[k]).astype(I64), np.asarray(want[k]).astype(I64)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, f"{label}: {k} differs in {len(bad)} rows, first row {bad[0]}: got {a[bad[0]]} want {b[bad[0]]}"
