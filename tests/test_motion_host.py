"""CPU: the terrain-following motion model as DEFINED (tests/motion_ref.py; include/rover_step.h, rover_motion_step) — the plane-fit
constant pinned against the library's host entry, the model's limits (a constant heightfield gives KinematicSim's flat unicycle, the
pose's euler angles are the fitted ones, the turn-on-the-spot rule on both sides of its bound) —, the refusals of rover_motion_step that
need no device (the C layer validates the descriptor before it looks at the ctx) and VecEnv's ``sim`` switch.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as R


def test_symbols_declared_and_exported():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for name in ("rover_motion_step", "rover_motion_plane_fit"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert [f for f, _ in _lib.MotionDesc._fields_] == ["pos3", "quat4", "lin", "ang", "cmd_stride", "E", "substeps", "dt", "max_lin", "max_ang",
                                                        "ride_height", "joint_pos_targets13", "joint_vel_targets13", "joint_pos13", "joint_vel13"]


def test_plane_fit_is_the_pseudo_inverse_of_the_wheel_matrix():
    """rover_motion_plane_fit against numpy.linalg.pinv of [1, a_i, b_i], rounded to float32: bit for bit.  C A = I to 1e-6: A's entries
    are below 1 and C's below 0.6, so the float32 rounding of C moves an entry of C A by at most 6 * 0.6 * 2^-24 = 2.2e-7."""
    from isaac_rover_amd import _lib
    a = R.wheel_matrix()
    assert a.shape == (6, 3) and np.array_equal(a[:, 0], np.ones(6))
    assert np.array_equal(a[:, 1], [0.438, 0.438, 0.0, 0.0, -0.411, -0.411]) and np.array_equal(a[:, 2], [0.385, -0.385, 0.447, -0.447, 0.385, -0.385])
    got = _lib.motion_plane_fit()
    want = np.linalg.pinv(a).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (3, 6)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got, R.plane_fit())
    assert np.abs(got.astype(np.float64) @ a - np.eye(3)).max() <= 1e-6
    assert 2.8 < np.linalg.cond(a) < 3.0
    lib = _lib.load()
    assert lib.rover_motion_plane_fit(None) == -1 and b"motion_plane_fit" in lib.rover_last_error(None)


def test_constant_heightfield_reproduces_the_flat_unicycle():
    """On a constant heightfield the model is KinematicSim.step: yaw' = yaw + w dt, x' = x + v cos(yaw') dt, y' likewise, z = h +
    ride_height, a pure-yaw quaternion (away from the turn-on-the-spot rule, which KinematicSim does not have).  The rows of the float32 C
    sum to (1, 0, 0) within 6 * 2^-25 each, so z_c = h and p = q = 0 within 2e-7 h; 1e-6 covers it."""
    rng = np.random.default_rng(3)
    n, h, ride, dt = 200, 0.37, 0.3, 0.05
    field = R.Field(np.full((40, 56), h, dtype=np.float32), 0.05, 1.0, (-0.2, 0.1))
    yaw0 = rng.uniform(-3.0, 3.0, n)
    quat = np.stack((np.cos(yaw0 / 2), np.zeros(n), np.zeros(n), np.sin(yaw0 / 2)), 1).astype(np.float32)
    pos = np.concatenate((rng.uniform(-1, 3, (n, 2)), rng.uniform(-1, 1, (n, 1))), 1).astype(np.float32)
    ang = rng.uniform(-1, 1, n).astype(np.float32)
    lin = (np.abs(ang) * rng.uniform(0.5, 1.0, n) * rng.choice((-1.0, 1.0), n)).astype(np.float32)      # |v / w| >= 0.5
    out = R.step(field, pos, quat, lin, ang, dt=dt, ride_height=ride)
    q64 = quat.astype(np.float64)
    yaw = 2.0 * np.arctan2(q64[:, 3], q64[:, 0]) + ang.astype(np.float64) * np.float64(np.float32(dt))       # vec_env.KinematicSim.step
    step = lin.astype(np.float64) * np.float64(np.float32(dt))
    want_pos = np.stack((pos[:, 0] + step * np.cos(yaw), pos[:, 1] + step * np.sin(yaw), np.full(n, np.float64(np.float32(h)) + np.float32(ride))), 1)
    want_quat = np.stack((np.cos(yaw / 2), np.zeros(n), np.zeros(n), np.sin(yaw / 2)), 1)
    assert np.abs(out["pos"] - want_pos).max() <= 1e-6
    sign = np.sign((out["quat"] * want_quat).sum(1))[:, None]
    assert np.abs(out["quat"] * sign - want_quat).max() <= 1e-6
    assert np.abs(out["roll"]).max() <= 1e-6 and np.abs(out["pitch"]).max() <= 1e-6


def test_pose_euler_angles_are_the_fitted_ones():
    """tensor_quat_to_eul of the model's quaternion is (roll, pitch, yaw1) to 1e-12 in float64, slopes up to 5 (79 degrees) included; and
    the roll is the one that puts the body's y axis into the plane z = p a + q b."""
    rng = np.random.default_rng(11)
    n = 500
    p, q = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    p[:4], q[:4] = (5.0, -5.0, 0.0, 5.0), (5.0, 5.0, 0.0, -5.0)
    yaw = rng.uniform(-6.0, 6.0, n)                                   # past +-pi: the quaternion's yaw is the wrapped one
    roll, pitch, quat = R.orientation(p, q, yaw)
    assert np.abs(np.linalg.norm(quat, axis=1) - 1).max() <= 1e-12
    eul = R.quat_to_eul(quat)
    assert np.abs(eul[:, 0] - roll).max() <= 1e-12 and np.abs(eul[:, 1] - pitch).max() <= 1e-12
    dy = eul[:, 2] - yaw
    assert np.abs(dy - 2 * np.pi * np.round(dy / (2 * np.pi))).max() <= 1e-12
    assert np.abs(p).max() == 5.0 and np.abs(q).max() == 5.0
    # the body axes in the heading frame (a forward, b left, z up): R = Ry(pitch) Rx(roll) there; x and y lie in the plane
    bx = np.stack((np.cos(pitch), np.zeros(n), -np.sin(pitch)), 1)
    by = np.stack((np.sin(pitch) * np.sin(roll), np.cos(roll), np.cos(pitch) * np.sin(roll)), 1)
    for b in (bx, by):
        assert np.abs(b[:, 2] - (p * b[:, 0] + q * b[:, 1])).max() <= 1e-12


def _ladder(centre, steps):
    """``centre`` and its ``steps`` float32 neighbours on each side."""
    up, down = [centre], [centre]
    for _ in range(steps):
        up.append(np.nextafter(up[-1], np.float32(np.inf)))
        down.append(np.nextafter(down[-1], np.float32(-np.inf)))
    return np.array(down[:0:-1] + up, dtype=np.float32)


def test_turn_on_the_spot_rule_on_both_sides_of_its_bound():
    """v is kept where the float32 quotient |v / w| is ABOVE float32(0.45), else the rover turns on the spot: float32 ladders of v around
    0.45 w for several w of both signs; w = 0 keeps v; v = w = 0 gives 0.  The expected side comes from the exactly rounded quotient
    (a float64 division of two float32 values, rounded to float32, is the float32 division)."""
    bound = np.float32(0.45)
    kept = dropped = 0
    for w in np.array([0.3, -0.3, 1.0, -1.0, 0.0123, -0.77, 2.0 ** -10], dtype=np.float32):
        for sign in (1.0, -1.0):
            v = _ladder(np.float32(sign) * (bound * np.abs(w)), 4)
            ws = np.full_like(v, w)
            got = R.effective_speed(v, ws)
            quotient = np.abs(v.astype(np.float64) / np.float64(w)).astype(np.float32)
            keep = quotient > bound
            assert np.array_equal(got, np.where(keep, v, np.float32(0))), (w, sign)
            assert got.dtype == np.float32 and keep.any() and not keep.all(), (w, sign)         # the ladder straddles the bound
            assert np.array_equal(keep, np.sort(keep)) or np.array_equal(keep, np.sort(keep)[::-1])      # one switch along the ladder
            kept, dropped = kept + int(keep.sum()), dropped + int((~keep).sum())
            # the float64 model takes the same side wherever the exact quotient is not within an ulp of the bound
            got64 = R.effective_speed(v.astype(np.float64), ws.astype(np.float64))
            far = np.abs(v.astype(np.float64) / np.float64(w)) - np.float64(bound)
            sel = np.abs(far) > 1e-7
            assert np.array_equal(got64[sel] != 0, keep[sel])
    assert kept >= 14 and dropped >= 14
    v = np.array([0.5, -0.5, 1e-30, 0.0, -0.0], dtype=np.float32)
    assert np.array_equal(R.effective_speed(v, np.zeros_like(v)), np.array([0.5, -0.5, 1e-30, 0.0, 0.0], dtype=np.float32))
    assert np.array_equal(R.effective_speed(np.float32([0.0, 0.0]), np.float32([0.7, -0.7])), np.float32([0.0, 0.0]))
    # in the whole step: a rover below the bound turns but does not move
    field = R.Field(np.zeros((8, 8), dtype=np.float32), 0.05, 1.0, (0.0, 0.0))
    pos, quat = np.zeros((2, 3), dtype=np.float32), np.float32([[1, 0, 0, 0], [1, 0, 0, 0]])
    out = R.step(field, pos, quat, np.float32([0.2, 0.5]), np.float32([1.0, 1.0]), dt=0.05)
    assert np.array_equal(out["pos"][0, :2], [0.0, 0.0]) and out["pos"][1, 0] > 0.02
    assert np.allclose(out["yaw"], 0.05, atol=1e-9)


def test_boundary_distance():
    field = R.Field(np.zeros((10, 6), dtype=np.float32), 0.5, 1.0, (1.0, -1.0))
    c = np.zeros((1, 3, 6, 2))
    c[0, :, :, 0], c[0, :, :, 1] = 2.0, 0.0                     # scaled (2, 2): half a cell from every boundary
    c[0, 1, 3, 0] = 1.0 + 0.5 * 2.4999                          # scaled 2.4999
    c[0, 2, 5, 1] = -50.0                                       # clamped to 0
    assert np.allclose(R.boundary_distance(field, c), [0.5, 1e-4, 0.5], atol=1e-12)


def test_descriptor_refusals_need_no_device():
    """Every ROVER_E_INVALID of rover_motion_step is decided from the descriptor alone: with a NULL ctx each is reported by name, and a
    descriptor that passes them all is then refused for the NULL ctx."""
    from isaac_rover_amd import _lib
    lib = _lib.load()
    D = _lib.motion_desc

    def call(d):
        rc = lib.rover_motion_step(None, None if d is None else C.byref(d), None)
        return rc, lib.rover_last_error(None).decode()

    bad = [("null descriptor", None, "null descriptor"), ("E < 0", D(-1), "negative"), ("substeps 0", D(4, substeps=0), "substeps"),
           ("cmd_stride 0", D(4, cmd_stride=0), "cmd_stride"), ("dt 0", D(4, dt=0.0), "dt"), ("dt < 0", D(4, dt=-0.05), "dt"),
           ("dt nan", D(4, dt=float("nan")), "dt"), ("dt inf", D(4, dt=float("inf")), "dt"),
           ("no pos", D(4, pos3=None), "pos3"), ("no quat", D(4, quat4=None), "quat4"), ("no lin", D(4, lin=None), "lin"), ("no ang", D(4, ang=None), "ang")]
    names = ("joint_pos_targets13", "joint_vel_targets13", "joint_pos13", "joint_vel13")
    for mask in range(1, 15):                                   # every partial joint quadruple
        bad.append((f"joints {mask:04b}", D(4, **{n: 16 for i, n in enumerate(names) if mask >> i & 1}), "go together"))
    for what, d, word in bad:
        rc, msg = call(d)
        assert rc == -1 and msg.startswith("motion_step:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    for d in (D(4), D(0), D(0, pos3=None, quat4=None, lin=None, ang=None), D(4, **{n: 16 for n in names})):
        assert call(d) == (-1, "motion_step: null ctx")


def test_vec_env_sim_switch():
    from isaac_rover_amd import vec_env

    class Task:
        num_envs, observation_space, action_space = 3, None, None

        def set_up_scene(self, spawn_positions=None):
            pass

        def post_reset(self):
            pass

    assert set(vec_env.SIMS) == {"kinematic", "terrain"}
    for bad in ("physx", "", None, "Terrain"):
        with pytest.raises(ValueError, match="sim must be one of"):
            vec_env.VecEnv(sim=bad)
    for kw, cls in (({}, vec_env.KinematicSim), ({"sim": "kinematic"}, vec_env.KinematicSim), ({"sim": "terrain"}, vec_env.TerrainSim)):
        env = vec_env.VecEnv(headless=True, **kw)
        env.set_task(Task(), sim_params={"dt": 0.02})
        assert type(env._world) is cls and env._world.dt == 0.02 and env._world.is_playing()
    assert not hasattr(vec_env.KinematicSim, "advance") and hasattr(vec_env.TerrainSim, "advance")
