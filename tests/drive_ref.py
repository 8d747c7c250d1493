"""Independent restatement of the wheel-level drive mode of the motion model (include/rover_step.h, rover_motion_step_drive; DESIGN.md
§4.24) in numpy, written from the definition and not from the kernel.  `step(..., dtype=np.float64)` is the model in double,
`step(..., dtype=np.float32)` the same operations with one float32 rounding each (every operand is a float32 array or scalar).  The
heading, the heightfield lookup, the plane fit and the ZYX quaternion are those of tests/motion_ref.py, the bogie solve that of
tests/bogie_ref.py; what is new is the rate-limited actuators, the wheel velocity vectors, the least-squares body twist and the slip.

``wrong=`` selects one deliberately wrong variant, so that a test can show that the restatement tells them apart:
"yaw_from_command" (the heading integrates ``w_cmd`` instead of the fitted w), "no_landing" (rule 1 as a clipped step, without taking
the target itself), "rl_sign" (RL's steering angle read as -j7, as the wheel rays read it), "sum_order" (P's rows summed from the last
column downwards).
"""
import numpy as np

import bogie_ref as B
import motion_ref as M

STEER_COLS = (4, 6, None, None, 7, 8)         # FL, FR, ML, MR, RL, RR: the joint_pos column of the steering angle (the centre pair has none)
DRIVE_COLS = (9, 10, 3, 5, 11, 12)            # the joint_vel column of the wheel speed
STEERED = tuple(c for c in STEER_COLS if c is not None)
WHEEL_RADIUS = 0.2                            # kinematics.py:18,61 divides the ground speed by wheel_diameter = 0.2


def rigid_matrix():
    """M [12, 3] float64: a rigid motion (vx, vy, w) gives wheel i the velocity (vx - w b_i, vy + w a_i), a_i = f_i, b_i = -r_i."""
    rows = []
    for r, f in M.WHEELS:
        rows += [[1.0, 0.0, r], [0.0, 1.0, f]]
    return np.array(rows, dtype=np.float64)


def drive_fit():
    """P [3, 12] = pinv(M) in double, rounded to float32 once.  sum b_i = 0, so vx is the mean of the x components: the six entries
    that pair vx with a y component are exactly 0 (test_drive_host shows it in rational arithmetic), where pinv's SVD leaves rounding
    noise of some 1e-17; that noise is set to the 0 it stands for (every other entry is above 1e-2 in magnitude)."""
    p = np.linalg.pinv(rigid_matrix())
    p[np.abs(p) < 1e-12] = 0.0
    return p.astype(np.float32)


def rate_limit(state, target, step, wrong=None):
    """Rule 1: the target where it is within ``step``, else one step towards it; a NaN difference takes the target."""
    d = target - state
    with np.errstate(invalid="ignore"):
        if wrong == "no_landing":
            return state + np.minimum(np.maximum(d, -step), step)
        return np.where(np.abs(d) > step, state + np.copysign(step, d), target)


def wheel_vectors(delta, omega, wheel_radius, wrong=None):
    """Step 2 -> the 12 components t [12] of arrays [n]: delta [4] (FL, FR, RL, RR), omega [6]."""
    sign = delta[0].dtype.type(-1.0) if wrong == "rl_sign" else delta[0].dtype.type(1.0)
    angle = {0: delta[0], 1: delta[1], 4: sign * delta[2], 5: delta[3]}
    t = []
    for i in range(6):
        s = wheel_radius * omega[i]
        t += [s * np.cos(angle[i]), s * np.sin(angle[i])] if i in angle else [s, np.zeros_like(s)]
    return t


def twist(t, fit, wrong=None):
    """Step 3 -> (vx, vy, w): each row of P t summed from column 0 upwards."""
    order = list(range(12))[::-1] if wrong == "sum_order" else list(range(12))
    out = []
    for r in range(3):
        acc = fit[r, order[0]] * t[order[0]]
        for j in order[1:]:
            acc = acc + fit[r, j] * t[j]
        out.append(acc)
    return out


def slip_of(t, tw, dtype):
    """Step 4: the root mean square of the wheels' velocity against the rigid motion."""
    k = dtype.type
    total = None
    for i, (r, f) in enumerate(M.WHEELS):
        dx = (tw[0] + tw[2] * k(np.float32(r))) - t[2 * i]
        dy = (tw[1] + tw[2] * k(np.float32(f))) - t[2 * i + 1]
        q = dx * dx + dy * dy
        total = q if total is None else total + q
    return np.sqrt(total / k(6.0))


def plane_posture(field, x, y, yaw, c, s, ride, dtype):
    """Steps 4-7 of rover_motion_step, as tests/motion_ref.py:step writes them -> (z, quat, contacts [E, 6, 2])."""
    k = dtype.type
    fit = M.plane_fit().astype(dtype)
    wx = [(x + k(np.float32(f)) * c) + k(np.float32(r)) * s for r, f in M.WHEELS]
    wy = [(y + k(np.float32(f)) * s) - k(np.float32(r)) * c for r, f in M.WHEELS]
    zs = [field.height(wx[i], wy[i], dtype) for i in range(6)]
    zc, p, q = (sum((fit[n, i] * zs[i] for i in range(1, 6)), fit[n, 0] * zs[0]) for n in range(3))
    _, _, quat = M.orientation(p, q, yaw)
    return zc + ride, quat, None, np.stack((np.stack(wx, 1), np.stack(wy, 1)), axis=2)


def bogie_posture(field, x, y, yaw, c, s, ride, dtype, iters, lim):
    """Steps 4-7 of rover_motion_step_bogie, as tests/bogie_ref.py:step writes them -> (z, quat, clamped joints [E, 3], contacts)."""
    k = dtype.type
    off = ride - k(np.float32(B.ORIGIN_Z))
    wx = [(x + k(np.float32(a)) * c) - k(np.float32(b)) * s for a, b in B.LAYOUT]
    wy = [(y + k(np.float32(a)) * s) + k(np.float32(b)) * c for a, b in B.LAYOUT]
    target = np.stack([field.height(wx[i], wy[i], dtype) + off for i in range(6)], 1)
    u, _ = B.solve(target, iters, dtype)
    raw = np.stack(u[3:6], 1)
    return u[0], M.euler_to_quat(u[1], u[2], yaw), np.minimum(np.maximum(raw, -lim), lim), np.stack((np.stack(wx, 1), np.stack(wy, 1)), axis=2)


def step(field, pos, quat, joints, *, dt, substeps=1, ride_height=0.3, wheel_radius=WHEEL_RADIUS, steer_rate=np.inf, wheel_accel=np.inf,
         suspension="plane", iters=B.ITERS, max_bogie=B.MAX_BOGIE, dtype=np.float64, wrong=None, w_cmd=None):
    """``substeps`` sub-steps on copies of ``pos`` [E, 3], ``quat`` [E, 4] and ``joints`` = (joint_pos_targets, joint_vel_targets,
    joint_pos, joint_vel), each [E, 13] (float32 inputs, taken exactly).  ``field`` None: no posture (z and the quaternion's tilt stay
    out; the quaternion is the pure yaw one).  -> dict: pos, quat, joint_pos, joint_vel [E, 13], slip [E], twist [E, 3] (the last
    sub-step's vx, vy, w), yaw and contacts [substeps, E, 6, 2]."""
    dtype = np.dtype(dtype)
    k = dtype.type
    pos, quat = np.array(pos, dtype=np.float32).astype(dtype), np.array(quat, dtype=np.float32).astype(dtype)
    pt, vt, jp, jv = (np.array(a, dtype=np.float32).astype(dtype) for a in joints)
    dt_, ride, radius = k(np.float32(dt)), k(np.float32(ride_height)), k(np.float32(wheel_radius))
    with np.errstate(over="ignore"):
        step_s, step_w = k(np.float32(steer_rate)) * dt_, k(np.float32(wheel_accel)) * dt_
    fit = drive_fit().astype(dtype)
    delta, omega = [jp[:, c] for c in STEERED], [jv[:, c] for c in DRIVE_COLS]
    delta_t, omega_t = [pt[:, c] for c in STEERED], [vt[:, c] for c in DRIVE_COLS]
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    bent = None
    contacts = []
    for _ in range(int(substeps)):
        delta = [rate_limit(delta[j], delta_t[j], step_s, wrong) for j in range(4)]
        omega = [rate_limit(omega[i], omega_t[i], step_w, wrong) for i in range(6)]
        with np.errstate(invalid="ignore"):
            t = wheel_vectors(delta, omega, radius, wrong)
            tw = twist(t, fit, wrong)
            turn = np.asarray(w_cmd, dtype=np.float32).astype(dtype) if wrong == "yaw_from_command" else tw[2]
            yaw = M.yaw_of(quat) + turn * dt_
            c, s = np.cos(yaw), np.sin(yaw)
            x = x + ((tw[0] * c) - (tw[1] * s)) * dt_
            y = y + ((tw[0] * s) + (tw[1] * c)) * dt_
            if field is None:
                quat = M.euler_to_quat(np.zeros_like(yaw), np.zeros_like(yaw), yaw)
            elif suspension == "bogie":
                z, quat, bent, cont = bogie_posture(field, x, y, yaw, c, s, ride, dtype, iters, k(np.float32(max_bogie)))
                contacts.append(cont)
            else:
                z, quat, bent, cont = plane_posture(field, x, y, yaw, c, s, ride, dtype)
                contacts.append(cont)
    with np.errstate(invalid="ignore"):
        slip = slip_of(t, tw, dtype)
    joint_pos, joint_vel = pt.copy(), vt.copy()
    for j, col in enumerate(STEERED):
        joint_pos[:, col] = delta[j]
    for i, col in enumerate(DRIVE_COLS):
        joint_vel[:, col] = omega[i]
    if bent is not None:
        joint_pos[:, 0:3] = bent
    return dict(pos=np.stack((x, y, z), 1), quat=quat, joint_pos=joint_pos, joint_vel=joint_vel, slip=slip, twist=np.stack(tw, 1), yaw=yaw,
                contacts=np.stack(contacts) if contacts else None)
