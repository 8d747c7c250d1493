"""Independent restatement of the rocker-bogie posture mode of the motion model (include/rover_step.h, rover_motion_step_bogie;
DESIGN.md §4.22) in numpy, written from the definition and not from the kernel.  `step(..., dtype=np.float64)` is the model in double,
`step(..., dtype=np.float32)` the same operations with one float32 rounding each.  Steps 1-3 (commands, heading, position) and the
heightfield lookup are those of tests/motion_ref.py; what is new is the wheel layout of the wheel rays, the forward map F(u) of the six
wheel-frame origins through the reference's suspension chain, its Jacobian at rest, and the chord iteration with the constant inverse.
"""
import numpy as np

import motion_ref as M

# rock_detect.py:201-215: the wheel frame's origin is  T1 + Rsus (T0)  in the body frame, in the order FL, FR, CL, CR, RL, RR
WP0 = ((0.286, 0.385, -0.197), (0.286, -0.385, -0.197), (-0.146, 0.447, -0.197), (-0.146, -0.447, -0.197),
       (-0.440, 0.385, -0.197), (-0.440, -0.385, -0.197))
WP1 = ((0.153, 0.0, 0.03),) * 4 + ((0.0, 0.0, 0.03),) * 2
# (forward a_i, left b_i) of the origins with all joints at 0, and their common body z
LAYOUT = ((0.439, 0.385), (0.439, -0.385), (0.007, 0.447), (0.007, -0.447), (-0.440, 0.385), (-0.440, -0.385))
ORIGIN_Z = 0.167                     # the origins lie at body z = -0.167
ITERS, MAX_BOGIE = 4, 0.6


def _suspension(j, i):
    """(susX, susY) of wheel i from the joint angles j = (j0, j1, j2) (rock_detect.py:263-264)."""
    zero = np.zeros_like(j[0])
    sus_y = (-j[0], j[1], -j[0], j[1], zero, zero)[i]
    sus_x = (zero, zero, zero, zero, -j[2], -j[2])[i]
    return sus_x, sus_y


def body_points(j, dtype, const=np.float32):
    """The six wheel-frame origins in the body frame for joint angles j = (j0, j1, j2), arrays [n] -> list of (x, y, z), through
    rock_detect.py:256-258 with zero steering and :275-277.  Wheels 0-3 have susX = 0 and wheels 4, 5 susY = 0 identically, so the
    factors cos 0 = 1 and sin 0 = 0 are left out: the operations written here are the ones the kernel does.  The constants are the
    kernel's float32 ones; ``const=np.float64`` takes the decimal constants themselves, from which the Jacobian is derived."""
    t = np.dtype(dtype).type
    pts = []
    for i in range(6):
        x0, y0, z0 = (t(const(v)) for v in WP0[i])
        t1x, t1z = t(const(WP1[i][0])), t(const(WP1[i][2]))
        sus_x, sus_y = _suspension(j, i)
        if i < 4:
            ssy, csy = np.sin(sus_y), np.cos(sus_y)
            pts.append(((t1x + x0 * csy) - ssy * z0, np.full_like(sus_y, y0), (t1z + x0 * ssy) + csy * z0))
        else:
            ssx, csx = np.sin(sus_x), np.cos(sus_x)
            c1 = z0 * csx - y0 * ssx
            pts.append((np.full_like(sus_x, x0), y0 * csx + z0 * ssx, t1z + c1))
    return pts


def forward(u, dtype=np.float64, const=np.float32):
    """F(u): the world z of the six wheel-frame origins, [n, 6], for u = (z_c, roll, pitch, j0, j1, j2) as six arrays [n]: the body
    points through the third row (-sin pitch, cos pitch sin roll, cos pitch cos roll) of the ZYX body rotation."""
    zc, roll, pitch = u[0], u[1], u[2]
    sr, cr, sp, cp = np.sin(roll), np.cos(roll), np.sin(pitch), np.cos(pitch)
    out = []
    for bx, by, bz in body_points(u[3:6], dtype, const):
        cc = bz * cr + by * sr
        out.append((zc - bx * sp) + cp * cc)
    return np.stack(out, axis=1)


def world_points(pos, eul, j):
    """The six wheel-frame origins in the world, [n, 6, 3] float64, for poses pos [n, 3], ZYX euler angles eul [n, 3] and joints j [n, 3]
    — the full ZYX rotation, of which `forward` uses the third row."""
    pos, eul, j = (np.asarray(a, dtype=np.float64) for a in (pos, eul, j))
    sr, cr, sp, cp, sy, cy = np.sin(eul[:, 0]), np.cos(eul[:, 0]), np.sin(eul[:, 1]), np.cos(eul[:, 1]), np.sin(eul[:, 2]), np.cos(eul[:, 2])
    rot = np.stack((np.stack((cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr), 1),
                    np.stack((sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr), 1),
                    np.stack((-sp, cp * sr, cp * cr), 1)), 1)                              # [n, 3, 3]
    body = np.stack([np.stack(p, 1) for p in body_points((j[:, 0], j[:, 1], j[:, 2]), np.float64)], 1)      # [n, 6, 3]
    return pos[:, None, :] + np.einsum("nrc,nwc->nwr", rot, body)


def jacobian():
    """J = dF/du at u = 0, [6, 6] float64, analytically: dF_i/dz_c = 1, dF_i/droll = b_i, dF_i/dpitch = -a_i; a wheel on a bogie
    swings about its pivot: dF_i/dj0 = -x0_i (FL, CL), dF_i/dj1 = +x0_i (FR, CR), dF_i/dj2 = +-y0_i (RL, RR)."""
    jm = np.zeros((6, 6))
    for i in range(6):
        jm[i, 0], jm[i, 1], jm[i, 2] = 1.0, LAYOUT[i][1], -LAYOUT[i][0]
    jm[0, 3], jm[2, 3] = -WP0[0][0], -WP0[2][0]
    jm[1, 4], jm[3, 4] = WP0[1][0], WP0[3][0]
    jm[4, 5], jm[5, 5] = WP0[4][1], WP0[5][1]
    return jm


def chord_inverse():
    """D [6, 6] = inv(J) in double, rounded to float32 once."""
    return np.linalg.inv(jacobian()).astype(np.float32)


def solve(target, iters=ITERS, dtype=np.float64, const=np.float32):
    """The chord iteration from u = 0 on targets [n, 6]: u <- u + D (t - F(u)), `iters` times, each row of D r summed from i = 0
    upwards.  -> (u as a list of six arrays, the residuals max_i |t_i - F(u)_i| after every iteration [iters, n])."""
    dtype = np.dtype(dtype)
    d = chord_inverse().astype(dtype)
    target = np.asarray(target, dtype=dtype)
    u = [np.zeros(target.shape[0], dtype=dtype) for _ in range(6)]
    res = []
    for _ in range(int(iters)):
        r = target - forward(u, dtype, const)
        u = [u[k] + sum((d[k, i] * r[:, i] for i in range(1, 6)), d[k, 0] * r[:, 0]) for k in range(6)]
        res.append(np.abs(target.astype(np.float64) - forward([a.astype(np.float64) for a in u], np.float64, const)).max(1))
    return u, np.stack(res)


def step(field, pos, quat, lin, ang, *, dt, substeps=1, max_lin=1.0, max_ang=1.0, ride_height=0.3, iters=ITERS, max_bogie=MAX_BOGIE,
         dtype=np.float64, const=np.float32):
    """``substeps`` sub-steps on copies of ``pos`` [E, 3] and ``quat`` [E, 4] (float32 inputs, taken exactly).  -> dict: pos, quat,
    roll, pitch, yaw (the last sub-step's angles, yaw not wrapped), joints [E, 3] (clamped), joints_raw [E, 3] (the last solve's),
    residual [E] (the last solve's, in float64), target [E, 6] and contacts [substeps, E, 6, 2].  ``const=np.float64`` takes the
    layout's decimal constants themselves in place of the kernel's float32 ones (0.007f differs from 0.153f - 0.146f by 9e-10 m)."""
    dtype = np.dtype(dtype)
    t = dtype.type
    pos, quat = np.array(pos, dtype=np.float32).astype(dtype), np.array(quat, dtype=np.float32).astype(dtype)
    dt_, lim = t(np.float32(dt)), t(np.float32(max_bogie))
    off = t(np.float32(ride_height)) - t(const(ORIGIN_Z))
    v = np.asarray(lin, dtype=np.float32).astype(dtype) * t(np.float32(max_lin))
    w = np.asarray(ang, dtype=np.float32).astype(dtype) * t(np.float32(max_ang))
    v_eff = M.effective_speed(v, w)
    x, y = pos[:, 0], pos[:, 1]
    out = dict(contacts=[])
    for _ in range(int(substeps)):
        yaw = M.yaw_of(quat) + w * dt_
        c, s = np.cos(yaw), np.sin(yaw)
        x = x + (v_eff * c) * dt_
        y = y + (v_eff * s) * dt_
        wx = [(x + t(const(a)) * c) - t(const(b)) * s for a, b in LAYOUT]
        wy = [(y + t(const(a)) * s) + t(const(b)) * c for a, b in LAYOUT]
        target = np.stack([field.height(wx[i], wy[i], dtype) + off for i in range(6)], 1)
        u, res = solve(target, iters, dtype, const)
        quat = M.euler_to_quat(u[1], u[2], yaw)
        z = u[0]
        out["contacts"].append(np.stack((np.stack(wx, 1), np.stack(wy, 1)), axis=2))
    raw = np.stack(u[3:6], 1)
    out.update(pos=np.stack((x, y, z), 1), quat=quat, roll=u[1], pitch=u[2], yaw=yaw, joints_raw=raw,
               joints=np.minimum(np.maximum(raw, -lim), lim), residual=res[-1], residuals=res, target=target, contacts=np.stack(out["contacts"]))
    return out
