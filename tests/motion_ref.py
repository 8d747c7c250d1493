"""Independent restatement of the terrain-following motion model (include/rover_step.h, rover_motion_step) in numpy,
written from the definition and not from the kernel: `step(..., dtype=np.float64)` is the model in double, `step(..., dtype=np.float32)`
the same operations with one float32 rounding each (every operand is a float32 array, so numpy rounds after every operation);
`boundary_distance` lists how far every wheel contact's scaled coordinate lies from the next rounding boundary of the height lookup, so
that a test can leave out the envs in which a last-bit difference of a coordinate picks another cell.
"""
import numpy as np

# (right r_i, forward f_i) of FL, FR, ML, MR, RL, RR (the reference's tasks/utils/kinematics.py:20-25)
WHEELS = ((-0.385, 0.438), (0.385, 0.438), (-0.447, 0.0), (0.447, 0.0), (-0.385, -0.411), (0.385, -0.411))
BOUND = np.float32(0.45)            # turn on the spot at or below this |v / w| (kinematics.py:31, compared in float32)


def wheel_matrix():
    """A [6, 3] = [1, a_i, b_i] with a_i = f_i (forward) and b_i = -r_i (left), float64."""
    return np.array([[1.0, f, -r] for r, f in WHEELS], dtype=np.float64)


def plane_fit():
    """C [3, 6] = pinv(A) in double, rounded to float32 once: (z_c, p, q) = C z."""
    return np.linalg.pinv(wheel_matrix()).astype(np.float32)


class Field:
    """A heightfield as rover_set_heightfield takes it: heights [N0, N1] float32, the two scales and the shift as float32 values,
    ``rcp`` the cell_index_mode (0: divide by the cell size, 1: multiply by its float32 reciprocal)."""

    def __init__(self, heights, horizontal_scale, vertical_scale, shift, rcp=0):
        self.hm = np.ascontiguousarray(heights, dtype=np.float32)
        self.hscale, self.vscale = np.float32(horizontal_scale), np.float32(vertical_scale)
        self.shift = (np.float32(shift[0]), np.float32(shift[1]))
        self.rcp = int(rcp)

    def scaled(self, v, axis, dtype):
        """The scaled, clamped coordinate before rounding (get_pos_height, rover.py:590-592: the clamp bound is the dim-0 size on both axes)."""
        t = dtype.type
        d = v - t(self.shift[axis])
        s = d * t(np.float32(1.0) / self.hscale) if self.rcp else d / t(self.hscale)
        return np.minimum(np.maximum(s, t(0.0)), t(self.hm.shape[0] - 1))

    def height(self, x, y, dtype):
        """rover.py:594-606: round half to even, look up, scale (the y index is also held inside the map's second dimension)."""
        ix = np.rint(self.scaled(x, 0, dtype)).astype(np.int64)
        iy = np.minimum(np.rint(self.scaled(y, 1, dtype)).astype(np.int64), self.hm.shape[1] - 1)
        return self.hm[ix, iy].astype(dtype) * dtype.type(self.vscale)


def effective_speed(v, w):
    """Turn on the spot (kinematics.py:34-39): v where |v / w| > 0.45, else 0; w = 0 keeps a non-zero v, v = w = 0 gives 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.abs(v / w)
    return np.where(ratio > ratio.dtype.type(BOUND), v, ratio.dtype.type(0.0))


def yaw_of(quat):
    w, x, y, z = (quat[..., i] for i in range(4))
    t = quat.dtype.type
    return np.arctan2(t(2.0) * (w * z + x * y), t(1.0) - t(2.0) * (y * y + z * z))


def quat_to_eul(quat):
    """The reference's tensor_quat_to_eul (ZYX, quaternion w x y z) -> [..., 3] roll, pitch, yaw."""
    w, x, y, z = (quat[..., i] for i in range(4))
    t = quat.dtype.type
    roll = np.arctan2(t(2.0) * (w * x + y * z), t(1.0) - t(2.0) * (x * x + y * y))
    sinp = t(2.0) * (w * y - z * x)
    with np.errstate(invalid="ignore"):
        pitch = np.where(sinp - t(1.0) >= 0, np.copysign(t(np.pi / 2), sinp), np.arcsin(np.clip(sinp, -1, 1)))
    return np.stack((roll, pitch, yaw_of(quat)), axis=-1)


def euler_to_quat(roll, pitch, yaw):
    """The standard ZYX formula on the half angles -> [..., 4] (w, x, y, z)."""
    h = roll.dtype.type(0.5)
    cr, sr, cp, sp, cy, sy = np.cos(roll * h), np.sin(roll * h), np.cos(pitch * h), np.sin(pitch * h), np.cos(yaw * h), np.sin(yaw * h)
    return np.stack(((cr * cp) * cy + (sr * sp) * sy, (sr * cp) * cy - (cr * sp) * sy,
                     (cr * sp) * cy + (sr * cp) * sy, (cr * cp) * sy - (sr * sp) * cy), axis=-1)


def orientation(p, q, yaw):
    """Step 6: pitch = -atan(p), roll = atan(q cos(pitch)) -> (roll, pitch, quaternion)."""
    pitch = -np.arctan(p)
    roll = np.arctan(q * np.cos(pitch))
    return roll, pitch, euler_to_quat(roll, pitch, yaw)


def step(field, pos, quat, lin, ang, *, dt, substeps=1, max_lin=1.0, max_ang=1.0, ride_height=0.3, dtype=np.float64):
    """``substeps`` sub-steps on copies of ``pos`` [E, 3] and ``quat`` [E, 4] (float32 inputs, taken exactly).  -> dict: pos, quat,
    roll, pitch, yaw (the last sub-step's euler angles, yaw not wrapped), p, q (its plane slopes) and contacts [substeps, E, 6, 2]
    (the wheel contacts' world coordinates)."""
    dtype = np.dtype(dtype)
    t = dtype.type
    pos, quat = np.array(pos, dtype=np.float32).astype(dtype), np.array(quat, dtype=np.float32).astype(dtype)
    fit = plane_fit().astype(dtype)
    dt_, ride = t(np.float32(dt)), t(np.float32(ride_height))
    v = np.asarray(lin, dtype=np.float32).astype(dtype) * t(np.float32(max_lin))
    w = np.asarray(ang, dtype=np.float32).astype(dtype) * t(np.float32(max_ang))
    v_eff = effective_speed(v, w)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    out = dict(contacts=[])
    for _ in range(int(substeps)):
        yaw = yaw_of(quat) + w * dt_
        c, s = np.cos(yaw), np.sin(yaw)
        x = x + (v_eff * c) * dt_
        y = y + (v_eff * s) * dt_
        wx = [(x + t(np.float32(f)) * c) + t(np.float32(r)) * s for r, f in WHEELS]
        wy = [(y + t(np.float32(f)) * s) - t(np.float32(r)) * c for r, f in WHEELS]
        zs = [field.height(wx[i], wy[i], dtype) for i in range(6)]
        zc, p, q = (sum((fit[k, i] * zs[i] for i in range(1, 6)), fit[k, 0] * zs[0]) for k in range(3))
        roll, pitch, quat = orientation(p, q, yaw)
        z = zc + ride
        out["contacts"].append(np.stack((np.stack(wx, 1), np.stack(wy, 1)), axis=2))
    out.update(pos=np.stack((x, y, z), 1), quat=quat, roll=roll, pitch=pitch, yaw=yaw, p=p, q=q, contacts=np.stack(out["contacts"]))
    return out


def boundary_distance(field, contacts):
    """Per env, the least distance in cells from a wheel contact's scaled coordinate to a rounding boundary k + 1/2 of the height lookup,
    over every sub-step, wheel and axis of ``contacts`` [substeps, E, 6, 2] (float64).  Clamped coordinates sit on an integer: 0.5."""
    f64 = np.dtype(np.float64)
    dist = []
    for axis in range(2):
        s = field.scaled(np.asarray(contacts, dtype=np.float64)[..., axis], axis, f64)
        dist.append(np.abs((s - np.floor(s)) - 0.5))
    return np.minimum(dist[0], dist[1]).min(axis=(0, 2))
