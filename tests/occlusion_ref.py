"""Independent restatement of the line-of-sight occlusion (include/rover_step.h, rover_obs_occlusion; csrc/rover_occlusion.hip) in numpy
float32: every operation of the definition is one float32 numpy operation, in the written order, so the result is the definition's bit
for bit (numpy's float32 +, -, *, /, sqrt, ceil and rint are IEEE, one rounding each).  Vectorised over rows and columns, a loop over k.
No torch, no library."""
import numpy as np

F32 = np.float32
DEFAULT = dict(camera=(0.0, 0.0, 0.7), step=0.05, clearance=0.03, max_steps=256, miss=5.0)


class Field:
    """A heightfield as rover_set_heightfield takes it: hm [N0, N1] float32, node spacing, vertical scale, shift; rcp = cell_index_mode."""

    def __init__(self, hm, hscale=0.025, vscale=1.0, shift=(0.0, 0.0), rcp=0):
        self.hm = np.ascontiguousarray(hm, dtype=F32)
        self.hscale, self.vscale, self.shift, self.rcp = F32(hscale), F32(vscale), (F32(shift[0]), F32(shift[1])), int(rcp)

    def coord(self, v, axis):
        """cell_coord of rover_height.h: the clamp bound is the dim-0 size for both axes, round half to even, a NaN goes to node 0."""
        with np.errstate(invalid="ignore"):
            s = (v - self.shift[axis]) * (F32(1.0) / self.hscale) if self.rcp else (v - self.shift[axis]) / self.hscale
            hi = F32(self.hm.shape[0] - 1)
            s = np.where(s < 0, F32(0.0), s)
            s = np.where(s > hi, hi, s)
            s = np.rint(s)
            return np.where(s == s, s, F32(0.0)).astype(np.int64)

    def nodes(self, x, y):
        return self.coord(x, 0), np.minimum(self.coord(y, 1), self.hm.shape[1] - 1)

    def height(self, x, y):
        ix, iy = self.nodes(x, y)
        return self.hm[ix, iy] * self.vscale


def body_points(points, sparse_idx, dense_idx):
    """[C, 3] float32: points[j] of the columns in obs order, each f64 coordinate rounded to f32 once."""
    idx = np.concatenate([np.asarray(sparse_idx, dtype=np.int64).reshape(-1), np.asarray(dense_idx, dtype=np.int64).reshape(-1)])
    return np.asarray(points, dtype=np.float64)[idx].astype(F32)


def order(points, sparse_idx, dense_idx, camera=DEFAULT["camera"]):
    """rover_occlusion_order restated: far first by (bx - cx)^2 + (by - cy)^2 in f64 on the f32-rounded values, stable."""
    b = body_points(points, sparse_idx, dense_idx).astype(np.float64)
    cam = np.asarray(camera, dtype=F32).astype(np.float64)
    key = (b[:, 0] - cam[0]) ** 2 + (b[:, 1] - cam[1]) ** 2
    return np.argsort(-key, kind="stable").astype(np.int32)


def rotation(quat):
    """r[i][j] arrays [M] from quat [M, 4] = (w, x, y, z), not normalised."""
    w, x, y, z = (quat[:, i] for i in range(4))
    one, two = F32(1.0), F32(2.0)
    return [[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
            [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
            [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]


def occlude(field, body3, pos, quat, clean, in_=None, first=0, drop_value=0.0, camera=DEFAULT["camera"], step=DEFAULT["step"],
            clearance=DEFAULT["clearance"], max_steps=DEFAULT["max_steps"], miss=DEFAULT["miss"]):
    """-> dict: out [M, F], hidden [M, C] uint8, target [M, C, 3] (NaN where the miss test said visible: the library leaves those
    unwritten), has_point [M, C] bool, n [M, C] int64 (0 without a point), margin [M, C] (the smallest (Cam_z + t dz) + clearance - h over
    ALL the column's samples, +inf without one, NaN samples skipped)."""
    clean = np.asarray(clean, dtype=F32)
    in_ = clean if in_ is None else np.asarray(in_, dtype=F32)
    pos, quat, body3 = np.asarray(pos, dtype=F32), np.asarray(quat, dtype=F32), np.asarray(body3, dtype=F32)
    M, F = clean.shape
    C = F - first
    assert body3.shape == (C, 3) and pos.shape == (M, 3) and quat.shape == (M, 4)
    cam_b = np.asarray(camera, dtype=F32)
    step, clearance, miss = F32(step), F32(clearance), F32(miss)
    with np.errstate(all="ignore"):
        r = rotation(quat)
        rot = lambda i, v0, v1, v2: (r[i][0][:, None] * v0 + r[i][1][:, None] * v1) + r[i][2][:, None] * v2
        cam = [pos[:, i:i + 1] + rot(i, cam_b[0], cam_b[1], cam_b[2]) for i in range(3)]                 # [M, 1]
        S = [pos[:, i:i + 1] + rot(i, body3[None, :, 0], body3[None, :, 1], body3[None, :, 2]) for i in range(3)]     # [M, C]
        D = [-r[i][2][:, None] for i in range(3)]
        v = clean[:, first:]
        has = np.abs(v) < miss
        d = F32(2.0) * v
        T = [S[i] + d * D[i] for i in range(3)]
        dx, dy, dz = (T[i] - cam[i] for i in range(3))
        L = np.sqrt(dx * dx + dy * dy)
        u = np.ceil(L / step)
        small = u < F32(max_steps)
        n = np.where(small, np.where(small, u, F32(0.0)).astype(np.int64), max_steps)
        n = np.where(has, n, 0)
        hidden = np.zeros((M, C), dtype=bool)
        margin = np.full((M, C), np.inf, dtype=F32)
        camx, camy, camz = (np.broadcast_to(cam[i], (M, C)) for i in range(3))
        for k in range(1, int(n.max(initial=0))):
            live = np.nonzero(k < n)
            if live[0].size == 0:
                break
            t = F32(k) / n[live].astype(F32)
            line = (camz[live] + t * dz[live]) + clearance
            h = field.height(camx[live] + t * dx[live], camy[live] + t * dy[live])
            hidden[live] |= h > line
            margin[live] = np.fmin(margin[live], line - h)
    out = in_.copy()
    out[:, first:] = np.where(hidden, F32(drop_value), in_[:, first:])
    target = np.stack(T, axis=-1)
    target[~has] = np.nan
    return dict(out=out, hidden=hidden.astype(np.uint8), target=target, has_point=has, n=n, margin=margin)


def lane_slot_ratio(n, order_=None, wave=64):
    """Lane-slots a wave spends per useful sample when the columns of a row are taken ``wave`` at a time in ``order_`` (None: obs order):
    a wave marches as long as its longest lane.  n [M, C] from occlude(); a column has max(n - 1, 0) samples."""
    s = np.maximum(np.asarray(n) - 1, 0)
    if order_ is not None:
        s = s[:, np.asarray(order_)]
    M, C = s.shape
    pad = (-C) % wave
    sp = np.pad(s, ((0, 0), (0, pad))).reshape(M, -1, wave)
    return float(wave * sp.max(axis=2).sum()) / float(s.sum())


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- seeded cases shared by tests/test_occlusion_host.py and tests/test_occlusion_gpu.py ---------------------------------------------
def make_field(seed=0, nodes=400, hscale=0.025, hills=5, rocks=150):
    """A [nodes, nodes] field at ``hscale`` m: a few Gaussian hills plus ``rocks`` steep bumps (0.1 - 0.45 m high, 0.08 - 0.3 m wide)."""
    rng = np.random.default_rng(seed)
    ext = nodes * hscale
    x = (np.arange(nodes) * hscale)[:, None]
    y = (np.arange(nodes) * hscale)[None, :]
    hm = np.zeros((nodes, nodes))
    for _ in range(hills):
        cx, cy, s, a = rng.uniform(0, ext), rng.uniform(0, ext), rng.uniform(1.0, 2.5), rng.uniform(-0.4, 0.6)
        hm += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    for _ in range(rocks):
        cx, cy, s, a = rng.uniform(0, ext), rng.uniform(0, ext), rng.uniform(0.08, 0.3), rng.uniform(0.1, 0.45)
        hm += a * np.clip(1.0 - ((x - cx) ** 2 + (y - cy) ** 2) / (s * s), 0.0, None) ** 0.5
    return Field(hm.astype(F32), hscale)


def quat_of_euler(roll, pitch, yaw):
    """(w, x, y, z) float32 of the ZYX rotation (synth.quat_from_euler in numpy float64, rounded once)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack((cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy), axis=1).astype(F32)


def make_case(field, body3, envs, seed=0, tilt=0.3, first=4, margin=2.5, ride=0.35, sentinel=0.02):
    """Random poses on ``field`` (position ``margin`` m inside the map, yaw anywhere, roll and pitch up to ``tilt`` rad, the body ``ride`` m
    above the ground) and a plausible clean observation: column c holds half the height of its ray origin S above the field, so that
    the targets lie near the surface; a share ``sentinel`` of the columns holds the clipped miss value 5.0 instead, and every 97th of
    those a NaN.  -> dict(pos, quat, clean [envs, first + C])."""
    rng = np.random.default_rng(1000 + seed)
    ext = field.hm.shape[0] * float(field.hscale)
    pos = np.empty((envs, 3), dtype=F32)
    pos[:, :2] = rng.uniform(margin, ext - margin, (envs, 2))
    pos[:, 2] = field.height(pos[:, 0], pos[:, 1]) + F32(ride)
    quat = quat_of_euler(rng.uniform(-tilt, tilt, envs), rng.uniform(-tilt, tilt, envs), rng.uniform(-np.pi, np.pi, envs))
    r = rotation(quat)
    S = [pos[:, i:i + 1] + ((r[i][0][:, None] * body3[None, :, 0] + r[i][1][:, None] * body3[None, :, 1]) + r[i][2][:, None] * body3[None, :, 2])
         for i in range(3)]
    clean = np.empty((envs, first + body3.shape[0]), dtype=F32)
    clean[:, :first] = rng.standard_normal((envs, first))
    clean[:, first:] = (S[2] - field.height(S[0], S[1])) * F32(0.5)
    miss = np.nonzero(rng.random((envs, body3.shape[0])) < sentinel)
    clean[miss[0], first + miss[1]] = np.where(np.arange(miss[0].size) % 97 == 96, F32(np.nan), F32(5.0))
    return dict(pos=pos, quat=quat, clean=clean)
