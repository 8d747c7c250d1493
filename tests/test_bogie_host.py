"""CPU: the rocker-bogie posture mode of the motion model as DEFINED (tests/bogie_ref.py; include/rover_step.h,
rover_motion_step_bogie) — the constant inverse against the library's host entry, the geometry against the oracle's
restatement of the reference's wheel rays, the convergence of the chord iteration on the field the GPU test uses, the model's limits
(planar, constant, one wheel raised, mirrored), the refusals that need no device and the ``suspension`` switch.  No GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import bogie_ref as B
import motion_ref as R

# the field and the inputs of tests/test_bogie_gpu.py: test_motion_gpu's map and inputs, at a vertical scale of 0.1
N0, N1, HSCALE, VSCALE, SHIFT = 96, 80, 0.05, 0.1, (-1.3, 0.7)
KW = dict(dt=0.05, max_lin=1.3, max_ang=0.9, ride_height=0.3)
E_MAX = 257


def make_inputs(n, seed):
    """tests/test_motion_gpu.py:make_inputs, restated (that module needs torch)."""
    rng = np.random.default_rng(seed)
    lo = np.array([SHIFT[0] - 0.5, SHIFT[1] - 0.5])
    hi = np.array([SHIFT[0] + N0 * HSCALE + 0.5, SHIFT[1] + N1 * HSCALE + 0.5])
    pos = np.concatenate((rng.uniform(lo, hi, (n, 2)), rng.uniform(-1, 1, (n, 1))), 1).astype(np.float32)
    quat = rng.normal(size=(n, 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
    lin, ang = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    return pos, quat, lin, ang


HEIGHTS = np.random.default_rng(7).uniform(0.0, 1.0, (N0, N1)).astype(np.float32)


def test_symbols_declared_and_exported():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for name in ("rover_motion_step_bogie", "rover_motion_bogie_fit"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert [f for f, _ in _lib.BogieParams._fields_] == ["iters", "max_bogie"] and C.sizeof(_lib.BogieParams) == 8


def _exact_inverse(j):
    """inv(j) in rational arithmetic on the doubles of j, by Gauss-Jordan: no rounding at all."""
    n = j.shape[0]
    m = [[Fraction(float(v)) for v in row] + [Fraction(int(r == c)) for c in range(n)] for r, row in enumerate(j)]
    for c in range(n):
        piv = next(r for r in range(c, n) if m[r][c] != 0)
        m[c], m[piv] = m[piv], m[c]
        m[c] = [v / m[c][c] for v in m[c]]
        for r in range(n):
            if r != c and m[r][c] != 0:
                m[r] = [a - m[r][c] * b for a, b in zip(m[r], m[c])]
    return [row[n:] for row in m]


def test_the_inverse_is_the_inverse_of_the_jacobian_at_rest():
    """rover_motion_bogie_fit against numpy.linalg.inv of bogie_ref's analytic Jacobian, rounded to float32: bit for bit — in the 34
    entries whose exact value is not 0.  Entries [1][4] and [1][5] (roll's answer to the rear pair) are exactly 0 by the layout's mirror
    symmetry; numpy.linalg.inv returns rounding noise of some 1e-17 there, whose bits depend on the LAPACK build and the CPU, so no
    library can be held to them.  Instead all 36 entries are held to something stronger: each is the float32 NEAREST to the exact
    rational inverse of J (no double-rounding slack is needed), and the two zeros are +0 exactly.  |D J - I| <= 1e-5: |D| < 2.8 and
    |J| <= 1, so float32 rounding of D moves an entry of D J by at most 6 * 2.8 * 2^-24 = 1e-6."""
    from isaac_rover_amd import _lib
    j = B.jacobian()
    got = _lib.motion_bogie_fit()
    assert got.dtype == np.float32 and got.shape == (6, 6)
    want = np.linalg.inv(j).astype(np.float32)
    exact = _exact_inverse(j)
    zeros = [(r, c) for r in range(6) for c in range(6) if exact[r][c] == 0]
    assert zeros == [(1, 4), (1, 5)]
    for r in range(6):
        for c in range(6):
            g = got[r, c]
            if (r, c) in zeros:
                assert g.view(np.uint32) == 0 and abs(np.linalg.inv(j)[r, c]) < 1e-15, (r, c)
                continue
            assert g.view(np.uint32) == want[r, c].view(np.uint32), (r, c, g, want[r, c])
            err = abs(Fraction(float(g)) - exact[r][c])
            for other in (np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))):
                assert err <= abs(Fraction(float(other)) - exact[r][c]), (r, c)
    assert np.array_equal(got[np.array(exact) != 0], B.chord_inverse()[np.array(exact) != 0])
    assert np.abs(got.astype(np.float64) @ j - np.eye(6)).max() <= 1e-5
    assert 10 < np.linalg.cond(j) < 11
    lib = _lib.load()
    assert lib.rover_motion_bogie_fit(None) == -1 and b"motion_bogie_fit" in lib.rover_last_error(None)


def test_the_jacobian_is_the_derivative_of_the_forward_map():
    """Central differences of F at u = 0 with h = 1e-5: the truncation error is h^2 / 6 times a third derivative below 0.5 m, 1e-11,
    and the rounding error 1e-16 / h = 1e-11: well inside 1e-8.  F is taken with the decimal constants J is derived from; the kernel's
    float32 constants (0.286f + 0.153f is 0.439 + 1.05e-8) move a column by up to 1.05e-8, which the second loop bounds by 2e-8."""
    j, h = B.jacobian(), 1e-5
    for k in range(6):
        up, dn = [np.zeros(1) for _ in range(6)], [np.zeros(1) for _ in range(6)]
        up[k], dn[k] = up[k] + h, dn[k] - h
        fd = (B.forward(up, const=np.float64)[0] - B.forward(dn, const=np.float64)[0]) / (2 * h)
        assert np.abs(fd - j[:, k]).max() <= 1e-8, (k, fd, j[:, k])
        fd32 = (B.forward(up)[0] - B.forward(dn)[0]) / (2 * h)
        assert np.abs(fd32 - j[:, k]).max() <= 2e-8, (k, fd32, j[:, k])
    # the rest position: the layout of the wheel rays, at body z = -0.167
    rest = B.forward([np.zeros(1) for _ in range(6)])[0]
    assert np.abs(rest + B.ORIGIN_Z).max() <= 1e-8            # float32 constants: 0.03f - 0.197f is 0.167 to 1e-9
    pts = B.world_points(np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)))[0]
    assert np.abs(pts[:, :2] - np.array(B.LAYOUT)).max() <= 1e-7


def test_the_geometry_is_the_wheel_rays():
    """bogie_ref's wheel-frame origins in the world against the oracle's restatement of rock_detect.py:160-319, which the step kernels
    are held to: the local ray pattern is symmetric about (0, 0, 0.1) and its direction is local -z, so the origin is the mean of the
    wheel's four ray sources + 0.1 * the wheel's direction.  Random postures, angles and joints up to 0.3 rad, zero steering; 1e-5 m,
    since the oracle works in float32.  This pins the sign and the axis of all three joints."""
    import torch
    from oracle import torch_ref
    rng = np.random.default_rng(21)
    n = 64
    pos = rng.uniform(-3, 3, (n, 3))
    eul = np.concatenate((rng.uniform(-0.3, 0.3, (n, 2)), rng.uniform(-3.1, 3.1, (n, 1))), 1)
    joints = np.zeros((n, 13))
    joints[:, 0:3] = rng.uniform(-0.3, 0.3, (n, 3))
    joints[0, 0:3], joints[1, 0:3], joints[2, 0:3] = (0.3, 0, 0), (0, 0.3, 0), (0, 0, 0.3)       # each joint alone
    src, dirs = torch_ref._wheel_rays(*(torch.from_numpy(a.astype(np.float32)) for a in (pos, eul, joints)))
    src, dirs = src.numpy().astype(np.float64).reshape(n, 6, 4, 3), dirs.numpy().astype(np.float64).reshape(n, 6, 4, 3)
    want = src.mean(2) + 0.1 * dirs[:, :, 0]
    got = B.world_points(pos.astype(np.float32), eul.astype(np.float32), joints[:, 0:3].astype(np.float32))
    assert np.abs(got - want).max() <= 1e-5
    # and the check can tell: a joint's sign, or j0 and j1 swapped, is centimetres off
    for wrong in (joints[:, 0:3] * [-1, 1, 1], joints[:, 0:3] * [1, 1, -1], joints[:, [1, 0, 2]]):
        assert np.abs(B.world_points(pos.astype(np.float32), eul.astype(np.float32), wrong.astype(np.float32)) - want).max() > 1e-2
    # F is the z of these points
    u = [pos[:, 2], eul[:, 0], eul[:, 1], joints[:, 0], joints[:, 1], joints[:, 2]]
    assert np.abs(B.forward(u) - B.world_points(pos, eul, joints[:, 0:3])[:, :, 2]).max() <= 1e-12


@pytest.mark.parametrize("rcp", [0, 1])
def test_convergence_on_the_gpu_tests_field(rcp):
    """iters = 4 leaves at most 1e-6 m of residual on every one of the 257 envs of the GPU test (measured: 2.7e-7 m, the largest angle
    0.30 rad), and the worst residual falls with every iteration from 1 to 4."""
    field = R.Field(HEIGHTS, HSCALE, VSCALE, SHIFT, rcp)
    out = B.step(field, *make_inputs(E_MAX, 0), iters=4, **KW)
    worst = out["residuals"].max(1)
    print("worst residual after 1 .. 4 iterations:", worst, "largest angle:", max(np.abs(out["joints_raw"]).max(), np.abs(out["roll"]).max(), np.abs(out["pitch"]).max()))
    assert out["residual"].shape == (E_MAX,) and out["residual"].max() <= 1e-6
    assert np.all(np.diff(worst) < 0)
    assert np.all(np.diff(out["residuals"], axis=0) <= 0)                # and per env
    for it in (1, 2, 3):
        assert np.array_equal(B.step(field, *make_inputs(E_MAX, 0), iters=it, **KW)["residual"], out["residuals"][it - 1])
    assert 0.25 < np.abs(out["joints_raw"]).max() < 0.35                  # the field does bend the bogies
    # the share of envs the clamp test of the GPU file counts on
    over = (np.abs(out["joints_raw"]) > 0.25).any(1)
    assert 0 < over.sum() < E_MAX // 4


class PlaneField:
    """z = h + p (x cos g + y sin g) + q (-x sin g + y cos g): a plane with slopes (p, q) along the directions of heading g."""

    def __init__(self, h, p, q, g):
        self.h, self.p, self.q, self.g = h, p, q, g

    def height(self, x, y, dtype):
        c, s = np.cos(self.g), np.sin(self.g)
        return (self.h + self.p * (x * c + y * s) + self.q * (-x * s + y * c)).astype(dtype)


def test_a_planar_field_bends_no_joint():
    """On a plane with slopes p (forward) and q (left), up to 0.3 each, u = (z_c, roll, pitch, 0, 0, 0) with -sin(pitch) = p and
    cos(pitch) sin(roll) = q meets the six targets exactly: the joints of the model's solution are 0.  1e-9 is below what 4 chord
    iterations leave at these angles, so the property is checked on the converged iteration, iters = 8, and on the model with its
    decimal constants: the kernel's float32 constants put the centre wheels' contacts at 0.007f where their frame origin is at
    0.153f - 0.146f, 9.3e-10 m apart, which on a slope of 0.3 is a height mismatch of 2.8e-10 m over a lever of 0.146 m: joints of
    up to 2e-9.  With those constants, and after 4 iterations, the joints are asserted below 1e-8.
    The body then lies in the plane in this sense: the rotation's third row is (p, q, .), so the body's x and y axes rise by p and q
    per metre of body coordinate.  Its z axis is normal to the plane z = p a + q b over the BODY's horizontal coordinates (a, b).  The
    contacts are sampled at yaw only, so against the plane over WORLD coordinates the pitch has sin(pitch) = -p where the true normal
    has tan(pitch) = -p: the two differ by pitch^3 / 2 (0.014 rad at 0.3), and likewise for roll.  That difference is the model's, not
    the solver's; the angle to the world normal is third order in the slope s = hypot(p, q), asserted below s^3 (the
    leading term is s^3 / 2 for a pure pitch; 0.042 rad at p = q = 0.3)."""
    rng = np.random.default_rng(5)
    n = 100
    p, q, g = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-3, 3, n)
    p[:4], q[:4] = (0.3, -0.3, 0.3, 0.0), (0.3, 0.3, 0.0, -0.3)
    quat = np.stack((np.cos(g / 2), np.zeros(n), np.zeros(n), np.sin(g / 2)), 1).astype(np.float32)
    g = R.yaw_of(quat.astype(np.float64))                                       # the heading the model reads
    pos = np.concatenate((rng.uniform(-2, 2, (n, 2)), np.zeros((n, 1))), 1).astype(np.float32)
    zero = np.zeros(n, dtype=np.float32)
    field = PlaneField(0.4, p, q, g)
    for iters in (4, 8):
        out32c = B.step(field, pos, quat, zero, zero, dt=0.05, iters=iters)
        print(f"planar field, float32 constants, largest joint after {iters} iterations:", np.abs(out32c["joints"]).max())
        assert np.abs(out32c["joints"]).max() <= 1e-8
    out = B.step(field, pos, quat, zero, zero, dt=0.05, iters=8, const=np.float64)
    assert np.abs(out["joints"]).max() <= 1e-9
    # the pose converges more slowly than the joints at the steepest corner: 8 iterations leave a residual below 1e-8 m, and an error
    # of the unknowns of at most 6 max|D| = 17 times that
    assert out["residual"].max() <= 1e-8
    tol = 17e-8
    sr, cr, sp, cp = np.sin(out["roll"]), np.cos(out["roll"]), np.sin(out["pitch"]), np.cos(out["pitch"])
    assert np.abs(-sp - p).max() <= tol and np.abs(cp * sr - q).max() <= tol             # the third row's first two entries
    # the body's z axis in the heading frame (the rotation's third column) against the world plane's normal
    zb = np.stack((sp * cr, -sr, cp * cr), 1)
    normal = np.stack((-p, -q, np.ones(n)), 1)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    angle = np.arccos(np.clip((zb * normal).sum(1), -1, 1))
    bound = (p * p + q * q) ** 1.5 + tol
    assert np.all(angle <= bound), (angle.max(), bound.max())
    assert angle.max() > 1e-3                                                   # and the difference is real
    # z_c: the wheel origins, rest_z() below the centre along the third row's last entry, sit on plane + ride_height - 0.167
    want_z = 0.4 + p * (pos[:, 0] * np.cos(g) + pos[:, 1] * np.sin(g)) + q * (-pos[:, 0] * np.sin(g) + pos[:, 1] * np.cos(g))
    want_z = want_z + (np.float64(np.float32(0.3)) - B.ORIGIN_Z) - (cp * cr) * rest_z()
    assert np.abs(out["pos"][:, 2] - want_z).max() <= tol


def rest_z():
    """The wheel origins' body z with all joints at 0, from the model's decimal constants."""
    return float(B.body_points([np.zeros(1)] * 3, np.float64, np.float64)[0][2][0])


def test_constant_heightfield_reproduces_the_flat_unicycle():
    """As test_motion_host's test for the plane mode: on a constant heightfield the model is KinematicSim.step — z = h + ride_height
    (the origins' rest z is -0.167 to 1e-9), a pure-yaw quaternion, joints 0 — here within 1e-6 in float64 AND in float32."""
    rng = np.random.default_rng(3)
    n, h, ride, dt = 200, 0.37, 0.3, 0.05
    field = R.Field(np.full((40, 56), h, dtype=np.float32), 0.05, 1.0, (-0.2, 0.1))
    yaw0 = rng.uniform(-3.0, 3.0, n)
    quat = np.stack((np.cos(yaw0 / 2), np.zeros(n), np.zeros(n), np.sin(yaw0 / 2)), 1).astype(np.float32)
    pos = np.concatenate((rng.uniform(-1, 3, (n, 2)), rng.uniform(-1, 1, (n, 1))), 1).astype(np.float32)
    ang = rng.uniform(-1, 1, n).astype(np.float32)
    lin = (np.abs(ang) * rng.uniform(0.5, 1.0, n) * rng.choice((-1.0, 1.0), n)).astype(np.float32)      # |v / w| >= 0.5
    q64 = quat.astype(np.float64)
    yaw = 2.0 * np.arctan2(q64[:, 3], q64[:, 0]) + ang.astype(np.float64) * np.float64(np.float32(dt))       # vec_env.KinematicSim.step
    step = lin.astype(np.float64) * np.float64(np.float32(dt))
    want_pos = np.stack((pos[:, 0] + step * np.cos(yaw), pos[:, 1] + step * np.sin(yaw), np.full(n, np.float64(np.float32(h)) + np.float32(ride))), 1)
    want_quat = np.stack((np.cos(yaw / 2), np.zeros(n), np.zeros(n), np.sin(yaw / 2)), 1)
    for dtype in (np.float64, np.float32):
        out = B.step(field, pos, quat, lin, ang, dt=dt, ride_height=ride, dtype=dtype)
        assert out["pos"].dtype == dtype
        assert np.abs(out["pos"] - want_pos).max() <= 1e-6
        sign = np.sign((out["quat"] * want_quat).sum(1))[:, None]
        assert np.abs(out["quat"] * sign - want_quat).max() <= 1e-6
        assert np.abs(out["roll"]).max() <= 1e-6 and np.abs(out["pitch"]).max() <= 1e-6 and np.abs(out["joints"]).max() <= 1e-6


def _raised(under, lift=0.05):
    """A 4 x 4 m field at 0 with the nodes within 0.1 m of wheel ``under``'s contact raised by ``lift``, a rover at its centre with yaw 0
    and no command -> the model's answer after one sub-step (float64, 8 iterations: converged)."""
    hm = np.zeros((81, 81), dtype=np.float32)
    cx, cy = 2.0 + B.LAYOUT[under][0], 2.0 + B.LAYOUT[under][1]
    ix, iy = int(round(cx / 0.05)), int(round(cy / 0.05))
    hm[ix - 2:ix + 3, iy - 2:iy + 3] = lift
    field = R.Field(hm, 0.05, 1.0, (0.0, 0.0))
    one = lambda *v: np.float32([v])
    return B.step(field, one(2.0, 2.0, 0.0), one(1, 0, 0, 0), np.float32([0]), np.float32([0]), dt=0.05, iters=8)


def test_one_raised_wheel_bends_its_bogie_and_the_mirror_image_mirrors():
    """The ground raised by 0.05 m under FL alone: j0 = -0.1056 (the front-left bogie tips its front wheel up), the other two joints an
    order of magnitude smaller.  Raised under FR instead, the answer is the mirror image: (z_c, -roll, pitch, -j1, -j0, -j2).  Under RL:
    j2 = +0.0650."""
    fl, fr, rl = _raised(0), _raised(1), _raised(4)
    assert fl["residual"].max() <= 1e-12 and rl["residual"].max() <= 1e-12
    j = fl["joints"][0]
    assert j[0] < 0 and abs(j[0] + 0.1056) <= 1e-4
    assert abs(j[1]) < 0.2 * abs(j[0]) and abs(j[2]) < 0.2 * abs(j[0])
    assert fl["roll"][0] > 0 and fl["pitch"][0] < 0                  # left side up, nose up
    m = fr["joints"][0]
    assert np.abs(np.array([-m[1], -m[0], -m[2]]) - j).max() <= 1e-12
    assert abs(fr["roll"][0] + fl["roll"][0]) <= 1e-12 and abs(fr["pitch"][0] - fl["pitch"][0]) <= 1e-12
    assert abs(fr["pos"][0, 2] - fl["pos"][0, 2]) <= 1e-12
    assert abs(rl["joints"][0, 2] - 0.0650) <= 1e-4 and rl["joints"][0, 2] > 0
    # the clamp acts on the joints alone
    hm_out = B.step(R.Field(np.zeros((8, 8), dtype=np.float32), 0.05, 1.0, (0.0, 0.0)), np.zeros((1, 3), dtype=np.float32),
                    np.float32([[1, 0, 0, 0]]), np.float32([0]), np.float32([0]), dt=0.05, max_bogie=0.05)
    assert np.array_equal(hm_out["joints"], hm_out["joints_raw"])
    lim = np.float64(np.float32(0.05))
    assert np.array_equal(np.clip(fl["joints_raw"], -lim, lim)[0], [-lim, fl["joints_raw"][0, 1], fl["joints_raw"][0, 2]])


def test_substeps_are_repeated_steps_in_the_restatement():
    field = R.Field(HEIGHTS, HSCALE, VSCALE, SHIFT, 0)
    pos, quat, lin, ang = make_inputs(40, 0)
    for dtype in (np.float32, np.float64):
        p, q = pos, quat
        for _ in range(3):
            one = B.step(field, p, q, lin, ang, dtype=dtype, **KW)
            p, q = one["pos"].astype(np.float32), one["quat"].astype(np.float32)
        if dtype is np.float32:                                      # the float32 pose survives the hand-over between calls exactly
            three = B.step(field, pos, quat, lin, ang, substeps=3, dtype=dtype, **KW)
            assert np.array_equal(three["pos"], one["pos"]) and np.array_equal(three["quat"], one["quat"])
            assert np.array_equal(three["joints"], one["joints"])


def test_descriptor_and_parameter_refusals_need_no_device():
    """Every ROVER_E_INVALID of rover_motion_step_bogie is decided before the ctx is looked at: rover_motion_step's own, and the new
    ones — NULL parameters, iters outside 1 .. 8, max_bogie not finite or not > 0 —, each reported by name with a NULL ctx."""
    from isaac_rover_amd import _lib
    lib = _lib.load()
    D, P = _lib.motion_desc, _lib.BogieParams

    def call(d, p):
        rc = lib.rover_motion_step_bogie(None, None if d is None else C.byref(d), None if p is None else C.byref(p), None)
        return rc, lib.rover_last_error(None).decode()

    ok = P(4, 0.6)
    bad = [("null descriptor", None, ok, "null descriptor"), ("E < 0", D(-1), ok, "negative"), ("substeps 0", D(4, substeps=0), ok, "substeps"),
           ("cmd_stride 0", D(4, cmd_stride=0), ok, "cmd_stride"), ("dt 0", D(4, dt=0.0), ok, "dt"), ("dt < 0", D(4, dt=-0.05), ok, "dt"),
           ("dt nan", D(4, dt=float("nan")), ok, "dt"), ("dt inf", D(4, dt=float("inf")), ok, "dt"),
           ("no pos", D(4, pos3=None), ok, "pos3"), ("no quat", D(4, quat4=None), ok, "quat4"), ("no lin", D(4, lin=None), ok, "lin"),
           ("no ang", D(4, ang=None), ok, "ang")]
    names = ("joint_pos_targets13", "joint_vel_targets13", "joint_pos13", "joint_vel13")
    for mask in range(1, 15):
        bad.append((f"joints {mask:04b}", D(4, **{n: 16 for i, n in enumerate(names) if mask >> i & 1}), ok, "go together"))
    bad += [("null params", D(4), None, "null parameters"), ("iters 0", D(4), P(0, 0.6), "iters"), ("iters -1", D(4), P(-1, 0.6), "iters"),
            ("iters 9", D(4), P(9, 0.6), "iters"), ("max_bogie 0", D(4), P(4, 0.0), "max_bogie"), ("max_bogie < 0", D(4), P(4, -0.6), "max_bogie"),
            ("max_bogie nan", D(4), P(4, float("nan")), "max_bogie"), ("max_bogie inf", D(4), P(4, float("inf")), "max_bogie"),
            ("E 0, iters 0", D(0), P(0, 0.6), "iters")]
    for what, d, p, word in bad:
        rc, msg = call(d, p)
        assert rc == -1 and msg.startswith("motion_step_bogie:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    for d, p in ((D(4), ok), (D(0), ok), (D(4), P(1, 1e-3)), (D(4), P(8, 3.0)), (D(4, **{n: 16 for n in names}), ok)):
        assert call(d, p) == (-1, "motion_step_bogie: null ctx")


def test_the_suspension_switch():
    from isaac_rover_amd import _lib, vec_env

    class Task:
        num_envs, observation_space, action_space = 3, None, None

        def set_up_scene(self, spawn_positions=None):
            pass

        def post_reset(self):
            pass

    assert set(vec_env.SIMS) == {"kinematic", "terrain"}
    assert vec_env.SUSPENSIONS == ("plane", "bogie") == _lib.SUSPENSIONS
    with pytest.raises(ValueError, match="needs sim='terrain'"):
        vec_env.VecEnv(sim="kinematic", suspension="bogie")
    with pytest.raises(ValueError, match="needs sim='terrain'"):
        vec_env.VecEnv(suspension="bogie")
    with pytest.raises(TypeError):
        vec_env.KinematicSim(Task(), suspension="bogie")
    for bad in ("rigid", "", None, "Bogie"):
        with pytest.raises(ValueError, match="suspension must be one of"):
            vec_env.VecEnv(sim="terrain", suspension=bad)
        with pytest.raises(ValueError, match="suspension must be one of"):
            vec_env.TerrainSim(Task(), suspension=bad)
    for kw, cls, mode in (({}, vec_env.KinematicSim, None), ({"sim": "kinematic", "suspension": "plane"}, vec_env.KinematicSim, None),
                          ({"sim": "terrain"}, vec_env.TerrainSim, "plane"), ({"sim": "terrain", "suspension": "plane"}, vec_env.TerrainSim, "plane"),
                          ({"sim": "terrain", "suspension": "bogie"}, vec_env.TerrainSim, "bogie")):
        env = vec_env.VecEnv(headless=True, **kw)
        env.set_task(Task(), sim_params={"dt": 0.02})
        assert type(env._world) is cls and env._world.dt == 0.02
        assert getattr(env._world, "suspension", None) == mode
    w = vec_env.TerrainSim(Task(), suspension="bogie", iters=6, max_bogie=0.4)
    assert (w.suspension, w.iters, w.max_bogie) == ("bogie", 6, 0.4)
    w = vec_env.TerrainSim(Task())
    assert (w.suspension, w.iters, w.max_bogie) == ("plane", 4, 0.6)
