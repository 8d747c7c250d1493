"""Property test (CPU, numpy) of the staged ray cast's REBASED level bound — `lane_scan_kernel` with bit 4 of `forms` ("lane_rebase") in
csrc/rover_cull.hip, DESIGN.md §5.3.

The level loop measures a steep ray against a suffix bound {G, z0, z1, rho_out} of its row.  With the option on it does so from
s' = s - (s_z / d_z) d, the point where the ray's LINE crosses the row's own height z_c (all coordinates relative to the row's centre C):

    |dz| G - c3 rho_out - (|dz| 1.0004 + c3) o' - kz |s_z|  >  dzm' (|dxy| + k2 |dz|^2) 1.0004
    o' = dist_xy(s', C),  dzm' = max(|z0|, |z1|),  c3 = k2 |dz| |dxy| 1.0004,  kz = k2 1.0004 1.0021 + LN_REB_ERR

W, the distance from a sphere's centre to the line, may be bounded from any point of the line — that is what removes the drift
|s_z - z| tan(beta) from the offset.  The AXIAL part of h = s - m, which test (A) charges with k2, belongs to the true origin: it is the
axial part about s' plus |s_z| |d| / |d_z|, the term kz |s_z|.  The claim checked here, as tests/test_level_bound_property.py checks it for
the origin form: whenever this restatement (float32, the kernel's operation order, fp16 level records rounded as the builder rounds them)
clears a suffix, EVERY record of the suffix passes test (A) about the TRUE origin in float64 — `c_a |h|^2 - (h.d)^2 > r2` with the f32
test's rounding allowance (§5.4), and with it §5.1's premise W >= rho + alpha (|h| + 2 rho).  No case is skipped: a cleared suffix with one
failing record fails the test.  The sets are moved towards the ray until the bound JUST clears, and sampled at random distances too.

Rays: cos(beta) on both sides of 0.9, origins 0 to 4 m above and below z_c, the line's ground point on C (o' = 0), inside the row and at
the tame limit (1e4 m), d_z of either sign, |d|^2 off 1 by the 1e-5 that §5.4 allows, suffixes whose z range straddles z_c or lies on one
side of it.

`v_rcp_f32` is good to 1 ulp where numpy's division rounds correctly, `v_fma_mix_f32` / `v_fma_f32` round once (`_fma32`): the difference
is what LN_REB_ERR |s_z| pays for four times over (`static_assert` in rover_cull.hip).
"""
import math

import numpy as np

from test_level_bound_property import ALPHA, C_RHO, _clears, _far_consts, _fma32, _level_record, _records, _test_a_margin

f32 = np.float32
LN_REB_ERR = f32(1.0e-6)                                 # rover_cull.hip
KZ_D = f32(1.0004) * f32(1.0021)                         # 1.0004f * 1.0021f, folded by the compiler in float


def _consts(d, k2):
    dx, dy, dz = (f32(x) for x in d)
    dxy2 = dx * dx + dy * dy
    adz = abs(dz)
    sq = np.sqrt(dxy2, dtype=f32)
    steep = bool(adz * adz >= f32(0.81) * (dxy2 + adz * adz) * f32(1.0001))
    c3 = k2 * adz * sq * f32(1.0004)
    c4 = (sq + k2 * adz * adz) * f32(1.0004)
    return dx, dy, dz, adz, sq, steep, c3, c4


def _s_prime(s, d):
    """(s'x, s'y) as the kernel computes them."""
    sx, sy, sz = (f32(x) for x in s)
    dx, dy, dz = (f32(x) for x in d)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tz = sz * (f32(1.0) / dz)
        return _fma32(-tz, dx, sx), _fma32(-tz, dy, sy)


def _rebased_form(level, s, d, k2):
    """lane_scan_kernel's level test with forms bit 4 set -> (steep, lhs - rhs)."""
    Gq, z0, z1, ro = (f32(x) for x in level)
    sz = f32(s[2])
    dx, dy, dz, adz, sq, steep, c3, c4 = _consts(d, k2)
    lx, ly = _s_prime(s, d)
    with np.errstate(invalid="ignore", over="ignore"):
        o = np.sqrt(lx * lx + ly * ly, dtype=f32)
        kz = k2 * KZ_D + LN_REB_ERR
        base = -((adz * f32(1.0004) + c3) * o + kz * abs(sz))
        dzm = max(abs(f32(0.0) - z0), abs(f32(0.0) - z1))
        lhs = _fma32(Gq, adz, _fma32(ro, -c3, base))
        return steep, f32(lhs - dzm * c4)


def _origin_form(level, s, d, k2):
    """... with the bit clear (the form tests/test_level_bound_property.py restates as `_clears`) -> (steep, lhs - rhs)."""
    Gq, z0, z1, ro = (f32(x) for x in level)
    sx, sy, sz = (f32(x) for x in s)
    dx, dy, dz, adz, sq, steep, c3, c4 = _consts(d, k2)
    o = np.sqrt(sx * sx + sy * sy, dtype=f32)
    base = -((adz * f32(1.0004) + c3) * o + f32(0.0) * abs(sz))
    dzm = max(abs(sz - z0), abs(sz - z1))
    lhs = _fma32(Gq, adz, _fma32(ro, -c3, base))
    return steep, f32(lhs - dzm * c4)


def _clears_rebased(level, s, d, k2):
    steep, slack = _rebased_form(level, s, d, k2)
    return steep and bool(slack > 0.0)


def _direction(rng, tilt):
    az = rng.uniform(0.0, 2.0 * math.pi)
    unit = np.array([math.sin(tilt) * math.cos(az), math.sin(tilt) * math.sin(az), -math.cos(tilt)]) * rng.choice([1.0, -1.0])
    dd = float(rng.choice([1.0 - 1.0e-5, 1.0, 1.0 + 1.0e-5, rng.uniform(1.0 - 1.0e-5, 1.0 + 1.0e-5)]))      # |d|^2
    return (unit * math.sqrt(dd)).astype(f32)


def _ray(rng, steep=True, ground=None):
    """A ray whose line crosses the height z_c at the chosen ground point, from an origin 0 ... 4 m above or below z_c."""
    tilt = float(rng.choice([rng.uniform(0.0, 0.44), rng.uniform(0.40, 0.4505), 0.0])) if steep else float(rng.uniform(0.4525, 1.2))
    d = _direction(rng, tilt)
    hgt = float(rng.choice([0.0, rng.uniform(-4.0, 4.0), 4.0, -4.0, rng.uniform(-0.3, 0.3), rng.uniform(0.3, 1.2)]))
    if ground is None:
        ground = rng.choice(["centre", "row", "row", "row"])
    if ground == "centre":
        p = np.zeros(2)
    elif ground == "row":                                   # inside a shared row's reach: o' <= 0.112 m and a little beyond
        r, a = rng.uniform(0.0, 0.13), rng.uniform(0.0, 2.0 * math.pi)
        p = np.array([r * math.cos(a), r * math.sin(a)])
    else:                                                    # the tame limit: |s_x|, |s_y| < 1e4 m
        a = rng.uniform(0.0, 2.0 * math.pi)
        p = 9.0e3 * np.array([math.cos(a), math.sin(a)])
    d64 = d.astype(np.float64)
    s = np.array([p[0], p[1], 0.0]) + (hgt / d64[2]) * d64
    return s.astype(f32), d


def _set(rng):
    m = int(rng.integers(1, 40))
    ang = rng.uniform(0.0, 2.0 * math.pi, m)
    spread = rng.uniform(0.0, 1.5, m) * rng.uniform(0.0, 1.0)
    hz = rng.uniform(-0.6, 0.6, m) * rng.uniform(0.05, 1.0) + float(rng.choice([0.0, 0.0, 0.35, -0.35]))     # straddles z_c, or lies on one side
    r = rng.uniform(0.01, 0.25, m)
    return ang, spread, hz, r


def _check_cleared(rec, s, d, label):
    """Every record of a cleared suffix: test (A) about the true origin with the f32 test's allowance, and the proof's premise on W."""
    s64, d64 = s.astype(np.float64), d.astype(np.float64)
    margin = _test_a_margin(*rec, s64, d64)
    assert (margin > 0.0).all(), f"{label}: cleared, but a record fails test (A): {margin.min()} (s {s.tolist()}, d {d.tolist()})"
    hx, hy, hz, r2h = rec
    h = np.stack([s64[0] - hx.astype(np.float64), s64[1] - hy.astype(np.float64), s64[2] - hz.astype(np.float64)], axis=1)
    dhat = d64 / np.linalg.norm(d64)
    W = np.linalg.norm(h - (h @ dhat)[:, None] * dhat[None, :], axis=1)
    rho = np.sqrt(r2h.astype(np.float64) / C_RHO)
    need = rho + ALPHA * (np.linalg.norm(h, axis=1) + 2.0 * rho)
    assert (W >= need).all(), f"{label}: cleared, but W - need = {(W - need).min()}"
    return float(margin.min())


def test_a_suffix_cleared_from_the_lines_ground_point_passes_test_a_record_by_record():
    rng = np.random.default_rng(20261020)
    k1, k2 = _far_consts()
    tight = sampled = 0
    worst = math.inf
    seen = dict(up=0, down=0, above=0, below=0, high=0, straddle=0, one_side=0, centre=0)
    for it in range(1300):
        ang, spread, hz, r = _set(rng)
        s, d = _ray(rng, ground="centre" if it % 5 == 0 else None)
        # at random distances: whatever is cleared is checked
        for _ in range(3):
            rec = _records(float(rng.uniform(0.0, 3.9 - float(spread.max()))), ang, spread, hz, r)
            if rec is not None and _clears_rebased(_level_record(*rec, k1), s, d, k2):
                _check_cleared(rec, s, d, "random distance")
                sampled += 1
        # at the bound's edge: the smallest distance at which the set is still cleared
        lo, hi = 0.0, 3.9 - float(spread.max())
        rec = _records(hi, ang, spread, hz, r)
        if rec is None or not _clears_rebased(_level_record(*rec, k1), s, d, k2):
            continue                                   # never cleared inside the +-4 m the builder admits: there is no suffix to check
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            rec = _records(mid, ang, spread, hz, r)
            if _clears_rebased(_level_record(*rec, k1), s, d, k2):
                hi = mid
            else:
                lo = mid
        rec = _records(hi, ang, spread, hz, r)
        assert _clears_rebased(_level_record(*rec, k1), s, d, k2)
        worst = min(worst, _check_cleared(rec, s, d, f"edge D = {hi}"))
        tight += 1
        zmin, zmax = float(rec[2].astype(np.float64).min()), float(rec[2].astype(np.float64).max())
        seen["up" if d[2] > 0 else "down"] += 1
        seen["above" if s[2] > 0 else "below"] += 1
        seen["high"] += abs(float(s[2])) >= 2.0
        seen["straddle" if zmin < 0.0 < zmax else "one_side"] += 1
        seen["centre"] += it % 5 == 0
    assert tight > 500 and sampled > 300, (tight, sampled)
    assert all(v > 40 for v in seen.values()), seen              # every kind of ray and suffix reached the bound's edge
    assert worst < 0.5                                           # the edge is not far from test (A)'s own: the bound is not vacuous


def test_only_steep_rays_clear_and_none_from_the_tame_limit():
    """cos(beta) < 0.9: nothing is cleared, whatever the distances (the division by d_z is used only where it is well conditioned); d_z = 0
    gives an infinity or a NaN that compares false.  A line whose ground point lies 9 km from the row clears nothing either."""
    rng = np.random.default_rng(7)
    k1, k2 = _far_consts()
    rec = _records(3.0, np.array([0.3]), np.array([0.0]), np.array([0.0]), np.array([0.01]))
    level = _level_record(*rec, k1)
    n_flat = 0
    for _ in range(400):
        s, d = _ray(rng, steep=False)
        assert not _clears_rebased(level, s, d, k2)
        n_flat += 1
    for d in (np.array([1.0, 0.0, 0.0], dtype=f32), np.array([0.6, -0.8, 0.0], dtype=f32)):
        for s in (np.zeros(3, dtype=f32), np.array([0.05, 0.02, 0.7], dtype=f32)):
            assert not _clears_rebased(level, s, d, k2)
    for _ in range(200):
        s, d = _ray(rng, ground="limit")
        assert np.abs(s[0:2]).max() < 1.0e4
        assert not _clears_rebased(level, s, d, k2)
    # both sides of the limit in one sweep: cos(beta) = 0.9 at 0.4510 rad
    for tilt, want in ((0.4450, True), (0.4500, True), (0.4512, False), (0.4600, False)):
        d = np.array([math.sin(tilt), 0.0, -math.cos(tilt)], dtype=f32)
        s = (np.array([0.0, 0.0, 0.0]) + (1.0 / float(d[2])) * d.astype(np.float64)).astype(f32)      # 1 m up, ground point on C
        assert _clears_rebased(level, s, d, k2) == want, tilt
    assert n_flat == 400


def test_s_prime_lies_on_the_line_at_the_rows_height():
    """What catches a sign error in s': the float32 point is within LN_REB_ERR |s_z| + 1e-7 |s'| of where the float64 line crosses z_c."""
    rng = np.random.default_rng(3)
    for _ in range(3000):
        s, d = _ray(rng, ground=rng.choice(["centre", "row", "limit"]))
        lx, ly = _s_prime(s, d)
        s64, d64 = s.astype(np.float64), d.astype(np.float64)
        want = s64[0:2] - (s64[2] / d64[2]) * d64[0:2]
        err = math.hypot(float(lx) - want[0], float(ly) - want[1])
        assert err <= 0.25 * float(LN_REB_ERR) * abs(float(s[2])) + 1.0e-7 * math.hypot(*want) + 1.0e-12, (err, s, d)


def test_the_rebased_form_gives_up_only_the_axial_term():
    """On a suffix that lies at the row's height (z0 = z1 = 0: the two forms bound the same geometry) the rebased form's slack is never
    below the origin form's by more than

        2 k2 |dxy|^2 |s_z|   +   0.0025 k2 |s_z|   +   the rounding term,

    the price of bounding the axial part by the triangle inequality about s' (first term; zero for a vertical ray) with |d| <= 1.0021
    (second).  Both are a few per cent of the drift |s_z| tan(beta) that the origin form charges in full whenever the line's ground point is
    nearer to C than the origin is.  (Stated for suffixes off the row's height the comparison is no theorem and is not asserted: a set at
    the ORIGIN's height has dzm = 0 from the origin and |s_z| from s', e.g. z0 = z1 = s_z = 0.3, a vertical ray: the origin form charges
    nothing for height, the rebased one 0.3 k2 (|dz|^2 + 1.0025).)  The sum over the cases must also show the gain: with the ground point
    drawn independently of the origin's height, the rebased slack is the larger one on average."""
    rng = np.random.default_rng(11)
    k1, k2 = _far_consts()
    gain = []
    for _ in range(3000):
        s, d = _ray(rng)
        G = f32(np.float16(rng.uniform(0.05, 1.5)))
        ro = f32(np.float16(float(G) + rng.uniform(0.0, 1.0)))
        level = (G, f32(0.0), f32(0.0), ro)
        steep_r, slack_r = _rebased_form(level, s, d, k2)
        steep_o, slack_o = _origin_form(level, s, d, k2)
        assert steep_r == steep_o and steep_r
        assert (_clears(level, s, d, k2)) == bool(slack_o > 0.0)              # the origin form is the one the existing test restates
        sq2 = float(d[0]) ** 2 + float(d[1]) ** 2
        asz = abs(float(s[2]))
        allowed = (2.0 * sq2 + 0.0025) * float(k2) * asz * 1.001 + 2.0e-6 * (1.0 + asz + math.hypot(float(s[0]), float(s[1])))
        assert float(slack_r) >= float(slack_o) - allowed, (float(slack_r), float(slack_o), allowed, s, d)
        gain.append(float(slack_r) - float(slack_o))
    assert np.mean(gain) > 0.01, np.mean(gain)
