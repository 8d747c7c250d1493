"""Property test (CPU, numpy) of test (A) in BOX form — `lane_build_kernel` (box records) / `lane_scan_kernel` (the kBX body) in
csrc/rover_cull.hip, DESIGN.md §5.6.

A pair of triangles stored as one box {M', e, mrg} is cleared for a ray iff on one of the axes d x e_i
    |(d x h^)_i| - sum_{j != i} e_j |d_k| - (alpha' |h^|_1 + mrg) >= +0        (float32, in the kernel's operation order).
The claim the rejection proof needs: there is then a unit u perpendicular to d with
    |u . h| - max over the padded triangles' corners Q of |u . (Q - M)|  >=  alpha (|h|_2 + 2 rho'),   rho' >= max |Q - M|,
with room for the rounding of the ray's cell-relative origin upstream of the test; in particular the ray's line cannot meet a padded
triangle, so no triangle `ray_distance` can hit is ever cleared.  The GPU suite checks the consequence (tests/test_lane_box_gpu.py); this
test checks the inequality itself at its edge: the ray is moved towards the box until the float32 test JUST clears it, for random pairs
and rays, for lines that graze a box corner, for exactly axis-parallel directions and for a degenerate box of zero extent.

numpy rounds each operation; an fma is restated as float32(float64 product + float64 addend): a double rounding differs from the single
one by an ulp at most, three orders of magnitude below the slack between alpha' and alpha.
"""
import math

import numpy as np

f32 = np.float32
f64 = np.float64
ALPHA = 0.005                          # CullK<0>::alpha
BOX_ALPHA = f32(5.05e-3)               # LN_BOX_ALPHA
PAD = 0.101                            # CullK<0>::pad
LN_PAD = 5.0e-5


def _h_up(v):
    """fp16 >= v (half_bits_up)."""
    h = np.float16(v)
    if float(h) < float(v):
        h = np.nextafter(h, np.float16(np.inf))
    return h


def _padded_corners(v0, v1, v2):
    """Corners of {a + n b + m c : n, m >= -pad, n + m <= 1 + pad}, a = v2, b = fl(v1 - a), c = fl(v0 - a) (ray_casting.py:34-36)."""
    a = v2.astype(f32)
    b = (v1.astype(f32) - a).astype(f64)
    c = (v0.astype(f32) - a).astype(f64)
    a = a.astype(f64)
    return np.stack([a - PAD * b - PAD * c, a + (1 + 2 * PAD) * b - PAD * c, a - PAD * b + (1 + 2 * PAD) * c]), a, b, c


def _box_record(corners, centre, extra=1.0e-4 + LN_PAD):
    """lane_build_kernel's box of a pair: centre fp16 relative to the cell's `centre`, half extents about the centre AS DECODED plus the
    builder's allowances, rounded up; mrg from the rounded extents.  -> (M' fp16 [3], e fp16 [3], mrg fp16, M float64 [3])"""
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    mh = np.float16((0.5 * (lo + hi) - centre).astype(f32))
    M = centre + mh.astype(f64)
    e = np.maximum(hi - M, M - lo) + extra
    eh = np.array([_h_up(f32(x * 1.0000001)) for x in e], dtype=np.float16)
    rho = math.sqrt(float((eh.astype(f64) ** 2).sum()))
    mrg = max(_h_up(f32((2.0 * float(BOX_ALPHA) * rho + 2.0e-5) * 1.000001)), np.float16(6.104e-5))
    return mh, eh, np.float16(mrg), M


def _fma(a, b, c):
    return f32(f64(a) * f64(b) + f64(c))


def _clears(rec, s_rel, d):
    """The kBX body of lane_scan_kernel: s_rel = the ray's cell-relative origin (float32), d its direction (float32)."""
    mh, eh, mrg = rec
    m = mh.astype(f32)
    ex, ey, ez = (f32(x) for x in eh)
    hx, hy, hz = f32(s_rel[0] - m[0]), f32(s_rel[1] - m[1]), f32(s_rel[2] - m[2])
    dx, dy, dz = (f32(x) for x in d)
    z = _fma(f32(f32(abs(hx) + abs(hy)) + abs(hz)), BOX_ALPHA, f32(mrg))
    cx = _fma(dz, hy, -f32(dy * hz)); cy = _fma(dx, hz, -f32(dz * hx)); cz = _fma(dy, hx, -f32(dx * hy))
    tx = _fma(-ez, abs(dy), _fma(-ey, abs(dz), f32(abs(cx) - z)))
    ty = _fma(-ez, abs(dx), _fma(-ex, abs(dz), f32(abs(cy) - z)))
    tz = _fma(-ey, abs(dx), _fma(-ex, abs(dy), f32(abs(cz) - z)))
    return max(tx, ty, tz) >= 0.0


def _proof_margin(corner_sets, M, s_abs, d):
    """max over the three axes of  |u . h| - max_Q |u . (Q - M)| - ALPHA (|h| + 2 rho'),  float64, true geometry (h = s - M)."""
    d = d.astype(f64)
    h = s_abs - M
    Q = np.concatenate(corner_sets) - M
    rho = float(np.sqrt((Q * Q).sum(axis=1)).max())
    best = -np.inf
    for i in range(3):
        u = np.cross(d, np.eye(3)[i])
        n = np.linalg.norm(u)
        if n < 1e-12:
            continue
        u /= n
        best = max(best, abs(u @ h) - float(np.abs(Q @ u).max()) - ALPHA * (np.linalg.norm(h) + 2.0 * rho))
    return best, float(np.linalg.norm(h))


def _line_meets_padded(a, b, c, s, d):
    """float64: does the LINE through s along d meet the padded triangle (ray_casting.py:59's region, either side of the origin)?"""
    A = np.stack([b, c, -d.astype(f64)], axis=1)                          # a + n b + m c = s + t d
    if abs(np.linalg.det(A)) < 1e-14 * np.linalg.norm(b) * np.linalg.norm(c):
        return False
    n, m, _t = np.linalg.solve(A, s - a)
    return n >= -PAD and m >= -PAD and n + m <= 1.0 + PAD


def _edge_check(tris, centre, s_in, s_out, d, label):
    """Bisect the origin between s_in (not cleared) and s_out (cleared) to where the float32 test just clears; check the proof's
    inequality there."""
    sets = [_padded_corners(*t) for t in tris]
    mh, eh, mrg, M = _box_record(np.concatenate([x[0] for x in sets]), centre)
    rec = (mh, eh, mrg)
    to_rel = lambda s: (s - centre).astype(f32)
    if _clears(rec, to_rel(s_in), d) or not _clears(rec, to_rel(s_out), d):
        return False                                                       # not a bracket (the far point is not far enough, say)
    lo, hi = 0.0, 1.0
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        if _clears(rec, to_rel(s_in + mid * (s_out - s_in)), d):
            hi = mid
        else:
            lo = mid
    s_rel = to_rel(s_in + hi * (s_out - s_in))
    assert _clears(rec, s_rel, d)
    s_abs = centre + s_rel.astype(f64)                                     # the origin the lane sees, as a real number
    margin, hn = _proof_margin([x[0] for x in sets], M, s_abs, d)
    # room for the upstream rounding of s' = fl(s - C): 2.4e-7 |h| + 5e-7 per component
    assert margin >= 1.0e-6 * (hn + 1.0), f"{label}: the box test cleared a pair {margin:.3e} from the proof's bound (|h| = {hn:.3f})"
    for _, a, b, c in sets:
        assert not _line_meets_padded(a, b, c, s_abs, d), f"{label}: cleared a triangle the line meets"
    return True


def _grid_pair(rng, scale=0.1):
    """The two halves of a (tilted, fp16) grid square near the cell centre, or a general pair of neighbouring triangles."""
    o = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)])
    if rng.random() < 0.6:
        p = [o + np.array([i * scale, j * scale, rng.uniform(-0.03, 0.03)]) for i in (0, 1) for j in (0, 1)]
        t = [(p[0], p[1], p[2]), (p[3], p[2], p[1])]
    else:
        p = [o + rng.uniform(-scale, scale, 3) * np.array([1.0, 1.0, 0.4]) for _ in range(4)]
        t = [(p[0], p[1], p[2]), (p[1], p[2], p[3])]
    h = lambda v: np.float16(v).astype(f64)
    return [tuple(h(v) for v in tri) for tri in t]


def _unit(v):
    v = np.asarray(v, dtype=f64)
    return (v / np.linalg.norm(v)).astype(f32)


def test_box_test_clears_no_pair_inside_the_proofs_bound_random():
    rng = np.random.default_rng(7)
    centre = np.array([12.35, 7.05, 0.4])
    done = 0
    for _ in range(1500):
        tris = _grid_pair(rng)
        tilt, az = rng.uniform(0.0, 1.55) * rng.choice([1.0, 0.3]), rng.uniform(0.0, 2.0 * math.pi)
        d = _unit([math.sin(tilt) * math.cos(az), math.sin(tilt) * math.sin(az), -math.cos(tilt)])
        mid = np.mean([np.mean(t, axis=0) for t in tris], axis=0)
        back = -d.astype(f64) * rng.uniform(0.05, 3.0)                     # the origin up the ray from a point inside the pair
        side = np.cross(d.astype(f64), rng.normal(size=3))
        side /= np.linalg.norm(side)
        done += _edge_check(tris, centre, mid + back, mid + back + side * 0.8, d, "random")
    assert done > 1200


def test_box_test_at_a_grazed_corner():
    """The line passes a corner of the box diagonally (the axis that separates is d x e_z for a flat ray, d x e_x / e_y for a steep one)."""
    rng = np.random.default_rng(11)
    centre = np.array([3.05, 3.05, 0.0])
    done = 0
    for _ in range(400):
        tris = _grid_pair(rng)
        corners = np.concatenate([_padded_corners(*t)[0] for t in tris])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        sx, sy = rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])
        corner = np.array([hi[0] if sx > 0 else lo[0], hi[1] if sy > 0 else lo[1], rng.uniform(lo[2], hi[2])])
        flat = rng.random() < 0.5
        if flat:       # in the horizontal plane, along the corner's diagonal tangent
            d = _unit([-sy, sx, rng.uniform(-1.0e-3, 1.0e-3)])
        else:          # steep, leaning along the tangent
            d = _unit([-sy * 0.3, sx * 0.3, -1.0])
        out = np.array([sx, sy, 0.0]) / math.sqrt(2.0)
        p_in = 0.5 * (lo + hi) - d.astype(f64) * rng.uniform(0.2, 2.0)
        p_out = corner + out * 0.5 - d.astype(f64) * rng.uniform(0.2, 2.0)
        done += _edge_check(tris, centre, p_in, p_out, d, "corner")
    assert done > 300


def test_box_test_with_axis_parallel_directions():
    """d = +-e_k exactly: one axis d x e_k vanishes (its test must fail by the margin alone), the other two are the box's own faces."""
    rng = np.random.default_rng(13)
    centre = np.array([0.95, 1.25, -0.2])
    done = 0
    for k in range(3):
        for sign in (1.0, -1.0):
            for _ in range(60):
                tris = _grid_pair(rng)
                d = np.zeros(3, dtype=f32); d[k] = sign
                mid = np.mean([np.mean(t, axis=0) for t in tris], axis=0)
                side = np.zeros(3); side[(k + 1 + int(rng.integers(0, 2))) % 3] = rng.choice([-1.0, 1.0])
                if rng.random() < 0.5:
                    side[(k + 2) % 3] += rng.uniform(-1.0, 1.0)
                    side[k] = 0.0
                start = mid - d.astype(f64) * rng.uniform(0.1, 2.0)
                done += _edge_check(tris, centre, start, start + side / np.linalg.norm(side) * 0.9, d, f"axis {k}")
    assert done > 300


def test_degenerate_box_of_zero_extent():
    """A box of zero extent (a point): hand-made record with e = 0 and the smallest mrg the builder can store; the test then says the line
    misses the point by alpha' |h|_1 + mrg on an axis — and the builder's own record of a degenerate (point) triangle pair is never smaller
    than its allowances."""
    rng = np.random.default_rng(17)
    centre = np.array([5.0, 5.0, 1.0])
    p = np.float16([0.03, -0.02, 0.01]).astype(f64) + centre
    mh = np.float16((p - centre).astype(f32))
    rec = (mh, np.zeros(3, dtype=np.float16), _h_up(f32(2.0e-5)))
    M = centre + mh.astype(f64)
    n_clear = 0
    for _ in range(600):
        d = _unit(rng.normal(size=3))
        if rng.random() < 0.2:
            d = np.zeros(3, dtype=f32); d[int(rng.integers(0, 3))] = rng.choice([-1.0, 1.0])
        side = np.cross(d.astype(f64), rng.normal(size=3))
        side /= np.linalg.norm(side)
        start = M - d.astype(f64) * rng.uniform(0.05, 3.0)
        lo, hi = 0.0, 0.5
        if _clears(rec, (start - centre).astype(f32), d) or not _clears(rec, (start + side * hi - centre).astype(f32), d):
            continue
        for _ in range(48):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if _clears(rec, (start + side * mid - centre).astype(f32), d) else (mid, hi)
        s_abs = centre + (start + side * hi - centre).astype(f32).astype(f64)
        margin, hn = _proof_margin([M[None, :]], M, s_abs, d)
        assert margin >= 1.0e-6 * (hn + 1.0), f"zero-extent box: {margin:.3e} from the bound at |h| = {hn:.3f}"
        n_clear += 1
    assert n_clear > 400
    # a ray THROUGH the point is never cleared, whatever its direction
    for _ in range(200):
        d = _unit(rng.normal(size=3))
        assert not _clears(rec, (M - d.astype(f64) * rng.uniform(0.0, 3.0) - centre).astype(f32), d)
    _, eh, mrg, _ = _box_record(np.stack([p, p, p]), centre)
    assert (eh.astype(f64) >= 1.0e-4 + LN_PAD).all() and float(mrg) >= 2.0e-5


def test_always_and_never_candidate_records():
    """Extents +6e4 (a pair that cannot be encoded): never cleared for any tame ray, axis-parallel ones included (no NaN from inf x 0);
    extents -6e4 (an empty pair): cleared for every unit direction."""
    rng = np.random.default_rng(19)
    always = (np.zeros(3, dtype=np.float16), np.float16([6.0e4] * 3), np.float16(1.0))
    never = (np.zeros(3, dtype=np.float16), np.float16([-6.0e4] * 3), np.float16(6.104e-5))
    for i in range(400):
        d = _unit(rng.normal(size=3))
        if i % 4 == 0:
            d = np.zeros(3, dtype=f32); d[i // 4 % 3] = 1.0 if i % 8 else -1.0
        s = (rng.uniform(-1.0, 1.0, 3) * rng.choice([1.0, 100.0, 9.9e3])).astype(f32)
        assert not _clears(always, s, d)
        assert _clears(never, s, d)
