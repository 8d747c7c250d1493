"""Property tests (CPU, numpy) of the staged tables' shared-row form — `lane_union_kernel`, `lane_build_kernel` with `upair`,
`lane_exact`'s membership filter in csrc/rover_cull.hip; DESIGN.md §5.7.

A row serves the cells (ix, 2j) and (ix, 2j + 1): it holds the union of their triangles, paired again, each id word carrying which of the
two cells lists the triangle, and its bounds are taken about the midpoint of the two cell centres.  Claims checked here:
  * the union row holds every triangle of each cell exactly once, and the membership bits reproduce each cell's own set exactly — so the
    exact phase, which drops a triangle the ray's cell does not list, evaluates candidates of the cell's own K-set only;
  * the suffix bound of `tests/test_level_bound_property.py`, restated about the midpoint, holds for every record of the suffix at the
    bound's edge with the ray's origin as far from the midpoint as a ray of either cell can be (o = o_max = sqrt(0.05^2 + 0.1^2) m at
    0.1 m cells) — including records listed by the OTHER cell only: a bound over a superset bounds each cell's subset.
"""
import math

import numpy as np

from test_level_bound_property import _clears, _far_consts, _level_record, _random_case, _records, _test_a_margin

f32 = np.float32
IDMASK = 0x3FFFFFFF
CELL = 0.1
O_MAX = math.sqrt((0.5 * CELL) ** 2 + CELL ** 2)


def _union_row(set0, set1):
    """lane_union_kernel: the distinct triangles of both cells in id order with their membership bits, partners (2p, 2p + 1) that are both
    in the union in one pair, the rest paired up in id order behind them -> [(word0, word1)], word = id | membership << 30 (0: no triangle)."""
    keys = sorted([(int(t) << 1) | 0 for t in set0] + [(int(t) << 1) | 1 for t in set1])
    uid = []
    for k in keys:
        t, side = k >> 1, k & 1
        if uid and (uid[-1] & IDMASK) == t:
            uid[-1] |= 1 << (30 + side)
        else:
            uid.append(t | (1 << (30 + side)))
    ids = [w & IDMASK for w in uid]
    have = set(ids)
    firsts = [w for w in uid if not (w & 1) and ((w & IDMASK) | 1) in have]
    seconds = {(w & IDMASK) ^ 1: w for w in uid if (w & 1) and ((w & IDMASK) ^ 1) in have}
    singles = [w for w in uid if not ((w & IDMASK) ^ 1) in have]
    rows = [(w, seconds[w & IDMASK]) for w in firsts]
    for i in range(0, len(singles), 2):
        rows.append((singles[i], singles[i + 1] if i + 1 < len(singles) else 0))
    return rows


def _listed(rows, parity):
    """The triangles lane_exact evaluates for a ray of the row's cell `parity`: those whose bit 30 + parity is set."""
    return sorted((w & IDMASK) for pair in rows for w in pair if (w >> (30 + parity)) & 1)


def _check_row(set0, set1):
    rows = _union_row(set0, set1)
    words = [w for pair in rows for w in pair if w >> 30]
    ids = [w & IDMASK for w in words]
    assert len(ids) == len(set(ids)), "a triangle sits in the row once"
    assert set(ids) == set(int(t) for t in set0) | set(int(t) for t in set1), "the row is the union"
    assert _listed(rows, 0) == sorted(int(t) for t in set0), "bit 30 reproduces the even cell's set"
    assert _listed(rows, 1) == sorted(int(t) for t in set1), "bit 31 reproduces the odd cell's set"
    for a, b in rows[:-1]:
        assert a >> 30 and b >> 30, "only the last pair may hold one triangle"
    return len(rows)


def test_union_row_holds_both_cells_and_the_bits_tell_them_apart():
    rng = np.random.default_rng(20261019)
    for _ in range(300):
        t_max = int(rng.choice([64, 1000, 1 << 20, (1 << 26) - 2]))
        k = int(rng.integers(1, 201))
        pool = rng.choice(t_max, size=min(t_max, int(k * rng.uniform(1.0, 2.5)) + 1), replace=False)
        set0 = rng.choice(pool, size=min(k, pool.size), replace=False)
        set1 = rng.choice(pool, size=min(k, pool.size), replace=False)
        _check_row(set0, set1)
    # a column's last row at Y odd: one cell, the other side empty
    assert _listed(_union_row([5, 4, 9], []), 0) == [4, 5, 9] and _listed(_union_row([5, 4, 9], []), 1) == []
    # disjoint neighbours: nothing shared, 2 K triangles
    assert _check_row(range(0, 400, 2), range(1, 400, 2)) == 200


def test_the_grid_meshs_unions_fit_a_row_at_k_200():
    """What the form is taken on: K = 200 nearest triangles of two neighbouring cells of the regular mesh share all but about 23, and with the
    two halves of a mesh cell numbered 2p, 2p + 1 the union is at most 112 pairs — 14 chunks of the 16 a row holds."""
    from isaac_rover_amd import synth
    n = 20
    m = synth.knn_map_grid(n, n + 1, 200, "cpu").numpy()
    worst = 0
    for x in range(n):
        for j in range(0, n - 1, 2):
            worst = max(worst, _check_row(m[x, j], m[x, j + 1]))
    assert 100 < worst <= 128, worst


def test_a_suffix_cleared_about_the_midpoint_passes_test_a_for_both_cells_records():
    """test_level_bound_property's search with the origin on the circle o = O_MAX about the row's centre: the corner of either cell that lies
    farthest from the midpoint of the two centres.  Every record of the suffix passes test (A), whichever cell lists its triangle."""
    rng = np.random.default_rng(4242)
    k1, k2 = _far_consts()
    tight, worst = 0, math.inf
    for _ in range(1500):
        ang, spread, hz, r, s, d = _random_case(rng)
        corner = rng.integers(4)                                           # (+-0.05, +-0.1) about the midpoint, as float32 holds them
        s = np.array([(0.5 * CELL) * (1 if corner & 1 else -1), CELL * (1 if corner & 2 else -1), s[2]], dtype=f32)
        assert abs(float(np.hypot(s[0], s[1])) - O_MAX) < 1.0e-7
        member = rng.integers(1, 4, size=ang.size)                         # 1: the even cell only, 2: the odd cell only, 3: both
        member[0] = 2 if s[1] < 0 else 1                                   # ... the nearest one by the OTHER cell only
        lo, hi = 0.0, 3.9 - float(spread.max())
        rec = _records(hi, ang, spread, hz, r)
        if rec is None or not _clears(_level_record(*rec, k1), s, d, k2):
            continue
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            rec = _records(mid, ang, spread, hz, r)
            if _clears(_level_record(*rec, k1), s, d, k2):
                hi = mid
            else:
                lo = mid
        rec = _records(hi, ang, spread, hz, r)
        assert _clears(_level_record(*rec, k1), s, d, k2)
        margin = _test_a_margin(*rec, s.astype(np.float64), d.astype(np.float64))
        assert (margin > 0.0).all(), f"cleared about the midpoint at D = {hi}, but a record (membership {member[margin.argmin()]}) fails test (A): {margin.min()}"
        worst = min(worst, float(margin.min()))
        tight += 1
    assert tight > 500
    assert worst < 0.5
