"""Property test (CPU, numpy) of the KNN map builder's ring search — `knn_select_kernel` in csrc/rover_knn.hip, DESIGN.md §4.6.

The search of a cell stops at ring r when its K-th key is within a bound that no centroid outside ring r can undercut.  "Outside ring r"
is decided by `knn_bucket` in float32 — a subtraction, a product with fl(1 / g), a floor — so a centroid can sit a few ulps NEARER than
r g and still be r + 1 buckets away.  The stop test therefore carries a slack (knn_ref.STOP_SLACK, the kernel's KNN_STOP_SLACK).  The GPU
suite (test_knn_builder_gpu.py) checks the consequence, lists equal to brute force; this file checks

  * that the inputs of knn_ref.contested_cells do reach the hazard: a model of the search WITHOUT slack returns wrong lists on them;
  * the inequality itself at its tightest, for both rankings, on pairs aimed at bucket edges up to 60 m from the origin;
  * that the model WITH the shipped slack equals brute force, on those inputs and on random soups.
"""
import numpy as np
import pytest

import knn_ref
from knn_ref import f32

# (x0, span, y0, span_y): bucket origin and extent of the centroids' bounding box; res = 0.1, a 40 x 40 map.  Origins 0.5, 0.7 and 2.3
# (span 4, 4, 3) and -49.7 (the last row with that x0) were scanned too and have no contested cell.
CONTESTED = {"x0=0.3": (0.3, 4.0, None, None), "x0=1.1": (1.1, 4.0, None, None), "offset 50 m": (-50.3, 56.3, 0.3, 1.2)}
N_CELLS, RES = 40, 0.1


def _contested(name, k):
    x0, span, y0, span_y = CONTESTED[name]
    return knn_ref.contested_cells(x0, span, RES, k=k, t=4096, n_x=N_CELLS, n_y=N_CELLS, y0=y0, span_y=span_y)


@pytest.mark.parametrize("name,k", [("x0=0.3", 2), ("x0=0.3", 5), ("x0=1.1", 2), ("x0=1.1", 5), ("offset 50 m", 2)])
def test_contested_inputs_defeat_a_stop_test_without_slack_and_not_the_shipped_one(name, k):
    verts, tris, corners, cells = _contested(name, k)
    assert len(tris) == 4096 and len(cells) >= 1, "the generator found no contested cell for this origin"
    cx, cy = knn_ref.centroids(verts, tris)
    grid = knn_ref.bucket_grid(cx, cy, k, RES)
    assert grid.g == f32(RES) and (cx[corners[0]], cy[corners[0]]) == (grid.x0, grid.y0)
    want = knn_ref.brute_force(verts, tris, N_CELLS, N_CELLS, RES, k)
    where = [(x, y) for x, y, _, _ in cells]
    naive = knn_ref.ring_search(cx, cy, N_CELLS, N_CELLS, RES, k, slack=0.0, cells=where)
    shipped = knn_ref.ring_search(cx, cy, N_CELLS, N_CELLS, RES, k, cells=where)
    for x, y, r, missed in cells:
        assert missed in want[x, y] and missed not in naive[x, y], f"cell ({x}, {y}): ring {r} without slack does not miss centroid {missed}"
        np.testing.assert_array_equal(shipped[x, y], want[x, y], err_msg=f"cell ({x}, {y}) with the shipped slack")
    print(f"{name}, K = {k}: contested cells (x, y, ring) {[(x, y, r) for x, y, r, _ in cells]}")


def _edge_pairs(rng, n, fp16, extent):
    """n (cell coordinate p, centroid coordinate c) pairs on one axis, both within 3 ulps of a bucket edge of a random grid: g in
    0.03 .. 0.5, origin and coordinates within +-extent (fp16 values for the reference ranking).  -> o, g, p, c, ring, with
    ring = |bucket(c) - bucket(p)| - 1: the largest ring that does not gather c."""
    g = rng.uniform(0.03, 0.5, n).astype(f32)
    o = rng.uniform(-extent, extent, n)
    o = (o.astype(np.float16) if fp16 else o).astype(f32)
    nb = np.floor((extent - o.astype(np.float64)) / g).astype(np.int64)               # buckets between the origin and +extent
    m = (rng.random(n) * np.maximum(nb - 1, 1)).astype(np.int64) + 1                  # p sits at the upper edge of bucket m - 1
    r = np.minimum(rng.integers(1, 5, n) * rng.choice([1, 1, 1, 10], n), np.maximum(nb - m, 1))
    side = rng.choice([1, -1], n)                                                     # c above p, or below it
    ep = o.astype(np.float64) + m * g.astype(np.float64)
    ec = o.astype(np.float64) + np.maximum(m + side * r, 0) * g.astype(np.float64)

    def near(e):
        if fp16:
            h = e.astype(np.float16).view(np.int16) + (rng.integers(-2, 3, n) * np.sign(e)).astype(np.int16)
            return h.view(np.float16).astype(f32)
        v = e.astype(f32).view(np.int32) + (rng.integers(-3, 4, n) * np.sign(e)).astype(np.int32)
        return v.view(f32)
    p, c = near(ep), near(ec)
    inv_g = f32(1) / g
    big = 1 << 22
    bp = np.array(knn_ref.knn_bucket(p, o, inv_g, big))
    bc = np.array(knn_ref.knn_bucket(c, o, inv_g, big))
    keep = (p >= o) & (c >= o) & (np.abs(bc - bp) >= 2)
    return o[keep], g[keep], p[keep], c[keep], (np.abs(bc - bp) - 1)[keep]


def test_no_centroid_outside_a_ring_undercuts_the_exact_f32_stop_bound():
    """exact_f32: d2 of a centroid outside ring r, in the kernel's arithmetic with dy = 0 (its smallest), is strictly above
    stop_limit(r) with span at ITS smallest (the larger of |c - o|, |p - o|) — so a K-th key <= stop_limit(r) is final.  Without the
    slack the same pairs do undercut (r g)^2: the bound is needed, and it is not far off."""
    rng = np.random.default_rng(20261019)
    n_pairs = n_naive = 0
    tightest = np.inf
    for extent in (60.0, 60.0, 60.0, 60.0, 60.0, 60.0, 4.0, 1.0):
        o, g, p, c, ring = _edge_pairs(rng, 400_000, False, extent)
        dx = c - p
        d2 = dx * dx
        span = np.maximum(np.abs(c - o), np.abs(p - o))
        lim = knn_ref.stop_limit(ring, g, span, knn_ref.STOP_SLACK)
        bad = ~(d2 > lim)
        assert not bad.any(), f"{bad.sum()} centroids outside their ring are within the stop bound, e.g. o, g, p, c = " \
                              f"{[float(a[bad][0]) for a in (o, g, p, c)]} ring {ring[bad][0]}"
        reach = ring.astype(f32) * g
        n_naive += int((d2 < reach * reach).sum())
        tightest = min(tightest, float(((np.sqrt(d2.astype(np.float64)) - np.sqrt(lim.astype(np.float64))) / g).min()))
        n_pairs += len(d2)
    assert n_pairs >= 1_000_000
    assert n_naive > 1000, "the pairs never reached the hazard: some must undercut (r g)^2 itself"
    assert tightest < 1.0e-2, "the bound gives away more than 1 % of a bucket edge"
    print(f"exact_f32: {n_pairs} pairs, {n_naive} below (r g)^2, smallest (d - lim) / g = {tightest:.3e}")


def test_no_centroid_outside_a_ring_undercuts_the_reference_fp16_stop_bound():
    """reference_fp16: the key of a centroid outside ring r — fp16(sqrt(fl(dx dx))) with dx = fp16(c - p) — is at least the
    threshold reach (1 - 2^-9) a K-th key has to stay strictly below (fp16-valued coordinates up to 60 m)."""
    rng = np.random.default_rng(7)
    n_pairs = 0
    closest = np.inf
    for extent in (60.0, 60.0, 60.0, 60.0, 60.0, 60.0, 4.0, 1.0):
        o, g, p, c, ring = _edge_pairs(rng, 400_000, True, extent)
        dx = (c - p).astype(np.float16).astype(f32)
        key = np.sqrt(dx * dx).astype(np.float16).astype(f32)
        thr = (ring.astype(f32) * g) * (f32(1) - f32(1) / f32(512))
        bad = ~(key >= thr)
        assert not bad.any(), f"{bad.sum()} keys outside their ring are below the threshold, e.g. o, g, p, c = " \
                              f"{[float(a[bad][0]) for a in (o, g, p, c)]} ring {ring[bad][0]}"
        closest = min(closest, float(((key - thr) / (ring.astype(f32) * g)).min()))
        n_pairs += len(key)
    assert n_pairs >= 1_000_000
    print(f"reference_fp16: {n_pairs} pairs, smallest (key - threshold) / reach = {closest:.3e}")


def test_the_search_with_the_shipped_slack_equals_brute_force_on_random_soups():
    for seed in range(20):
        rng = np.random.default_rng(seed)
        t, k, n = int(rng.integers(40, 700)), int(rng.integers(1, 24)), int(rng.integers(5, 12))
        off = float(rng.choice([0.0, 0.0, 30.0, -55.0]))
        centers = rng.uniform(-0.3, n * RES + 0.3, (t, 1, 2)) + np.array([off, 0.0])
        verts = np.concatenate([centers + rng.normal(0, 0.05, (t, 3, 2)), np.zeros((t, 3, 1))], axis=2).reshape(-1, 3).astype(f32)
        if seed % 3 == 0:
            verts = (np.round(verts / (RES / 3)) * (RES / 3)).astype(f32)          # a lattice: exact ties, centroids on bucket edges
        tris = np.arange(3 * t, dtype=np.int32).reshape(t, 3)
        cx, cy = knn_ref.centroids(verts, tris)
        got = knn_ref.ring_search(cx, cy, n, n, RES, k)
        np.testing.assert_array_equal(got, knn_ref.brute_force(verts, tris, n, n, RES, k), err_msg=f"soup {seed}")
