"""rover_build_knn_map against brute force (knn_ref.brute_force) at the edges of its bucketed ring search and of the three-level scan
behind it: csrc/rover_knn.hip `knn_*_kernel`, csrc/rover_sort.hip `launch_scan_exclusive`; csrc/rover_capi_scene.cpp `build_knn_map_impl`; DESIGN.md §4.6.

Every case compares the whole [X, Y, K] map with assert_array_equal.  A wrong list is otherwise silent: the step and the oracle are fed
the same built map.  Large meshes go with long thin maps, so that the brute force stays small.
"""
import numpy as np
import pytest

import knn_ref
from knn_ref import f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(8, device=0)
    yield e
    e.close()


def _build(eng, verts, tris, n_x, n_y, res, k, **kw):
    return eng.build_knn_map(verts, tris, n_x, n_y, res, k, **kw).cpu().numpy()


def _check(eng, verts, tris, n_x, n_y, res, k, **kw):
    got = _build(eng, verts, tris, n_x, n_y, res, k, **kw)
    np.testing.assert_array_equal(got, knn_ref.brute_force(verts, tris, n_x, n_y, res, k, **kw))
    return got


def _soup(rng, t, lo, hi, size=0.05):
    """t small random triangles with centres uniform in the box lo .. hi (xy) -> verts [3t, 3], tris [t, 3]."""
    centers = rng.uniform(lo, hi, (t, 1, 2))
    verts = np.concatenate([centers + rng.normal(0, size, (t, 3, 2)), rng.normal(0, 0.1, (t, 3, 1))], axis=2)
    return verts.reshape(-1, 3).astype(f32), np.arange(3 * t, dtype=np.int32).reshape(t, 3)


# ------------------------------------------------------------------------------------------------ the stop test at bucket edges
@pytest.mark.parametrize("name,k", [("x0=0.3", 2), ("x0=0.3", 5), ("x0=1.1", 2), ("x0=1.1", 5), ("offset 50 m", 2)])
def test_contested_cells(eng, name, k):
    """Inputs on which a centroid a few ulps inside r g is bucketed r + 1 rings away (knn_ref.contested_cells;
    test_knn_ring_property.py shows that a stop test without slack misses it).  Ids shuffled; two builds give the same bytes."""
    from test_knn_ring_property import CONTESTED, N_CELLS, RES
    x0, span, y0, span_y = CONTESTED[name]
    verts, tris, _, cells = knn_ref.contested_cells(x0, span, RES, k=k, t=4096, n_x=N_CELLS, n_y=N_CELLS, y0=y0, span_y=span_y)
    assert len(cells) >= 1
    tris, perm = knn_ref.shuffle_ids(tris, seed=11)
    got = _build(eng, verts, tris, N_CELLS, N_CELLS, RES, k)
    want = knn_ref.brute_force(verts, tris, N_CELLS, N_CELLS, RES, k)
    new_id = np.argsort(perm)
    for x, y, r, missed in cells:
        assert new_id[missed] in want[x, y]
        assert new_id[missed] in got[x, y], f"cell ({x}, {y}): the centroid bucketed outside ring {r} is missing from the list"
    np.testing.assert_array_equal(got, want)
    assert _build(eng, verts, tris, N_CELLS, N_CELLS, RES, k).tobytes() == got.tobytes()


@pytest.mark.parametrize("snap", [False, True])
def test_far_from_the_origin(eng, snap):
    """A soup over x in 50 .. 60 m under a 60 m long, 3 cells wide map: float32 coordinates are coarsest here, and most cells lie
    outside the bucket grid.  snap: vertices on multiples of res / 3, a lattice with exact ties and centroids on bucket edges."""
    res = 0.1
    verts, tris = _soup(np.random.default_rng(50), 5000, (50.0, -0.3), (60.0, 0.5))
    if snap:
        verts = (np.round(verts.astype(np.float64) / (res / 3)) * (res / 3)).astype(f32)
    _check(eng, verts, tris, 600, 3, res, 16)


# ------------------------------------------------------------------------------------------------ ties
def _tie_lattice(n, res, copies, k_max, seed):
    """Centroids on the cell points of an n x n map themselves (res a power of two: all distances exact, tie groups 1 / 4 / 4 / 4 by
    distance 0, res, sqrt2 res, 2 res), each `copies` times, a clump inside one bucket so that the sizing gives g = res; ids shuffled."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    sx = np.tile(3.0 * res * i.ravel(), copies)
    sy = np.tile(3.0 * res * j.ravel(), copies)
    area = ((n - 1) * res) ** 2
    n_fill = int(area * k_max / (4.0 * res * res) * 1.2) + 1 - len(sx)
    rng = np.random.default_rng(seed)
    fill = 3.0 * res * (n - 3 + 0.25 + 0.5 * rng.random((2, max(n_fill, 0))))
    verts, tris = knn_ref.mesh_of_sums(np.concatenate([sx, fill[0]]), np.concatenate([sy, fill[1]]))
    return verts, knn_ref.shuffle_ids(tris, seed)[0]


@pytest.mark.parametrize("copies,ks", [(1, (1, 4, 5, 9, 13)), (2, (1, 5, 9, 13))])
def test_exact_ties_and_duplicate_centroids(eng, copies, ks):
    """K inside and at the ends of the tie groups; copies = 2: coincident pairs, an odd K splits one.  Ties go by ascending id."""
    n, res = 24, 0.125
    verts, tris = _tie_lattice(n, res, copies, max(ks), seed=3)
    grid = knn_ref.bucket_grid(*knn_ref.centroids(verts, tris), max(ks), res)
    assert grid.g == f32(res) and grid.x0 == 0 and grid.y0 == 0            # every lattice centroid sits on a bucket corner
    for k in ks:
        got = _check(eng, verts, tris, n, n, res, k)
        assert _build(eng, verts, tris, n, n, res, k).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ the scan
@pytest.mark.parametrize("nbx,nby", [(23, 89), (32, 64), (63, 65), (64, 64), (201, 201)])
def test_scan_lengths(eng, nbx, nby):
    """launch_scan_exclusive scans nb + 1 bucket counts in tiles of 2048: lengths 2048, 2049, 4096, 4097 and 40 402 (20 tiles).  The
    mesh is sparse (K = 2), g = res; the map's 4 rows of cells run along x through the buckets of highest j, so every tile's offsets,
    the last bucket's included, are read."""
    res, k = 0.1, 2
    x0, y0 = -0.5 * res, -(nby - 3.5) * res
    x1, y1 = x0 + (nbx - 0.5) * res, y0 + (nby - 0.5) * res
    t = int(nbx * nby * k / 4 * 1.3) + 2
    rng = np.random.default_rng(nbx * nby)
    sx = np.concatenate([[x0, x1], rng.uniform(x0, x1, t - 2)]) * 3.0
    sy = np.concatenate([[y0, y1], rng.uniform(y0, y1, t - 2)]) * 3.0
    verts, tris = knn_ref.mesh_of_sums(sx, sy)
    grid = knn_ref.bucket_grid(*knn_ref.centroids(verts, tris), k, res)
    assert (grid.g, grid.nbx, grid.nby) == (f32(res), nbx, nby)
    n_x, n_y = nbx, 4
    px, py = knn_ref.cell_tables(n_x, n_y, res)
    bx = knn_ref.knn_bucket(px, grid.x0, grid.inv_g, nbx)
    by = knn_ref.knn_bucket(py, grid.y0, grid.inv_g, nby)
    np.testing.assert_array_equal(bx, np.arange(nbx))                    # one cell column per bucket column: every tile is visited
    last = int(bx[-1]) * nby + int(by[-1])
    assert last == grid.nb - 1 and (last + 1) // knn_ref.SCAN_TILE == grid.nb // knn_ref.SCAN_TILE     # bucket_start[nb]: the last tile's last entry
    _check(eng, verts, tris, n_x, n_y, res, k)


# ------------------------------------------------------------------------------------------------ overflow: retry and refusal
def _dense_patch_mesh():
    rng = np.random.default_rng(12)
    res = 0.1
    centre = np.array([15 * res, 2 * res])
    c = np.concatenate([centre + rng.uniform(-0.025, 0.025, (9000, 2)), rng.uniform(0.0, 3.0, (3000, 2))])
    verts, tris = knn_ref.mesh_of_sums(3.0 * c[:, 0], 3.0 * c[:, 1])
    return verts, knn_ref.shuffle_ids(tris, 12)[0], res


def test_a_ring_that_overflows_is_retried_with_smaller_buckets(eng):
    """9000 of 12 000 centroids inside a 0.05 m patch around cell (15, 2): ring 1 of that cell holds the whole patch on the first grid
    (more than the 8192 keys a search holds), the bucket edge is halved until it does not.  Same lists as brute force."""
    verts, tris, res = _dense_patch_mesh()
    cx, cy = knn_ref.centroids(verts, tris)
    assert 0.05 < float(knn_ref.bucket_grid(cx, cy, 16, res).g)
    with pytest.raises(OverflowError):
        knn_ref.ring_search(cx, cy, 30, 4, res, 16, cells=[(15, 2)])
    knn_ref.ring_search(cx, cy, 30, 4, res, 16, cells=[(15, 2)], attempts=6)     # some later grid does hold it
    _check(eng, verts, tris, 30, 4, res, 16)


def test_a_mesh_too_dense_is_refused_and_leaves_nothing_behind(eng):
    """9000 coincident centroids: no bucket edge separates them, every retry overflows.  The library's own error path; the engine
    then builds a good map as if nothing had happened."""
    from isaac_rover_amd import _lib
    verts, tris = knn_ref.mesh_of_sums(np.full(9000, 3.0), np.full(9000, 1.5))
    with pytest.raises(_lib.RoverError, match="more than 8192 candidate"):
        eng.build_knn_map(verts, tris, 12, 4, 0.1, 16)
    verts, tris = _soup(np.random.default_rng(1), 1500, (-0.2, -0.2), (1.4, 0.6))
    _check(eng, verts, tris, 12, 4, 0.1, 16)


# ------------------------------------------------------------------------------------------------ K
@pytest.mark.parametrize("t,k", [(500, 1), (300, 300), (4096, 4096)])
def test_k_edges(eng, t, k):
    """K = 1; K = T, where the search ends by covering the grid with exactly K keys; K = T = 4096, the builder's limit."""
    verts, tris = _soup(np.random.default_rng(t), t, (-0.2, -0.2), (1.0, 0.6))
    _check(eng, verts, tris, 9, 4, 0.1, k)


def test_k_above_the_limit_is_refused(eng):
    from isaac_rover_amd import _lib
    verts, tris = _soup(np.random.default_rng(2), 5000, (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(_lib.RoverError, match="limit of 4096"):
        eng.build_knn_map(verts, tris, 4, 4, 0.1, 4097)


# ------------------------------------------------------------------------------------------------ degenerate input
def test_nan_vertices_and_out_of_range_indices(eng):
    """2 % of the triangles have a NaN vertex (the first triangle among them), 2 % an index >= V or < 0, which reads vertex 0.  A NaN
    centroid ranks after every finite one: with more finite centroids than K none is listed."""
    t, k = 10000, 16
    rng = np.random.default_rng(4)
    verts, tris = _soup(rng, t, (-0.2, -0.2), (3.2, 0.6))
    nan_tris = np.concatenate([[0], rng.choice(np.arange(1, t), t // 50 - 1, replace=False)])
    for i, tri in enumerate(nan_tris):
        verts[3 * tri + i % 3, [(0,), (1,), (0, 1, 2)][i % 3]] = np.nan    # x, y, or the whole vertex
    bad = rng.choice(np.setdiff1d(np.arange(t), nan_tris), t // 50, replace=False)
    tris[bad, rng.integers(0, 3, len(bad))] = rng.choice([len(verts), len(verts) + 7, 2 ** 31 - 1, -1, -(2 ** 31)], len(bad))
    cx, cy = knn_ref.centroids(verts, tris)
    is_nan = np.isnan(cx) | np.isnan(cy)
    assert np.isnan(verts[0]).any() and is_nan[0] and is_nan[bad].all() and is_nan.sum() == len(nan_tris) + len(bad)
    got = _check(eng, verts, tris, 32, 4, 0.1, k)
    assert not is_nan[got].any()


def test_out_of_range_indices_read_vertex_zero(eng):
    """The same with a finite vertex 0: the triangles with a bad index have centroids like any other and are listed."""
    t = 3000
    rng = np.random.default_rng(5)
    verts, tris = _soup(rng, t, (-0.2, -0.2), (3.2, 0.6))
    bad = rng.choice(t, t // 50, replace=False)
    tris[bad, rng.integers(0, 3, len(bad))] = rng.choice([len(verts), 2 ** 31 - 1, -1, -(2 ** 31)], len(bad))
    got = _check(eng, verts, tris, 32, 4, 0.1, 16)
    assert np.isin(bad, got).any()


def test_an_infinite_centroid_is_refused(eng):
    """A centroid that overflows float32 has no bucket grid: refused on the host, before any search runs."""
    from isaac_rover_amd import _lib
    verts, tris = _soup(np.random.default_rng(6), 200, (0.0, 0.0), (1.0, 1.0))
    verts[0:3, 0] = 3.0e38
    with pytest.raises(_lib.RoverError, match="not finite"):
        eng.build_knn_map(verts, tris, 4, 4, 0.1, 8)


# ------------------------------------------------------------------------------------------------ the reference's ranking
@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("tables", [False, True])
def test_reference_fp16_ranking_matches_its_restatement(eng, k, tables):
    """ranking="reference_fp16": fp16 centroids, fp16 differences, fp16(sqrt) keys, ties by id — with the default coordinate tables
    and with explicit ones (x off the default grid)."""
    n_x, n_y, res = 24, 20, 0.1
    verts, tris = _soup(np.random.default_rng(k), 2000, (-0.3, -0.3), (2.6, 2.2))
    kw = {}
    if tables:
        kw = dict(cell_x_f16=(np.arange(n_x) * res + 0.013).astype(np.float16), cell_y_f16=(np.arange(n_y) * 0.0996).astype(np.float16))
    _check(eng, verts, tris, n_x, n_y, res, k, ranking="reference_fp16", **kw)
