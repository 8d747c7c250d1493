"""numpy definitions of what the KNN map builder (rover_build_knn_map: csrc/rover_knn.hip `knn_*_kernel`, csrc/rover_capi_scene.cpp
`build_knn_map_impl`) has to compute, every operation rounded to float32 as the kernels round it (the library is built with
-ffp-contract=off, so a product and the sum it feeds round separately).

  brute_force      the two rankings over ALL centroids: the definition the builder's lists are compared with
  bucket_grid      the host's sizing of the bucket grid and `knn_bucket`: used to aim inputs at bucket edges and to pick scan lengths
  ring_search      a CPU model of `knn_select_kernel`'s gather / sort / stop loop (exact_f32 ranking), the stop slack a parameter
  contested_cells  inputs on which a stop test WITHOUT slack returns a wrong list ("KNN stop test")
"""
import types

import numpy as np

f32 = np.float32
KNN_CAP = 8192                    # knn_select_kernel: keys a cell's search can hold
SCAN_TILE = 2048                  # launch_scan_exclusive: counts per workgroup

# The stop slack of the exact_f32 ranking — `KNN_STOP_SLACK` in csrc/rover_knn.hip (knn_select_kernel, "lim = reach - (reach + span) *
# KNN_STOP_SLACK"), the one place besides this line where the value is written.  Derivation: DESIGN.md §4.6.
STOP_SLACK = 2.0 ** -20


# ---------------------------------------------------------------------------------------------------------------------
# definitions
# ---------------------------------------------------------------------------------------------------------------------
def _corners(verts, tris):
    """Vertex rows of every triangle, an index outside [0, V) reading vertex 0 (knn_centroid_kernel)."""
    v = np.asarray(verts, dtype=f32)
    t = np.asarray(tris).astype(np.int64)
    t = np.where((t < 0) | (t >= len(v)), 0, t)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def centroids(verts, tris, ranking="exact_f32"):
    """knn_centroid_kernel -> (cx, cy) float32.  exact_f32: ((a + b) + c) / 3 in float32; reference_fp16: the float64 mean rounded to
    float32, then to fp16 (rover_utils.py:68-72), kept as that fp16 value in float32."""
    a, b, c = _corners(verts, tris)
    if ranking == "exact_f32":
        return (a[:, 0] + b[:, 0] + c[:, 0]) / f32(3), (a[:, 1] + b[:, 1] + c[:, 1]) / f32(3)
    if ranking != "reference_fp16":
        raise ValueError(ranking)
    a, b, c = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    with np.errstate(over="ignore"):
        m = (((a + b) + c) / 3.0).astype(f32).astype(np.float16).astype(f32)
    return m[:, 0], m[:, 1]


def cell_tables(n_x, n_y, res, ranking="exact_f32", cell_x_f16=None, cell_y_f16=None):
    """Cell coordinates as float32: float(i) * res; for the reference ranking the fp16 tables (default fp16(float(i) * res))."""
    px, py = np.arange(n_x, dtype=f32) * f32(res), np.arange(n_y, dtype=f32) * f32(res)
    if ranking == "exact_f32":
        return px, py
    px = px.astype(np.float16) if cell_x_f16 is None else np.asarray(cell_x_f16, dtype=np.float16)
    py = py.astype(np.float16) if cell_y_f16 is None else np.asarray(cell_y_f16, dtype=np.float16)
    return px.astype(f32), py.astype(f32)


def fp16_distances(verts, tris, cell_x, cell_y, i):
    """The reference's distances for map row i (rover_utils.py:68-72,99-100): fp16 centroids (float64 mean -> float -> half),
    fp16(c - p) per axis, norm in f32 rounded to fp16.  Returns [Y, T] fp16."""
    cx, cy = centroids(verts, tris, "reference_fp16")
    return _fp16_row(cx, cy, f32(np.float16(cell_x[i])), np.asarray(cell_y, dtype=np.float16).astype(f32))


def _fp16_row(cx, cy, px, py):
    with np.errstate(over="ignore", invalid="ignore"):
        dx = (cx - px).astype(np.float16).astype(f32)
        dy = (cy[None, :] - py[:, None]).astype(np.float16).astype(f32)
        return np.sqrt(dx[None, :] * dx[None, :] + dy * dy).astype(np.float16)


def row_keys(cx, cy, px, py, ranking="exact_f32"):
    """The 64-bit sort keys of one map row, [Y, T]: (bits of the non-negative float32 key) << 32 | triangle id.  exact_f32: the key is
    d2 = dx dx + dy dy; reference_fp16: fp16(sqrt(d2)) of the fp16-rounded differences.  A NaN key (NaN centroid) ranks after every
    number, infinity included."""
    with np.errstate(over="ignore", invalid="ignore"):
        if ranking == "exact_f32":
            dx = cx - px
            dy = cy[None, :] - py[:, None]
            key = dx[None, :] * dx[None, :] + dy * dy
        else:
            key = _fp16_row(cx, cy, px, py).astype(f32)
    bits = np.where(np.isnan(key), np.uint32(0xffffffff), np.ascontiguousarray(key, dtype=f32).view(np.uint32))
    return (bits.astype(np.uint64) << np.uint64(32)) | np.arange(len(cx), dtype=np.uint64)[None, :]


def brute_force(verts, tris, n_x, n_y, res, k, ranking="exact_f32", cell_x_f16=None, cell_y_f16=None):
    """numpy restatement of rover_utils.py:68-108 with the builder's stated rankings -> [X, Y, K] int32, nearest first, ties by id.
    Every centroid is ranked for every cell; lists are only defined where at least K centroids are not NaN."""
    cx, cy = centroids(verts, tris, ranking)
    px, py = cell_tables(n_x, n_y, res, ranking, cell_x_f16, cell_y_f16)
    out = np.zeros((n_x, n_y, k), np.int32)
    for x in range(n_x):
        key = row_keys(cx, cy, px[x], py, ranking)
        if k < key.shape[1]:
            key = np.partition(key, k - 1, axis=1)[:, :k]
        out[x] = (np.sort(key, axis=1)[:, :k] & np.uint64(0xffffffff)).astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the bucket grid (build_knn_map_impl) and knn_bucket
# ---------------------------------------------------------------------------------------------------------------------
def knn_bucket(v, origin, inv_g, n):
    """knn_bucket: floor((v - origin) * inv_g) in float32, clamped to [0, n - 1]; NaN -> 0."""
    with np.errstate(invalid="ignore"):
        f = (np.asarray(v, dtype=f32) - f32(origin)) * f32(inv_g)
        b = np.where(f > 0, np.minimum(np.floor(f), f32(n - 1)), f32(0))
    return b.astype(np.int64)


def bucket_grid(cx, cy, k, res, attempt=0):
    """The host's sizing: bounding box of the centroids that are not NaN, bucket edge = the radius that holds K/4 centroids at mean
    density, not below res, halved per retry `attempt`; -> namespace x0, y0, x1, y1, g, inv_g (float32), nbx, nby, nb."""
    cx, cy = np.asarray(cx, dtype=f32), np.asarray(cy, dtype=f32)
    fx, fy = cx[~np.isnan(cx)], cy[~np.isnan(cy)]
    x0, x1 = (fx.min(), fx.max()) if len(fx) else (f32(0), f32(0))
    y0, y1 = (fy.min(), fy.max()) if len(fy) else (f32(0), f32(0))
    area = (float(x1) - float(x0) + 1e-6) * (float(y1) - float(y0) + 1e-6)
    gsz = max(float(np.sqrt(area * float(k) / (4.0 * float(len(cx))))), float(f32(res))) * 0.5 ** attempt
    nbx, nby = int((float(x1) - float(x0)) / gsz) + 1, int((float(y1) - float(y0)) / gsz) + 1
    while nbx * nby > 1 << 22:
        gsz *= 2.0
        nbx, nby = int((float(x1) - float(x0)) / gsz) + 1, int((float(y1) - float(y0)) / gsz) + 1
    g = f32(gsz)
    return types.SimpleNamespace(x0=f32(x0), y0=f32(y0), x1=f32(x1), y1=f32(y1), g=g, inv_g=f32(1) / g, nbx=nbx, nby=nby, nb=nbx * nby)


def stop_span(grid, n_x, n_y, res):
    """build_knn_map_impl's `span`: the largest |coordinate - origin| of any centroid or cell point, as float32."""
    ex, ey = float(f32(n_x - 1) * f32(res)), float(f32(n_y - 1) * f32(res))
    x0, y0 = float(grid.x0), float(grid.y0)
    return f32(max(float(grid.x1) - x0, float(grid.y1) - y0, abs(x0), abs(ex - x0), abs(y0), abs(ey - y0)))


def stop_limit(r, g, span, slack):
    """knn_select_kernel: the squared distance up to which ring r settles a K-th key, in the kernel's float32 operations."""
    reach = np.asarray(r, dtype=f32) * np.asarray(g, dtype=f32)
    lim = reach - (reach + np.asarray(span, dtype=f32)) * f32(slack)
    return np.where(lim > 0, lim * lim, f32(-1))              # lim <= 0: no key passes, the next ring is gathered


def ring_search(cx, cy, n_x, n_y, res, k, slack=STOP_SLACK, cells=None, attempts=1):
    """CPU model of knn_select_kernel, exact_f32 ranking: per cell gather the buckets at Chebyshev distance <= r, sort, stop when
    the K-th key is within stop_limit(r) or the rings cover the grid.  -> [X, Y, K] int32 (only `cells`, if given, are filled).
    slack = 0 is the stop test `kth <= (r g)^2`.  A ring of more than KNN_CAP candidates raises OverflowError once `attempts` grids,
    each of half the bucket edge of the one before, have been tried (the host tries 6)."""
    for attempt in range(attempts):
        try:
            return _ring_search(np.asarray(cx, dtype=f32), np.asarray(cy, dtype=f32), n_x, n_y, res, k, slack, cells, attempt)
        except OverflowError:
            if attempt == attempts - 1:
                raise


def _ring_search(cx, cy, n_x, n_y, res, k, slack, cells, attempt):
    grid = bucket_grid(cx, cy, k, res, attempt)
    span = stop_span(grid, n_x, n_y, res)
    bi, bj = knn_bucket(cx, grid.x0, grid.inv_g, grid.nbx), knn_bucket(cy, grid.y0, grid.inv_g, grid.nby)
    px, py = cell_tables(n_x, n_y, res)
    out = np.zeros((n_x, n_y, k), np.int32)
    for x, y in (cells if cells is not None else [(x, y) for x in range(n_x) for y in range(n_y)]):
        bx, by = int(knn_bucket(px[x], grid.x0, grid.inv_g, grid.nbx)), int(knn_bucket(py[y], grid.y0, grid.inv_g, grid.nby))
        ring = np.maximum(np.abs(bi - bx), np.abs(bj - by))
        keys = row_keys(cx, cy, px[x], py[y:y + 1])[0]
        for r in range(max(grid.nbx, grid.nby) + 1):
            got = np.sort(keys[ring <= r])
            if len(got) > KNN_CAP:
                raise OverflowError(f"cell ({x}, {y}): ring {r} holds {len(got)} candidates")
            covers_all = bx - r <= 0 and by - r <= 0 and bx + r >= grid.nbx - 1 and by + r >= grid.nby - 1
            if len(got) < k and not covers_all:
                continue
            kth = np.uint32(got[k - 1] >> np.uint64(32)).view(f32) if len(got) >= k else f32(np.inf)
            if covers_all or kth <= stop_limit(r, grid.g, span, slack):       # (a NaN key compares false: the search goes on)
                n = min(k, len(got))
                out[x, y, :n] = (got[:n] & np.uint64(0xffffffff)).astype(np.int32)
                break
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def mesh_of_sums(sx, sy):
    """A mesh whose triangle t has the float32 centroid (sx[t] / 3, sy[t] / 3) exactly as knn_centroid_kernel computes it: vertex 0 is
    the origin, triangle t = (t + 1, 0, 0), so the sum (a + b) + c is the float32 sx[t] itself.  (Not every float32 is such a
    quotient: inputs are aimed by stepping the SUM through neighbouring floats.)"""
    sx, sy = np.asarray(sx, dtype=f32), np.asarray(sy, dtype=f32)
    verts = np.zeros((len(sx) + 1, 3), f32)
    verts[1:, 0], verts[1:, 1] = sx, sy
    tris = np.zeros((len(sx), 3), np.int32)
    tris[:, 0] = np.arange(1, len(sx) + 1)
    return verts, tris


def _ulp_steps(v, lo, hi):
    """The floats from lo to hi steps (in ulps) around the float32 v, ascending (v away from 0 and from a binade's end)."""
    return (np.asarray(v, dtype=f32).view(np.int32) + np.arange(lo, hi + 1, dtype=np.int32) * (1 if v > 0 else -1)).view(f32)


def _sum_for(c):
    """The float32 vertex sum whose third is nearest to c (c itself for three floats in four)."""
    s = _ulp_steps(f32(3) * f32(c), -3, 3)
    return s[np.argmin(np.abs((s / f32(3)).astype(np.float64) - float(c)))]


def _d2(cxv, cyv, px, py):
    dx, dy = f32(cxv) - f32(px), f32(cyv) - f32(py)
    return dx * dx + dy * dy


def _axis_hazards(origin, g, inv_g, n, pts):
    """For each cell coordinate p of `pts`: (r, sum) of a centroid coordinate c = sum / 3 within a few ulps of p +- r g whose bucket
    lies r + 1 or more away from p's while fl((c - p)^2) < fl((r g)^2); None where there is none for r in 1..3."""
    found = []
    for p in pts:
        bp = int(knn_bucket(p, origin, inv_g, n))
        hit = None
        for r in (1, 2, 3):
            reach = f32(r) * g
            for sgn in (1.0, -1.0):
                s = _ulp_steps(f32(3) * (p + f32(sgn) * reach), -12, 12)
                s = s[s != 0]
                c = s / f32(3)
                b = knn_bucket(c, origin, inv_g, n)
                d = c - p
                ok = (np.abs(b - bp) >= r + 1) & (d * d < reach * reach) & (c > origin) & (b < n - 1)
                if ok.any() and hit is None:
                    j = np.nonzero(ok)[0]
                    hit = (r, s[j[np.argmin((d * d)[j])]])           # the deepest one: leaves the widest window for the K-th key
        found.append(hit)
    return found


def contested_cells(x0, span, res, k=2, t=4096, n_x=40, n_y=40, y0=None, span_y=None, spacing=8):
    """Centroids on which the ring search stops too early when its stop test has no slack.

    The bounding box of the centroids is [x0, x0 + span] x [y0, y0 + span_y] (y defaults to x), pinned by two corner triangles.  For a
    cell (x, y) whose point has, along one axis, a centroid coordinate within ulps of p +- r g that the float32 bucket arithmetic puts
    r + 1 buckets away although its squared distance is below (r g)^2, the input holds: that centroid U (not gathered by ring r); the
    cell's own centroid and k - 2 more next to it; and a K-th candidate near (-0.6, +0.8) r g — inside ring r — moved by up to
    +-40 ulps per coordinate of its vertex sum until d2(U) < d2 <= (r g)^2.  Ring r then holds K keys whose K-th passes `kth <= (r g)^2`,
    and U, nearer than that K-th, is missed.  Chosen cells lie `spacing` cells apart so that no cell sees its neighbour's centroids
    inside its 3-ring reach.  A clump in the far corner pads the mesh to `t` triangles so that the sizing gives g = res.

    -> (verts, tris, corner triangle ids, [(x, y, r, id of U), ...]); the caller checks `bucket_grid(...).g == res`."""
    y0 = x0 if y0 is None else y0
    span_y = span if span_y is None else span_y
    g = f32(res)
    inv_g = f32(1) / g
    corner = [_sum_for(x0), _sum_for(y0), _sum_for(x0 + span), _sum_for(y0 + span_y)]                # vertex sums of the two corner triangles
    ox, oy, x1, y1 = (c / f32(3) for c in corner)
    nbx, nby = int((float(x1) - float(ox)) / float(g)) + 1, int((float(y1) - float(oy)) / float(g)) + 1
    px, py = cell_tables(n_x, n_y, res)
    # cells more than 4 buckets inside the box and, in x, clear of the clump
    xs = [i for i in range(n_x) if ox + f32(0.45) < px[i] < x1 - f32(1.2)]
    ys = [j for j in range(n_y) if oy + f32(0.45) < py[j] < y1 - f32(0.45)]
    hx = dict(zip(xs, _axis_hazards(ox, g, inv_g, nbx, px[xs])))
    hy = dict(zip(ys, _axis_hazards(oy, g, inv_g, nby, py[ys])))
    sx, sy, cells = [float(corner[0]), float(corner[2])], [float(corner[1]), float(corner[3])], []
    taken = []
    for i in xs:
        for j in ys:
            if any(abs(i - a) < spacing and abs(j - b) < spacing for a, b in taken):
                continue
            along_x = hx[i] is not None
            hit = hx[i] if along_x else hy[j]
            if hit is None:
                continue
            r, s_u = hit
            p, q = px[i], py[j]
            ux, uy = (s_u, f32(3) * q) if along_x else (f32(3) * p, s_u)
            d2_u = _d2(ux / f32(3), uy / f32(3), p, q)
            reach = f32(r) * g
            sgn = f32(1.0 if (ux / f32(3) - p if along_x else uy / f32(3) - q) > 0 else -1.0)
            # K-th candidate: away from U along its axis, 0.8 r g up the other one
            off_a, off_b = -sgn * f32(0.6) * reach, f32(0.8) * reach
            kx, ky = (p + off_a, q + off_b) if along_x else (p + off_b, q + off_a)
            ax, ay = _ulp_steps(f32(3) * kx, -40, 40), _ulp_steps(f32(3) * ky, -40, 40)
            cxk, cyk = (ax / f32(3))[:, None], (ay / f32(3))[None, :]
            dxk, dyk = cxk - p, cyk - q
            d2_k = dxk * dxk + dyk * dyk
            bxk = np.abs(knn_bucket(cxk, ox, inv_g, nbx) - int(knn_bucket(p, ox, inv_g, nbx)))
            byk = np.abs(knn_bucket(cyk, oy, inv_g, nby) - int(knn_bucket(q, oy, inv_g, nby)))
            ok = (d2_k > d2_u) & (d2_k <= reach * reach) & (bxk <= r) & (byk <= r)
            if not ok.any():
                continue
            a, b = np.argwhere(ok)[0]
            taken.append((i, j))
            cells.append((i, j, r, len(sx)))
            sx += [float(ux), float(ax[a])]
            sy += [float(uy), float(ay[b])]
            for m in range(k - 1):                                   # the cell's own centroid and k - 2 more within 4 mm of it
                sx.append(3.0 * (float(p) + 0.002 * m))
                sy.append(3.0 * (float(q) - 0.002 * m))
    n_fill = t - len(sx)
    if n_fill < 0:
        raise ValueError("t is too small for the contested cells")
    rng = np.random.default_rng(len(cells))
    sx += list(3.0 * (x0 + span - 0.05 - 0.3 * rng.random(n_fill)))
    sy += list(3.0 * (y0 + span_y - 0.05 - 0.3 * rng.random(n_fill)))
    verts, tris = mesh_of_sums(sx, sy)
    grid = bucket_grid(*centroids(verts, tris), k, res)
    assert (grid.g, grid.x0, grid.y0, grid.nbx, grid.nby) == (g, ox, oy, nbx, nby), "the sizing did not give the grid the inputs were aimed at"
    return verts, tris, np.array([0, 1]), cells


def shuffle_ids(tris, seed):
    """The same triangles in a shuffled order -> (tris, perm) with tris_new[i] = tris[perm[i]]."""
    perm = np.random.default_rng(seed).permutation(len(tris))
    return np.ascontiguousarray(np.asarray(tris)[perm]), perm
