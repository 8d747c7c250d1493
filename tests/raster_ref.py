"""The definition of rover_build_heightfield (include/rover_step.h) restated with numpy int64 / float64: what the HIP
rasteriser must reproduce bit for bit.  It is this project's own definition, like the motion model.

Every numpy operation below is one IEEE rounding (numpy does not fuse a multiply with an add), int64 -> float64 is exact for the values
that occur (|w| <= 2^53), and float64 -> float32 rounds to nearest even.  The box a triangle is tested on is its bounding box widened by
a node on every side — a superset on purpose: coverage is decided by the edge functions alone, not by how the box was rounded.
"""
import numpy as np

SUB = 256                    # sub-units per node spacing
MAX_SNAP = 1 << 25           # largest |X|, |Y| of a snapped vertex
MAX_NODES = 131072


def snap_vertices(vertices, horizontal_scale, shift):
    """-> (X [V] int64, Y [V] int64, z [V] float64, ok [V] bool): step 2 and the per-vertex part of step 3."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    hs = np.float64(np.float32(horizontal_scale))
    sx, sy = np.float64(np.float32(shift[0])), np.float64(np.float32(shift[1]))
    with np.errstate(all="ignore"):
        x = np.rint(((v[:, 0].astype(np.float64) - sx) / hs) * 256.0)
        y = np.rint(((v[:, 1].astype(np.float64) - sy) / hs) * 256.0)
        ok = np.isfinite(v).all(axis=1) & (np.abs(x) <= MAX_SNAP) & (np.abs(y) <= MAX_SNAP)
    return np.where(ok, x, 0.0).astype(np.int64), np.where(ok, y, 0.0).astype(np.int64), v[:, 2].astype(np.float64), ok


def height_key(z32):
    """The order-preserving uint32 key of float32 values: larger value <=> larger key, -0 below +0, never 0."""
    b = np.ascontiguousarray(z32, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_height(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def build_heightfield(vertices, triangles, n0, n1, horizontal_scale=0.025, shift=(0.0, 0.0), fill=0.0, return_count=False):
    """-> (hm [n0, n1] float32, uncovered, skipped) [, count [n0, n1] int32: how many triangles cover each node, on_edge [n0, n1] bool:
    the node lies exactly on an edge or a vertex of a triangle that covers it]."""
    X, Y, Z, ok = snap_vertices(vertices, horizontal_scale, shift)
    tris = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    n_v = len(X)
    keys = np.zeros((n0, n1), dtype=np.uint32)
    count = np.zeros((n0, n1), dtype=np.int32) if return_count else None
    on_edge = np.zeros((n0, n1), dtype=bool) if return_count else None
    skipped = 0
    in_range = ((tris >= 0) & (tris < n_v)).all(axis=1)
    for t in range(len(tris)):
        if not in_range[t] or not ok[tris[t]].all():
            skipped += 1
            continue
        ia, ib, ic = (int(i) for i in tris[t])
        ax, ay, bx, by, cx, cy = int(X[ia]), int(Y[ia]), int(X[ib]), int(Y[ib]), int(X[ic]), int(Y[ic])
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area == 0:
            continue
        sgn = 1 if area > 0 else -1
        i_lo, i_hi = max(min(ax, bx, cx) // SUB - 1, 0), min(max(ax, bx, cx) // SUB + 2, n0 - 1)
        j_lo, j_hi = max(min(ay, by, cy) // SUB - 1, 0), min(max(ay, by, cy) // SUB + 2, n1 - 1)
        if i_lo > i_hi or j_lo > j_hi:
            continue
        px = (np.arange(i_lo, i_hi + 1, dtype=np.int64) * SUB)[:, None]
        py = (np.arange(j_lo, j_hi + 1, dtype=np.int64) * SUB)[None, :]
        wa = ((cx - bx) * (py - by) - (cy - by) * (px - bx)) * sgn
        wb = ((ax - cx) * (py - cy) - (ay - cy) * (px - cx)) * sgn
        wc = ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) * sgn
        cov = (wa >= 0) & (wb >= 0) & (wc >= 0)
        if not cov.any():
            continue
        with np.errstate(over="ignore"):
            z = ((wa.astype(np.float64) * Z[ia] + wb.astype(np.float64) * Z[ib]) + wc.astype(np.float64) * Z[ic]) / np.float64(area * sgn)
            k = np.where(cov, height_key(z.astype(np.float32)), np.uint32(0))
        sub = keys[i_lo:i_hi + 1, j_lo:j_hi + 1]
        np.maximum(sub, k, out=sub)
        if return_count:
            count[i_lo:i_hi + 1, j_lo:j_hi + 1] += cov
            on_edge[i_lo:i_hi + 1, j_lo:j_hi + 1] |= cov & ((wa == 0) | (wb == 0) | (wc == 0))
    empty = keys == 0
    hm = np.where(empty, np.float32(fill), key_height(keys)).astype(np.float32)
    out = (hm, int(empty.sum()), skipped)
    return out + (count, on_edge) if return_count else out
