"""Meshes shared by the heightfield tests (test_heightfield_host.py, test_heightfield_gpu.py)."""
import numpy as np

DELAUNAY_N0, DELAUNAY_N1 = 96, 80
DELAUNAY_HS = 0.025
DELAUNAY_SHIFT = (-0.3, 0.2)
DELAUNAY_SEED = 7


def node_positions(n0, n1, hs, shift):
    """World (x [n0], y [n1]) of the nodes in float64, from the float32 arguments the library gets."""
    hs64, sx, sy = np.float64(np.float32(hs)), np.float64(np.float32(shift[0])), np.float64(np.float32(shift[1]))
    return sx + np.arange(n0, dtype=np.float64) * hs64, sy + np.arange(n1, dtype=np.float64) * hs64


def delaunay_case(seed=DELAUNAY_SEED):
    """A Delaunay mesh of ~700 random points that reaches 0.2 - 0.3 m beyond the 96 x 80 grid on every side; 40 of the points lie exactly
    on nodes, half the triangles have flipped winding, z is rough.  -> (vertices [V,3] float32, triangles [T,3] int32, the flat node indices i * n1 + j of those 40 points)."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    xs, ys = node_positions(DELAUNAY_N0, DELAUNAY_N1, DELAUNAY_HS, DELAUNAY_SHIFT)
    x0, x1, y0, y1 = xs[0] - 0.2, xs[-1] + 0.2, ys[0] - 0.2, ys[-1] + 0.2
    inner = np.stack((rng.uniform(x0, x1, 620), rng.uniform(y0, y1, 620)), axis=1)
    # the frame between 0.2 and 0.3 m outside the grid: the hull encloses the grid with room to spare
    m = 12
    t = np.linspace(0.0, 1.0, m, endpoint=False)
    out = rng.uniform(0.2, 0.3, (4, m))
    frame = np.concatenate([np.stack((xs[0] - out[0], ys[0] - 0.25 + t * (ys[-1] - ys[0] + 0.5)), 1),
                            np.stack((xs[-1] + out[1], ys[0] - 0.25 + t * (ys[-1] - ys[0] + 0.5)), 1),
                            np.stack((xs[0] - 0.25 + t * (xs[-1] - xs[0] + 0.5), ys[0] - out[2]), 1),
                            np.stack((xs[0] - 0.25 + t * (xs[-1] - xs[0] + 0.5), ys[-1] + out[3]), 1),
                            np.array([[xs[0] - 0.3, ys[0] - 0.3], [xs[0] - 0.3, ys[-1] + 0.3], [xs[-1] + 0.3, ys[0] - 0.3], [xs[-1] + 0.3, ys[-1] + 0.3]])])
    picks = rng.choice(DELAUNAY_N0 * DELAUNAY_N1, 40, replace=False)
    on_nodes = np.stack((xs[picks // DELAUNAY_N1], ys[picks % DELAUNAY_N1]), axis=1)
    p2 = np.concatenate([inner, frame, on_nodes]).astype(np.float32)          # the mesh IS its float32 coordinates
    z = rng.uniform(-0.4, 0.4, len(p2)).astype(np.float32)
    tris = Delaunay(p2.astype(np.float64)).simplices.astype(np.int32)
    flip = rng.random(len(tris)) < 0.5
    tris[flip] = tris[flip][:, ::-1]
    return np.concatenate([p2, z[:, None]], axis=1).astype(np.float32), np.ascontiguousarray(tris), picks


def pyramid(cx, cy, z0, wx, wy, h, duplicated=False):
    """Four side triangles of a pyramid with a wx x wy base at height z0 and its apex h above the centre."""
    base = np.array([[cx - wx / 2, cy - wy / 2, z0], [cx + wx / 2, cy - wy / 2, z0], [cx + wx / 2, cy + wy / 2, z0], [cx - wx / 2, cy + wy / 2, z0]])
    apex = np.array([cx, cy, z0 + h])
    if not duplicated:
        return np.concatenate([base, apex[None]]).astype(np.float32), np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], dtype=np.int32)
    v = np.concatenate([np.stack((base[k], base[(k + 1) % 4], apex)) for k in range(4)])      # every triangle with vertices of its own
    return v.astype(np.float32), np.arange(12, dtype=np.int32).reshape(4, 3)


def merge(meshes):
    """One mesh from (vertices, triangles) pairs."""
    vs, ts, base = [], [], 0
    for v, t in meshes:
        vs.append(np.asarray(v, dtype=np.float32))
        ts.append(np.asarray(t, dtype=np.int32) + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32)
