"""rover_build_heightfield without a GPU: the binding, the argument checks (all made before the ctx is looked at), the definition
(tests/raster_ref.py) against exact float64 geometry, stones_from_mesh, and the file layout of tools/build_scene.py."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import heightfield_cases as cases  # noqa: E402
import raster_ref  # noqa: E402

from isaac_rover_amd import _lib, assets, synth  # noqa: E402


def test_symbols_are_bound_and_exported():
    for name in ("rover_build_heightfield", "rover_heightfield_limits"):
        assert name in _lib.SYMBOLS
    _lib.build()
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rover_build_heightfield", "rover_heightfield_limits"} <= exported
    lim = _lib.heightfield_limits()
    assert lim["small_nodes"] >= 1 and lim["tile_i"] >= 1 and lim["tile_j"] >= 1 and lim["group_lanes"] in (1, 2, 4, 8, 16, 32, 64)
    assert lib.rover_heightfield_limits(None) == -1


def _call(lib, **kw):
    v = np.zeros((3, 3), dtype=np.float32)
    t = np.zeros((1, 3), dtype=np.int32)
    a = dict(vertices=v.ctypes.data, V=3, triangles=t.ctypes.data, T=1, N0=4, N1=4, hs=0.025, sx=0.0, sy=0.0, fill=0.0, hm=16)
    a.update(kw)
    rc = lib.rover_build_heightfield(None, a["vertices"], a["V"], a["triangles"], a["T"], a["N0"], a["N1"], a["hs"], a["sx"], a["sy"], a["fill"],
                                     a["hm"], None)
    return rc, lib.rover_last_error(None).decode()


@pytest.mark.parametrize("kw", [dict(N0=0), dict(N1=0), dict(N0=-3), dict(N0=131073), dict(N1=131073), dict(hs=0.0), dict(hs=-0.025),
                                dict(hs=float("inf")), dict(hs=float("nan")), dict(sx=float("nan")), dict(sy=float("inf")), dict(V=-1),
                                dict(T=-1), dict(vertices=None), dict(triangles=None), dict(hm=None)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_arguments_with_a_null_ctx(kw):
    """Every ROVER_E_INVALID of the argument list is reported before the ctx is looked at: a NULL ctx, no device, and a message that
    names the argument and not the ctx."""
    lib = _lib.load()
    rc, msg = _call(lib, **kw)
    assert rc == -1
    assert msg.startswith("build_heightfield:") and "null ctx" not in msg, msg


def test_valid_arguments_reach_the_ctx_check():
    lib = _lib.load()
    for kw in (dict(), dict(N0=131072, N1=1), dict(V=0, vertices=None, T=0, triangles=None)):
        rc, msg = _call(lib, **kw)
        assert rc == -1 and "null ctx" in msg, msg


# ---- the definition against exact geometry ----------------------------------------------------------------------------------------------
def _exact_reference(verts, tris, n0, n1, hs, shift):
    """Unsnapped float64 geometry.  -> z_exact [n0, n1] (max plane value over the triangles that contain the node with all three distances
    > eps), slope [n0, n1] (steepest such triangle), left_out [n0, n1] (the node is within eps = 2 hs / 256 of an edge line of a triangle
    that covers or nearly covers it), covered [n0, n1]."""
    v = verts.astype(np.float64)
    xs, ys = cases.node_positions(n0, n1, hs, shift)
    px, py = np.meshgrid(xs, ys, indexing="ij")
    eps = 2.0 * float(np.float32(hs)) / 256.0
    z_exact = np.full((n0, n1), -np.inf)
    slope = np.zeros((n0, n1))
    left_out = np.zeros((n0, n1), dtype=bool)
    covered = np.zeros((n0, n1), dtype=bool)
    for ia, ib, ic in tris:
        a, b, c = v[ia], v[ib], v[ic]
        area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area == 0.0:
            continue
        if area < 0.0:
            b, c, area = c, b, -area
        i0, i1 = np.searchsorted(xs, min(a[0], b[0], c[0]) - 2 * eps), np.searchsorted(xs, max(a[0], b[0], c[0]) + 2 * eps)
        j0, j1 = np.searchsorted(ys, min(a[1], b[1], c[1]) - 2 * eps), np.searchsorted(ys, max(a[1], b[1], c[1]) + 2 * eps)
        if i0 >= i1 or j0 >= j1:
            continue
        qx, qy = px[i0:i1, j0:j1], py[i0:i1, j0:j1]
        d, w = [], []
        for p, q in ((b, c), (c, a), (a, b)):                       # signed distance to each edge line, positive inside
            e = (q[0] - p[0]) * (qy - p[1]) - (q[1] - p[1]) * (qx - p[0])
            w.append(e / area)
            d.append(e / np.hypot(q[0] - p[0], q[1] - p[1]))
        dmin = np.minimum(np.minimum(d[0], d[1]), d[2])
        near = (dmin >= -eps) & (dmin <= eps)
        inside = dmin > eps
        z = w[0] * a[2] + w[1] * b[2] + w[2] * c[2]
        # gradient of the plane through a, b, c
        gx = ((b[2] - a[2]) * (c[1] - a[1]) - (c[2] - a[2]) * (b[1] - a[1])) / area
        gy = ((c[2] - a[2]) * (b[0] - a[0]) - (b[2] - a[2]) * (c[0] - a[0])) / area
        g = float(np.hypot(gx, gy))
        left_out[i0:i1, j0:j1] |= near
        covered[i0:i1, j0:j1] |= inside
        z_exact[i0:i1, j0:j1] = np.where(inside, np.maximum(z_exact[i0:i1, j0:j1], z), z_exact[i0:i1, j0:j1])
        slope[i0:i1, j0:j1] = np.where(inside, np.maximum(slope[i0:i1, j0:j1], g), slope[i0:i1, j0:j1])
    return z_exact, slope, left_out, covered


def test_definition_against_exact_geometry():
    """raster_ref on the Delaunay case (seed 7).  Snapping moves a vertex by <= hs / 512 per axis; inside the snapped triangle the new
    plane's value at a fixed point p is the old plane's value at p - sum(lambda_i delta_i), a convex combination of the vertex shifts, so
    |z - z_exact| <= g hs sqrt(2) / 512 + 4 ulp_f32(z), g the steepest slope among the covering triangles.  Measured with this seed:
    1.97 % of the nodes left out (limit 5 %), largest error 0.937 of the bound, no violation."""
    verts, tris, picks = cases.delaunay_case()
    n0, n1, hs, shift = cases.DELAUNAY_N0, cases.DELAUNAY_N1, cases.DELAUNAY_HS, cases.DELAUNAY_SHIFT
    assert 650 <= len(verts) <= 750
    hm, uncovered, skipped, count, on_edge = raster_ref.build_heightfield(verts, tris, n0, n1, hs, shift, fill=-9.0, return_count=True)
    assert uncovered == 0 and skipped == 0 and int(count.min()) >= 1
    # watertight and inclusive: a node on a shared edge or a vertex belongs to every triangle that meets it there
    assert int(on_edge.sum()) >= 40 and bool(on_edge.reshape(-1)[picks].all())
    assert bool((count[on_edge] >= 2).all())
    assert bool((count.reshape(-1)[picks] >= 3).all())
    z_exact, slope, left_out, covered = _exact_reference(verts, tris, n0, n1, hs, shift)
    keep = ~left_out
    frac = float(left_out.mean())
    assert bool(covered[keep].all())
    hs64 = float(np.float32(hs))
    ulp = np.spacing(np.abs(hm).astype(np.float32)).astype(np.float64)
    bound = slope * hs64 * np.sqrt(2.0) / 512.0 + 4.0 * ulp
    err = np.abs(hm.astype(np.float64) - z_exact)
    worst = float((err[keep] / bound[keep]).max())
    print(f"left out {frac:.4f}, largest error / bound {worst:.3f}")
    assert frac <= 0.05
    assert bool((err[keep] <= bound[keep]).all()), worst
    assert bool((count[keep] == 1).all())                          # away from the edges a Delaunay mesh covers a node once


def test_a_planar_mesh_returns_its_plane():
    """Vertices on the sub-unit lattice and a plane with dyadic coefficients: every product, sum and the division are exact, so the
    result is the plane's value at every node, to the bit; both windings."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(3)
    hs, shift, n0, n1 = 0.25, (-1.0, 0.5), 21, 17
    sub = np.concatenate([rng.integers(-600, 21 * 256 + 600, (60, 2)), [[-700, -700], [-700, 6000], [6500, -700], [6500, 6000]]])
    xy = sub / 1024.0 + np.array(shift)                            # (X / 256) hs + shift, exact in float32
    z = 0.5 * xy[:, 0] - 0.25 * xy[:, 1] + 1.0
    verts = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
    assert np.array_equal(verts.astype(np.float64), np.concatenate([xy, z[:, None]], axis=1))
    tris = Delaunay(sub).simplices.astype(np.int32)
    tris[::2] = tris[::2][:, ::-1]
    hm, uncovered, skipped = raster_ref.build_heightfield(verts, tris, n0, n1, hs, shift)
    xs, ys = cases.node_positions(n0, n1, hs, shift)
    want = (0.5 * xs[:, None] - 0.25 * ys[None, :] + 1.0).astype(np.float32)
    assert uncovered == 0 and skipped == 0
    assert np.array_equal(hm.view(np.uint32), want.view(np.uint32))


def test_ref_keys_order_like_the_values():
    z = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], dtype=np.float32)
    k = raster_ref.height_key(z)
    assert bool((np.diff(k.astype(np.int64)) > 0).all()) and int(k.min()) > 0
    assert np.array_equal(raster_ref.key_height(k).view(np.uint32), z.view(np.uint32))


# ---- stones -------------------------------------------------------------------------------------------------------------------------------
def test_stones_from_mesh():
    """Three separated pyramids, the middle one built from duplicated vertices (its triangles share coordinates, not indices): three rows
    with the known centres, widths and heights, sorted by (x, y); read_stone_info's radius is half the larger footprint width."""
    a = cases.pyramid(5.0, 1.0, 0.25, 0.5, 1.0, 0.75)
    b = cases.pyramid(2.0, 3.0, -0.5, 1.5, 0.5, 0.25, duplicated=True)
    c = cases.pyramid(2.0, 1.0, 0.0, 0.25, 0.25, 1.0)
    verts, tris = cases.merge([a, b, c])
    rows = assets.stones_from_mesh(verts, tris)
    assert rows.dtype == np.float64 and rows.shape == (3, 6)
    want = np.array([[2.0, 1.0, 0.0, 0.5, 0.5, 1.0], [2.0, 3.0, -0.5, 3.0, 1.0, 0.25], [5.0, 1.0, 0.25, 1.0, 2.0, 0.75]])
    assert np.array_equal(rows, want)
    info = synth.read_stone_info_array(rows)
    assert np.array_equal(info[:, 6], np.array([0.125, 0.75, 0.5], dtype=np.float32))
    # the order of the tables does not matter, an unused vertex and an out-of-range triangle make no stone
    perm = np.random.default_rng(0).permutation(len(tris))
    v2 = np.concatenate([verts, [[9.0, 9.0, 9.0]]]).astype(np.float32)
    t2 = np.concatenate([tris[perm], [[0, 1, 99]]]).astype(np.int32)
    assert np.array_equal(assets.stones_from_mesh(v2, t2), want)
    assert assets.stones_from_mesh(verts, np.zeros((0, 3), dtype=np.int32)).shape == (0, 6)


# ---- tools/build_scene.py ---------------------------------------------------------------------------------------------------------------
class _HostEngine:
    """Stands in for the two Engine calls of assets.build_scene_from_meshes with the host definitions of what they compute."""

    def build_knn_map(self, vertices, triangles, n_x, n_y, res=0.1, k=200, ranking="exact_f32", cell_x_f16=None, cell_y_f16=None):
        return synth.knn_map_bruteforce(np.asarray(vertices), np.asarray(triangles), n_x, n_y, k, res)

    def build_heightfield(self, vertices, triangles, n0, n1, horizontal_scale=0.025, shift=(0.0, 0.0), fill=0.0):
        hm, uncovered, skipped = raster_ref.build_heightfield(vertices, triangles, n0, n1, horizontal_scale, shift, fill)
        return torch.from_numpy(hm), uncovered, skipped


def test_build_scene_files_round_trip(tmp_path, capsys):
    spec = synth.IrregularSpec(extent_x=2.4, extent_y=2.4, n_rocks=3, seed=2, coarse=0.6, fine=0.075, n_dup=4, n_degenerate=2)
    verts, tris, rock_tris, _ = synth.irregular_mesh(spec)
    root = tmp_path / "assets"
    d = root / "tasks" / "utils" / "terrain"
    d.mkdir(parents=True)
    assets.save_ply(str(d / "map.ply"), verts, tris)
    assets.save_ply(str(d / "big_stones.ply"), verts, rock_tris)
    v2, t2 = assets.load_ply(str(d / "map.ply"))
    assert np.array_equal(v2, verts) and np.array_equal(t2, tris)
    sp = importlib.util.spec_from_file_location("build_scene_tool", os.path.join(ROOT, "tools", "build_scene.py"))
    tool = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(tool)
    assert tool.main([str(d), "--cells", "24", "--k", "8", "--hscale", "0.05"], make_engine=_HostEngine) == 0
    out = capsys.readouterr().out
    assert "0 uncovered" in out and "triangles skipped" in out
    for name in ("knn_terrain/map_indices.pt", "knn_terrain/triangles.pt", "knn_terrain/vertices.pt", "knn_rocks/map_indices.pt",
                 "heightmap_tensor.pt", "stone_info.npy"):
        assert (d / name).exists(), name
    scene = assets.load_reference_assets(str(root), horizontal_scale=0.05)
    assert tuple(scene.terrain.map_indices.shape) == (24, 24, 8) and tuple(scene.rocks.map_indices.shape) == (24, 24, 8)
    assert scene.terrain.vertices.dtype == torch.float16 and scene.vertical_scale == 1.0
    assert tuple(scene.heightmap.shape) == (48, 48) and scene.heightmap.dtype == torch.float32
    # the heightfield is that of the fp16-rounded vertices: the surface the rays hit
    v16 = torch.from_numpy(verts).to(torch.float16).to(torch.float32).numpy()
    want, uncovered, _ = raster_ref.build_heightfield(v16, tris, 48, 48, 0.05, (0.0, 0.0), fill=float(v16[:, 2].min()))
    assert uncovered == 0
    assert np.array_equal(scene.heightmap.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(scene.stone_info_raw, assets.stones_from_mesh(verts, rock_tris))
    assert 1 <= len(scene.stone_info_raw) <= 3 and synth.read_stone_info_array(scene.stone_info_raw).shape[1] == 7
