"""GPU: rover_build_heightfield (csrc/rover_raster.hip) against the numpy restatement of its definition (tests/raster_ref.py), bit for bit
and with equal stats: both routes of the kernel on either side of every size of rover_heightfield_limits, clipping, nodes exactly on
edges and vertices, layers, signed zeros, triangles that must not contribute, holes, skipped triangles, grid shapes, device and host
inputs, and a whole scene built from two meshes (assets.build_scene_from_meshes) under set_scene, sample_height and the terrain sim."""
import numpy as np
import pytest
import torch

import heightfield_cases as cases
import raster_ref

from isaac_rover_amd import _lib, assets, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(1, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def delaunay():
    verts, tris, _ = cases.delaunay_case()
    return verts, tris


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(eng, verts, tris, n0, n1, hs=0.025, shift=(0.0, 0.0), fill=-7.5, want=None):
    """One call against the restatement: the same bits, the same stats.  -> (hm as numpy, uncovered, skipped)."""
    if want is None:
        want = raster_ref.build_heightfield(verts, tris, n0, n1, hs, shift, fill)
    hm, uncovered, skipped = eng.build_heightfield(verts, tris, n0, n1, hs, shift, fill)
    assert tuple(hm.shape) == (n0, n1) and hm.dtype == torch.float32 and hm.is_cuda
    got = hm.cpu().numpy()
    diff = np.argwhere(bits(got) != bits(want[0]))
    assert len(diff) == 0, f"{len(diff)} nodes differ, first {diff[0]}: {got[tuple(diff[0])]!r} != {want[0][tuple(diff[0])]!r}"
    assert (uncovered, skipped) == (want[1], want[2])
    return got, uncovered, skipped


def box_nodes(verts, n0, n1, hs, shift):
    """The nodes of a triangle's bounding box, clipped to the grid — what rover_heightfield_limits' sizes refer to: (i0, i1, j0, j1)."""
    X, Y, _, ok = raster_ref.snap_vertices(verts, hs, shift)
    assert ok.all()
    return (max(-(-int(X.min()) // 256), 0), min(int(X.max()) // 256, n0 - 1), max(-(-int(Y.min()) // 256), 0), min(int(Y.max()) // 256, n1 - 1))


def box_triangle(i0, j0, h, w, hs, flip=False):
    """A right triangle (shift 0) whose bounding box holds exactly the nodes [i0, i0 + h) x [j0, j0 + w); its hypotenuse crosses the box."""
    lo_x, hi_x, lo_y, hi_y = (i0 - 0.3) * hs, (i0 + h - 1 + 0.3) * hs, (j0 - 0.3) * hs, (j0 + w - 1 + 0.3) * hs
    v = np.array([[lo_x, lo_y, 0.25], [hi_x, lo_y, -0.5], [lo_x, hi_y, 1.0]], dtype=np.float32)
    return v, np.array([[0, 2, 1] if flip else [0, 1, 2]], dtype=np.int32)


def test_delaunay_case_twice_the_same_bits(eng, delaunay):
    verts, tris = delaunay
    n0, n1, hs, shift = cases.DELAUNAY_N0, cases.DELAUNAY_N1, cases.DELAUNAY_HS, cases.DELAUNAY_SHIFT
    want = raster_ref.build_heightfield(verts, tris, n0, n1, hs, shift, -7.5)
    assert want[1] == 0 and want[2] == 0
    a, _, _ = check(eng, verts, tris, n0, n1, hs, shift, want=want)
    b, _, _ = check(eng, verts, tris, n0, n1, hs, shift, want=want)
    assert np.array_equal(bits(a), bits(b))


def test_device_and_host_inputs(eng, delaunay):
    verts, tris = delaunay
    n0, n1, hs, shift = cases.DELAUNAY_N0, cases.DELAUNAY_N1, cases.DELAUNAY_HS, cases.DELAUNAY_SHIFT
    host = eng.build_heightfield(verts, tris, n0, n1, hs, shift, 0.0)
    dv, dt = torch.from_numpy(verts).to(DEV), torch.from_numpy(tris).to(DEV)
    dev = eng.build_heightfield(dv, dt, n0, n1, hs, shift, 0.0)
    lists = eng.build_heightfield(verts.tolist(), tris.astype(np.int64), n0, n1, hs, shift, 0.0)
    assert np.array_equal(bits(host[0]), bits(dev[0])) and host[1:] == dev[1:]
    assert np.array_equal(bits(host[0]), bits(lists[0])) and host[1:] == lists[1:]


@pytest.mark.parametrize("n0,n1", [(1, 1), (1, 97), (97, 83)])
def test_grid_shapes(eng, delaunay, n0, n1):
    verts, tris = delaunay
    _, uncovered, _ = check(eng, verts, tris, n0, n1, cases.DELAUNAY_HS, cases.DELAUNAY_SHIFT)      # (1 x 97 runs past the mesh: fill)
    assert uncovered < n0 * n1


def test_two_triangles_cover_the_grid_and_more(eng):
    """A quad of two triangles around a 300 x 260 grid: the large route, 10 x 5 tiles per triangle, clipped on all four sides; every node
    of the diagonal's lattice points belongs to both."""
    hs, n0, n1 = 0.025, 300, 260
    lim = _lib.heightfield_limits()
    assert n0 > 2 * lim["tile_i"] and n1 > 2 * lim["tile_j"] and n0 * n1 > lim["small_nodes"]
    v = np.array([[-1.0, -0.75, 0.5], [8.5, -0.75, -1.25], [8.5, 7.0, 2.0], [-1.0, 7.0, 0.125]], dtype=np.float32)
    for tris in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[0, 1, 3], [3, 1, 2]]):
        _, uncovered, _ = check(eng, v, np.array(tris, dtype=np.int32), n0, n1, hs)
        assert uncovered == 0


def test_ladder_of_single_triangles(eng):
    """Boxes one below, at and one above the small route's largest box, and boxes that end one row / column before, at and after a tile
    boundary in either direction, from tile-aligned and unaligned origins; one box straddles a tile corner."""
    lim = _lib.heightfield_limits()
    small, ti, tj = lim["small_nodes"], lim["tile_i"], lim["tile_j"]
    assert (small, ti, tj) == (512, 32, 64)           # the shapes below are written for these values
    hs, n0, n1 = 0.05, 3 * ti + 7, 3 * tj + 5
    shapes = [(2 * ti, tj, 7, 73), (2 * ti, tj, 16, 32), (2 * ti, tj, 19, 27),        # 511, 512, 513 nodes
              (5, 9, 8, 64), (5, 9, 9, 57), (5, 9, 3, 171), (0, 0, 1, 1), (0, 0, 2, 1)]
    for h in (ti - 1, ti, ti + 1):
        shapes += [(ti, tj, h, 20), (ti + 1, tj + 3, h, 20)]                           # 20 columns: above `small` for every h here
    for w in (tj - 1, tj, tj + 1):
        shapes += [(ti, tj, 10, w), (ti + 5, tj + 1, 10, w)]
    shapes += [(ti - 6, tj - 20, 26, 31), (ti - 1, tj - 1, 2, 2), (2 * ti - 9, 2 * tj - 18, 40, 80)]      # across a tile corner
    sides = set()
    for n, (i0, j0, h, w) in enumerate(shapes):
        v, t = box_triangle(i0, j0, h, w, hs, flip=bool(n & 1))
        assert box_nodes(v, n0, n1, hs, (0.0, 0.0)) == (i0, i0 + h - 1, j0, j0 + w - 1)
        sides.add(h * w > small)
        got, uncovered, _ = check(eng, v, t, n0, n1, hs)
        assert uncovered < n0 * n1
    assert sides == {False, True}


def test_grid_mesh_nodes_on_edges_and_vertices(eng):
    """synth.grid_mesh(25) at hs = res / 4: every vertex sits on a node, every fourth row and column of nodes on an edge, the diagonals
    pass through nodes — hundreds of nodes that two or six triangles share."""
    verts, tris, _ = synth.grid_mesh(25)
    n = 24 * 4 + 1
    want = raster_ref.build_heightfield(verts, tris, n, n, 0.025, (0.0, 0.0), -7.5, return_count=True)
    assert want[1] == 0 and int(want[4].sum()) > 500 and int((want[3] >= 6).sum()) >= 23 * 23
    check(eng, verts, tris, n, n, 0.025, want=want)


def test_layers_negative_heights_and_signed_zeros(eng):
    hs, n0, n1 = 0.05, 40, 36
    ground = (np.array([[-1, -1, 0.125], [3, -1, 0.25], [3, 3, -0.125], [-1, 3, 0.0]], dtype=np.float32), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
    rock = cases.pyramid(1.0, 0.9, -0.25, 0.8, 0.6, 1.5)                     # its base lies below the ground, its apex above
    for order in ([ground, rock], [rock, ground]):
        v, t = cases.merge(order)
        got, _, _ = check(eng, v, t, n0, n1, hs)
        assert float(got[20, 18]) > 1.0 and float(got[2, 2]) < 0.3             # the rock wins where it is higher, the ground elsewhere
    v, t = cases.merge([ground, rock])
    v[:, 2] = v[:, 2] - 5.0                                                   # all negative
    got, _, _ = check(eng, v, t, n0, n1, hs, fill=1.0)
    assert float(got.max()) < 0.0
    pz = np.array([[-1, -1, 0.0], [3, -1, 0.0], [-1, 3, 0.0]], dtype=np.float32)
    nz = pz.copy()
    nz[:, 2] = -0.0
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    got, _, _ = check(eng, nz, tri, n0, n1, hs)
    assert int(bits(got)[0, 0]) == 0x80000000                                 # -0 stays -0 ...
    for order in ([(pz, tri), (nz, tri)], [(nz, tri), (pz, tri)]):
        got, _, _ = check(eng, *cases.merge(order), n0, n1, hs)
        assert int(bits(got)[0, 0]) == 0                                      # ... and +0 wins over it, in either order


def test_triangles_that_do_not_contribute(eng):
    hs, n0, n1 = 0.05, 33, 21
    tiny = np.array([[0.51, 0.51, 1.0], [0.54, 0.51, 1.0], [0.52, 0.54, 1.0]])              # between the nodes at 0.50 and 0.55
    wall = np.array([[0.4, 0.4, 0.0], [0.6, 0.6, 0.0], [0.6, 0.6, 2.0]])                    # vertical: zero area
    flat = np.array([[0.2, 0.2, 1.0], [0.2, 0.2, 1.0], [0.9, 0.3, 1.0]])                    # two equal vertices
    left = np.array([[-3.0, 0.1, 1.0], [-0.01, 0.1, 1.0], [-1.0, 0.9, 1.0]])
    above = np.array([[0.1, 1.001, 1.0], [1.5, 1.2, 1.0], [0.5, 4.0, 1.0]])                 # the last column of nodes is at y = 1.0
    right = np.array([[1.601, 0.0, 1.0], [5.0, 0.1, 1.0], [2.0, 1.0, 1.0]])                 # the last row at x = 1.6
    meshes = [(m.astype(np.float32), np.array([[0, 1, 2]], dtype=np.int32)) for m in (tiny, wall, flat, left, above, right)]
    v, t = cases.merge(meshes)
    got, uncovered, skipped = check(eng, v, t, n0, n1, hs, fill=-2.5)
    assert uncovered == n0 * n1 and skipped == 0 and bool((got == -2.5).all())
    # no vertices, no triangles
    got, uncovered, skipped = check(eng, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 5, 7, hs, fill=3.0)
    assert uncovered == 35 and skipped == 0


def test_a_mesh_with_a_hole(eng):
    verts, tris, _ = synth.grid_mesh(9)
    keep = np.ones(len(tris), dtype=bool)
    keep[2 * (3 * 8 + 3):2 * (3 * 8 + 5)] = False                             # cells (3, 3) and (3, 4)
    got, uncovered, _ = check(eng, verts, tris[keep], 33, 33, 0.025, fill=-1.0)
    assert uncovered == 3 * 7 and bool((got[13:16, 13:20] == -1.0).all())         # the nodes strictly inside the hole
    got, uncovered, _ = check(eng, verts, tris[keep], 40, 33, 0.025, fill=9.0)     # and rows beyond the mesh
    assert uncovered == 3 * 7 + 7 * 33


def test_skipped_triangles(eng):
    verts, tris, _ = synth.grid_mesh(9)
    hs = 0.025
    far = float(np.float32((2 ** 25 + 300) / 256.0 * hs))
    extra = np.array([[np.nan, 0.3, 0.0], [0.3, 0.4, np.inf], [-np.inf, 0.1, 0.0], [far, 0.2, 0.0], [0.35, 0.35, 5.0], [0.45, 0.35, 5.0],
                      [0.35, 0.45, np.nan]], dtype=np.float32)
    base = len(verts)
    v = np.concatenate([verts, extra]).astype(np.float32)
    V = len(v)
    bad = np.array([[base + 0, base + 4, base + 5], [base + 4, base + 1, base + 5], [base + 4, base + 5, base + 2], [base + 3, base + 4, base + 5],
                    [base + 4, base + 5, base + 6], [-1, base + 4, base + 5], [base + 4, V, base + 5], [base + 4, base + 5, 2 ** 31 - 1],
                    [-2 ** 31, 0, 1]], dtype=np.int32)
    t = np.concatenate([tris[:40], bad, tris[40:]]).astype(np.int32)
    got, uncovered, skipped = check(eng, v, t, 33, 33, hs)
    assert skipped == len(bad) and uncovered == 0 and float(got.max()) < 5.0
    # the same mesh without them: the same heights
    clean, _, _ = check(eng, verts, tris, 33, 33, hs)
    assert np.array_equal(bits(got), bits(clean))
    # a vertex exactly at the limit is still drawn
    edge = np.array([[0.0, 0.0, 1.0], [float(np.float32(2 ** 25 / 256.0 * hs)), 0.0, 1.0], [0.0, 1.0, 1.0]], dtype=np.float32)
    assert int(np.abs(raster_ref.snap_vertices(edge, hs, (0.0, 0.0))[0]).max()) == 2 ** 25
    _, uncovered, skipped = check(eng, edge, np.array([[0, 1, 2]], dtype=np.int32), 33, 33, hs)
    assert skipped == 0 and uncovered < 33 * 33


def test_binding_refuses_bad_shapes(eng):
    v, t = np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32)
    for kw in (dict(n0=0), dict(n1=131073), dict(horizontal_scale=0.0), dict(shift=(float("nan"), 0.0))):
        a = dict(n0=4, n1=4, horizontal_scale=0.025, shift=(0.0, 0.0))
        a.update(kw)
        with pytest.raises(_lib.RoverError):
            eng.build_heightfield(v, t, a["n0"], a["n1"], a["horizontal_scale"], a["shift"])
    with pytest.raises(_lib.RoverError):
        eng.build_heightfield(np.zeros((3, 2), np.float32), t, 4, 4)


def test_scene_from_two_meshes():
    """assets.build_scene_from_meshes on a small irregular mesh: set_scene takes the result, sample_height at every node's position
    returns the heightfield's bits, the heightfield is the restatement's on the fp16-rounded vertices, and the terrain sim steps on it."""
    from isaac_rover_amd.config import SimConfig
    from isaac_rover_amd.tasks.rover import RoverTask
    from isaac_rover_amd.vec_env import TerrainSim, VecEnv
    cells, e = 64, 32
    spec = synth.IrregularSpec(extent_x=cells * 0.1, extent_y=cells * 0.1, n_rocks=5, seed=4, coarse=0.6, fine=0.075)
    verts, tris, rock_tris, _ = synth.irregular_mesh(spec)
    eng = _lib.Engine(e, device=0)
    scene, uncovered, skipped = assets.build_scene_from_meshes(eng, (verts, tris), (verts, rock_tris), n_cells=cells, k=16, return_stats=True)
    n = cells * 4
    assert tuple(scene.heightmap.shape) == (n, n) and scene.vertical_scale == 1.0 and (uncovered, skipped) == (0, 0)
    v16 = torch.from_numpy(verts).to(torch.float16).to(torch.float32).numpy()
    want, w_uncovered, w_skipped = raster_ref.build_heightfield(v16, tris, n, n, 0.025, (0.0, 0.0), float(v16[:, 2].min()))
    assert np.array_equal(bits(scene.heightmap), bits(want)) and (w_uncovered, w_skipped) == (0, 0)
    assert np.array_equal(scene.stone_info_raw, assets.stones_from_mesh(verts, rock_tris)) and len(scene.stone_info_raw) >= 1
    eng.set_scene(scene, synth.ray_distribution("37"))
    pos = np.arange(n, dtype=np.float64) * float(np.float32(0.025))
    xy = torch.from_numpy(np.stack(np.meshgrid(pos, pos, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)).to(DEV)
    got = eng.sample_height(xy).reshape(n, n)
    assert np.array_equal(bits(got), bits(want))
    eng.close()
    env = VecEnv(headless=True, sim="terrain")
    task = RoverTask("Rover", SimConfig(num_envs=e, device=DEV), env, scene=scene, distribution=synth.ray_distribution("37"))
    g = torch.Generator().manual_seed(0)
    spawn = torch.zeros(e, 3)
    spawn[:, 0:2] = 0.2 * cells * 0.1 + 0.6 * cells * 0.1 * torch.rand(e, 2, generator=g)
    env.set_task(task, sim_params={"dt": 0.05}, spawn_positions=spawn)
    assert isinstance(env._world, TerrainSim)
    obs = env.reset()
    actions = torch.tensor([[0.8, 0.25]], device=DEV).repeat(e, 1)
    for _ in range(5):
        obs, rew, done, info = env.step(actions)
    assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
    pos3, _ = task._rover.get_world_poses()
    # a rover rides ride_height above the plane fitted through its wheel contacts: its z stays near the heightfield's range
    assert float(pos3[:, 2].min()) >= float(want.min()) - 1.0 and float(pos3[:, 2].max()) <= float(want.max()) + 1.0
    env.close()
