"""The staged ray cast on tables with one row per two cells (option "lane_pair_rows", rover_info.lane_pair_rows) against a
kernel that evaluates every triangle of a ray's cell — the env-order kernel (variant 1) in f32, the binned one (variant 2) for the
as-shipped arithmetic, which variant 1 does not have — and, on the device's own rays, against the oracle: obs, reward, done flags and all
26 + P distances identical with "lane_pair_rows" 0 and 1.  The smallest shapes that take every path: 24 x 24 cells and 25 x 25 (Y odd: a
column's last row serves one cell), K = 40 (5 chunks a row) and K = 200 (a union of 112 pairs: 14 chunks), 64 and 257 envs (one wave per
few cells / many rays per row and the queue's flushes), 37 and 120 heightmap rays, f32 and as shipped, behind the sort and in env order,
shuffled ids, the irregular mesh, rovers on the map's border, and hand-made rays (axis-parallel, flat, wild) through the same engines.
A map with a union of more than 128 pairs must keep its per-cell tables; "lane_pair_rows" 1 shares rows on the rocks map too, auto on
the terrain map only."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _scene(kind, cells, k):
    from isaac_rover_amd import _lib, assets, synth
    if kind == "grid":
        return synth.make_scene(n_cells=cells, k=k, n_stones=16), None
    if kind == "shuffled":
        return synth.shuffle_triangle_ids(_scene("grid", cells, k)[0], seed=3), None
    if kind == "irregular":
        spec = synth.IrregularSpec(extent_x=cells * 0.1, extent_y=cells * 0.1, n_rocks=5, seed=4, coarse=0.6, fine=0.0375)
        tool = _lib.Engine(8, device=0)
        irr, zf = assets.build_irregular_scene(tool, spec, 64)
        tool.close()
        return irr, zf
    assert kind == "disjoint"
    # K = 256, and cells that neighbour in iy list DISJOINT triangles (the even cells the nearest of the mesh cells with i + j even, the
    # odd cells of those with i + j odd): every union is 512 triangles = 256 pairs, twice what a row holds
    g = _scene("grid", cells, 200)[0]
    n_vert = cells + 1
    cx, cy = synth._centroid_lattice(n_vert, torch.device("cpu"))
    tri = torch.arange(cx.numel())
    mesh_cell = tri // 2
    colour = (mesh_cell // cells + mesh_cell % cells) % 2
    maps = [synth.knn_map_from_subset(cells, cx, cy, tri[colour == c], 256) for c in (0, 1)]
    idx = maps[0].clone()
    idx[:, 1::2] = maps[1][:, 1::2]
    return synth.Scene(terrain=synth.KnnMap(idx, g.terrain.triangles, g.terrain.vertices), rocks=g.rocks, stone_info_raw=g.stone_info_raw,
                       heightmap=g.heightmap, horizontal_scale=g.horizontal_scale, vertical_scale=g.vertical_scale, shift=g.shift), None


def _states(kind, cells, k, envs, border):
    from isaac_rover_amd import synth
    zf = _scene(kind, cells, k)[1]
    kw = {} if zf is None else dict(heightfn=zf, margin_m=0.5)
    if border:
        kw["margin_m"] = 0.0                                               # rovers up to the map's edge: rays in the border cells and beyond them
    st = synth.make_states(envs, cells * 0.1, seed=31, **kw)
    g = torch.Generator().manual_seed(9)
    # a third of the rovers tilted well off the vertical (their rays leave the rows' cones: tests (A) and (B)), a few upside down
    st["quat"][0:20] = synth.quat_from_euler(0.6 * torch.randn(20, generator=g), 0.6 * torch.randn(20, generator=g), 3.0 * torch.randn(20, generator=g))
    q = torch.randn(6, 4, generator=g)
    st["quat"][20:26] = q / q.norm(dim=1, keepdim=True)
    if border:
        st["pos"][26:30, 0] = torch.tensor([0.0, cells * 0.1, 0.3, 1.1])
        st["pos"][26:30, 1] = torch.tensor([0.7, 1.3, 0.0, cells * 0.1])
    return st


def _run(case, options, pair_rows=None, oracle=False):
    """One step and one cast of the crafted rays -> (outputs of the step, exported distances, distances of the crafted rays, rover_info's
    lane_pair_rows, the counters)."""
    from hip_helpers import _oracle_maps, _rays_vs_oracle, hip_step
    from test_lane_box_gpu import _crafted_rays
    from isaac_rover_amd import _lib, synth
    kind, cells, k, envs, rays, prec, _env_order, border = case
    scene = _scene(kind, cells, k)[0]
    eng = _lib.Engine(envs, device=0)
    if pair_rows is not None:
        eng.set_option("lane_pair_rows", pair_rows)                       # (read when the maps are set)
    eng.set_scene(scene, synth.ray_distribution(rays))
    eng.set_option("ray_precision", prec)
    for name, v in options.items():
        eng.set_option(name, v)
    assert eng.info().raycast_variant == options["raycast_variant"]
    out = hip_step(eng, _states(kind, cells, k, envs, border))
    if oracle:
        _rays_vs_oracle(eng, _oracle_maps(scene), prec == 2, f"lane_pair_rows={pair_rows} {case}")
    src, dirs, _cell, dist = eng.export_rays()
    crafted = eng.cast_rays(*_crafted_rays(src, dirs)).cpu().numpy()
    form = list(eng.info().lane_pair_rows)
    ci = eng.cull_info() if options["raycast_variant"] == 4 else None
    eng.close()
    return out, dist.cpu().numpy(), crafted, form, ci


@functools.lru_cache(maxsize=None)
def _reference(case):
    return _run(case, {"raycast_variant": 2 if case[5] == 2 else 1})


def _same(got, ref, label):
    for key in ref[0]:
        np.testing.assert_array_equal(got[0][key], ref[0][key], err_msg=f"{key} {label}")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"distances {label}")
    np.testing.assert_array_equal(got[2], ref[2], err_msg=f"crafted rays {label}")


# (kind, cells, K, envs, heightmap rays, ray_precision, lane_env_order, rovers on the border)
CASES = [
    ("grid", 24, 40, 64, "37", 0, 0, False),
    ("grid", 25, 40, 64, "37", 0, 0, False),
    ("grid", 24, 200, 64, "37", 0, 0, False),
    ("grid", 25, 200, 257, "120", 0, 0, False),
    ("grid", 25, 200, 257, "37", 2, 0, False),
    ("grid", 24, 40, 64, "120", 2, 1, False),
    ("grid", 25, 200, 64, "37", 0, 1, False),
    ("grid", 24, 200, 257, "37", 2, 1, False),
    ("shuffled", 25, 200, 64, "37", 0, 0, False),
    ("irregular", 40, 64, 64, "37", 0, 0, False),
    ("irregular", 40, 64, 64, "37", 2, 1, False),
    ("grid", 25, 200, 64, "37", 0, 0, True),
    ("grid", 24, 40, 64, "37", 2, 0, True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_pair_rows_change_no_bit(case):
    kind, cells, k, envs, rays, prec, env_order, border = case
    ref = _reference(case)
    assert (ref[1] < 11.0).mean() > 0.2 and (ref[2][0:6] < 11.0).mean() > 0.1      # the rays do meet triangles
    opts = {"raycast_variant": 4, "lane_env_order": env_order, "lane_rocks": 1}
    for pair_rows in (0, 1):
        got = _run(case, opts, pair_rows=pair_rows, oracle=True)
        form, ci = got[3], got[4]
        if pair_rows == 0:
            assert form == [0, 0]
        elif kind != "irregular":
            assert form == [1, 1], "a grid mesh's unions fit a row at K <= 200: both maps share rows when asked to"
        else:
            assert form[0] in (0, 1) and form[1] in (0, 1)
        print(f"lane_pair_rows={pair_rows} {case}: form {form}, bins {ci['bins']}, items {ci['lane_items']}, pairs per ray {ci['pairs_per_ray']:.3f}")
        assert ci["rays"] == envs * (int(rays) + 26) and ci["candidate_pairs"] > 0
        _same(got, ref, f"lane_pair_rows={pair_rows} {case}")


def test_auto_shares_rows_on_the_terrain_map_only():
    case = ("grid", 24, 200, 64, "37", 0, 0, False)
    ref = _reference(case)
    got = _run(case, {"raycast_variant": 4, "lane_env_order": 0, "lane_rocks": 1})
    assert got[3] == [1, 0]
    _same(got, ref, f"auto {case}")


def test_bins_keep_counting_cells():
    """The counters of rover_get_cull_info do not depend on the form where they count rays and cells."""
    case = ("grid", 25, 200, 64, "37", 0, 0, False)
    opts = {"raycast_variant": 4, "lane_env_order": 0, "lane_rocks": 1}
    a, b = _run(case, opts, pair_rows=0)[4], _run(case, opts, pair_rows=1)[4]
    assert a["rays"] == b["rays"] and a["bins"] == b["bins"]


@pytest.mark.parametrize("prec,env_order", [(0, 0), (2, 1)])
def test_a_union_that_does_not_fit_keeps_the_per_cell_tables(prec, env_order):
    case = ("disjoint", 24, 256, 64, "37", prec, env_order, False)
    ref = _reference(case)
    got = _run(case, {"raycast_variant": 4, "lane_env_order": env_order, "lane_rocks": 1}, pair_rows=1, oracle=True)
    assert got[3][0] == 0, "unions of 256 pairs: the terrain map keeps one row per cell"
    _same(got, ref, f"lane_pair_rows=1 {case}")
