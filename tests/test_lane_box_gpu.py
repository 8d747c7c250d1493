"""The staged ray cast with test (A) on boxes (option "lane_box", rover_info.lane_box) against the env-order kernel, which evaluates every
triangle: obs, reward, done flags and all 26 + P distances identical, on the smallest shapes that take every path — a 40 x 40-cell grid scene
(K = 200: 13 chunks a row, two runs of 64 rays and more per cell) behind the sort and in env order, 37 and 120 heightmap rays, the same
mesh with shuffled ids, a small irregular mesh (which must come out in sphere form), and a grid terrain over irregular rocks (both forms
in one launch: the wave at the border of the sorted list and every wave in env order read both).  Then hand-made rays through the same
engines: exactly axis-parallel, flat (d_z = 0 and nearly 0) and wild ones."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 64
CELLS = 40


@functools.lru_cache(maxsize=None)
def _scene(kind):
    from isaac_rover_amd import _lib, assets, synth
    if kind == "grid":
        return synth.make_scene(n_cells=CELLS, k=200, n_stones=16), None
    if kind == "shuffled":
        return synth.shuffle_triangle_ids(_scene("grid")[0], seed=3), None
    spec = synth.IrregularSpec(extent_x=CELLS * 0.1, extent_y=CELLS * 0.1, n_rocks=5, seed=4, coarse=0.6, fine=0.0375)
    tool = _lib.Engine(8, device=0)
    irr, zf = assets.build_irregular_scene(tool, spec, 64)
    tool.close()
    if kind == "irregular":
        return irr, zf
    assert kind == "mixed"
    g = _scene("grid")[0]
    return synth.Scene(terrain=g.terrain, rocks=irr.rocks, stone_info_raw=g.stone_info_raw, heightmap=g.heightmap,
                       horizontal_scale=g.horizontal_scale, vertical_scale=g.vertical_scale, shift=g.shift), None


def _states(kind):
    from isaac_rover_amd import synth
    zf = _scene(kind)[1]
    kw = {} if zf is None else dict(heightfn=zf, margin_m=0.5)
    st = synth.make_states(E, CELLS * 0.1, seed=31, **kw)
    g = torch.Generator().manual_seed(9)
    # a third of the rovers tilted well off the vertical (their rays leave the cells' cones: tests (A) and (B)), a few upside down
    st["quat"][0:20] = synth.quat_from_euler(0.6 * torch.randn(20, generator=g), 0.6 * torch.randn(20, generator=g), 3.0 * torch.randn(20, generator=g))
    q = torch.randn(6, 4, generator=g)
    st["quat"][20:26] = q / q.norm(dim=1, keepdim=True)
    return st


def _crafted_rays(src, dirs):
    """export_rays' arrays with the first rovers' rays replaced: env 0-3 exactly axis-parallel (+z, -z, +x, +y: the last two flat, d_z = 0),
    env 4 flat with d_z = 1e-4 ... 1e-3 at many azimuths, env 5 axis-parallel in the cell-boundary planes, env 6 wild (origins far away, NaN, inf: the library refuses directions that are not of unit length)."""
    src, dirs = src.clone(), dirs.clone()
    r = src.shape[1]
    for e, d in enumerate(((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))):
        dirs[e] = torch.tensor(d)
    src[2:4, :, 2] = src[2:4, :, 2].clamp(max=0.4)                         # low enough to meet ground and rocks side-on
    az = torch.arange(r, dtype=torch.float64) * (2 * math.pi / r) + 0.01
    dz = torch.linspace(1.0e-4, 1.0e-3, r, dtype=torch.float64)
    flat = torch.stack((torch.cos(az), torch.sin(az), dz), dim=1)
    dirs[4] = (flat / flat.norm(dim=1, keepdim=True)).to(torch.float32)
    src[4, :, 2] = src[4, :, 2].clamp(max=0.4)
    dirs[5] = torch.tensor((0.0, 0.0, 1.0))
    src[5, :, 0:2] = torch.round(src[5, :, 0:2] * 10) / 10                  # on the grid lines: through vertices and along box faces
    src[6, 0::3] *= 1.0e5
    src[6, 1::3, 0] = float("nan")
    src[6, 2::3, 2] = float("inf")
    return src.contiguous(), dirs.contiguous()


def _run(kind, rays, options, lane_box=None):
    """One step and one cast of the crafted rays -> (outputs of the step, exported distances, distances of the crafted rays, rover_info)."""
    from hip_helpers import hip_step
    from isaac_rover_amd import _lib, synth
    eng = _lib.Engine(E, device=0)
    if lane_box is not None:
        eng.set_option("lane_box", lane_box)                              # (read when the maps are set)
    eng.set_scene(_scene(kind)[0], synth.ray_distribution(rays))
    for k, v in options.items():
        eng.set_option(k, v)
    assert eng.info().raycast_variant == options["raycast_variant"]
    out = hip_step(eng, _states(kind))
    src, dirs, _cell, dist = eng.export_rays()
    crafted = eng.cast_rays(*_crafted_rays(src, dirs)).cpu().numpy()
    form = list(eng.info().lane_box)
    ci = eng.cull_info() if options["raycast_variant"] == 4 else None
    eng.close()
    return out, dist.cpu().numpy(), crafted, form, ci


@functools.lru_cache(maxsize=None)
def _reference(kind, rays):
    return _run(kind, rays, {"raycast_variant": 1})


CASES = [("grid", "37", 0), ("grid", "37", 1), ("grid", "120", 0), ("shuffled", "37", 0), ("irregular", "37", 0), ("mixed", "37", 0),
         ("mixed", "37", 1)]


@pytest.mark.parametrize("kind,rays,env_order", CASES)
def test_box_form_changes_no_bit(kind, rays, env_order):
    ref, ref_dist, ref_crafted, _, _ = _reference(kind, rays)
    assert (ref_dist < 11.0).mean() > 0.2 and (ref_crafted[0:6] < 11.0).mean() > 0.1      # the rays do meet triangles
    opts = {"raycast_variant": 4, "lane_env_order": env_order, "lane_rocks": 1}
    got, dist, crafted, form, ci = _run(kind, rays, opts)
    if kind == "irregular":
        assert form == [0, 0], "an irregular mesh stays in sphere form"
    elif kind == "mixed":
        assert form == [1, 0], "grid terrain in box form over irregular rocks in sphere form"
    else:
        assert form[0] == 1, "a grid terrain map is built in box form"
    assert ci["rays"] == E * (int(rays) + 26) and ci["candidate_pairs"] > 0
    for key in ref:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{key} {kind} P={rays} env_order={env_order}")
    np.testing.assert_array_equal(dist, ref_dist)
    np.testing.assert_array_equal(crafted, ref_crafted)


@pytest.mark.parametrize("kind,lane_box", [("grid", 0), ("irregular", 1), ("mixed", 1)])
def test_forced_form_changes_no_bit(kind, lane_box):
    """"lane_box" 0 keeps spheres on a grid (the A/B arm); 1 puts boxes on any mesh — needles, always-candidate triangles and pairs
    that cannot be encoded included — and the results stay what they are."""
    ref, ref_dist, ref_crafted, _, _ = _reference(kind, "37")
    for env_order in (0, 1):
        got, dist, crafted, form, _ = _run(kind, "37", {"raycast_variant": 4, "lane_env_order": env_order, "lane_rocks": 1}, lane_box=lane_box)
        assert form == [lane_box, lane_box]
        for key in ref:
            np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{key} {kind} lane_box={lane_box} env_order={env_order}")
        np.testing.assert_array_equal(dist, ref_dist)
        np.testing.assert_array_equal(crafted, ref_crafted)


def test_box_form_tests_fewer_pairs_exactly():
    """On the grid scene the box sends fewer pairs to the exact arithmetic than the two spheres (what the form is for)."""
    opts = {"raycast_variant": 4, "lane_env_order": 0, "lane_rocks": 1}
    box, sph = _run("grid", "37", opts)[4], _run("grid", "37", opts, lane_box=0)[4]
    print(f"candidate pairs per ray: box {box['pairs_per_ray']:.3f}, spheres {sph['pairs_per_ray']:.3f}; items {box['lane_items']} / {sph['lane_items']}")
    assert box["rays"] == sph["rays"] and box["candidate_pairs"] < sph["candidate_pairs"]
