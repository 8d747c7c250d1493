"""The staged ray cast with its level loop measured from the point where a ray's line crosses the row's own height (option "lane_rebase",
bit 4 of the kernel's `forms` word) against the same library with the option off, against a kernel that evaluates every
triangle of a ray's cell — the env-order kernel (variant 1) in f32, the binned one (variant 2) for the as-shipped arithmetic — and, on
the device's own rays, against the oracle: obs, reward, done flags and all 26 + P distances identical, bit for bit.  One engine per case
casts the same rays with the option as created, 0 and 1 (it is read at every launch).  The smallest shapes that take every path: 24 x 24
and 25 x 25 cells, K = 40 and 200, 64 and 257 envs, 37 and 120 heightmap rays, f32 and as shipped, behind the sort and in env order, rows
shared or per cell, boxes or spheres, the irregular mesh.  Poses: the tilted and upside-down rovers of tests/test_lane_pair_rows_gpu.py
(d_z of either sign), rovers on the map's border, sixteen rovers 2 m above the terrain tilted by 0.32 ... 0.52 rad (both sides of the
steep limit acos 0.9 = 0.451 rad, where the origin's height counts most), and the hand-made rays of tests/test_lane_box_gpu.py
(axis-parallel, flat, wild, NaN, inf)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _states(kind, cells, k, envs, border):
    from test_lane_pair_rows_gpu import _states as base_states
    from isaac_rover_amd import synth
    st = {key: v.clone() for key, v in base_states(kind, cells, k, envs, border).items()}
    n = 16
    tilt = torch.linspace(0.32, 0.52, n)
    sign = torch.tensor([1.0, -1.0]).repeat(n // 2)
    roll = torch.where(torch.arange(n) % 4 < 2, tilt * sign, torch.zeros(n))
    pitch = torch.where(torch.arange(n) % 4 < 2, torch.zeros(n), tilt * sign)
    st["quat"][30:30 + n] = synth.quat_from_euler(roll, pitch, torch.linspace(-3.0, 3.0, n))
    st["pos"][30:30 + n, 2] += 1.5                                        # make_states puts the origin 0.5 m above the surface: 2 m
    # six rovers on their backs, some of them lifted too: d_z < 0 (the reference casts lines: they meet the terrain behind their origin)
    flip = torch.tensor([0.0, 0.1, -0.2, 0.3, -0.4, 0.47])
    st["quat"][46:52] = synth.quat_from_euler(math.pi + flip, 0.5 * flip, torch.linspace(-2.0, 2.0, 6))
    st["pos"][49:52, 2] += 1.0
    return st


def _run(case, options, rebase_values, oracle=False):
    """One engine; per value of "lane_rebase" one step and one cast of the crafted rays -> [(outputs, distances, crafted distances, counters)]."""
    from hip_helpers import _oracle_maps, _rays_vs_oracle, hip_step
    from test_lane_box_gpu import _crafted_rays
    from test_lane_pair_rows_gpu import _scene
    from isaac_rover_amd import _lib, synth
    kind, cells, k, envs, rays, prec, _env_order, border, pair_rows, box = case
    scene = _scene(kind, cells, k)[0]
    eng = _lib.Engine(envs, device=0)
    eng.set_option("lane_pair_rows", pair_rows)                           # (both read when the maps are set)
    eng.set_option("lane_box", box)
    eng.set_scene(scene, synth.ray_distribution(rays))
    eng.set_option("ray_precision", prec)
    for name, v in options.items():
        eng.set_option(name, v)
    assert eng.info().raycast_variant == options["raycast_variant"]
    st = _states(kind, cells, k, envs, border)
    res = []
    for rebase in rebase_values:
        if rebase is not None:
            eng.set_option("lane_rebase", rebase)
        out = hip_step(eng, st)
        if oracle:
            _rays_vs_oracle(eng, _oracle_maps(scene), prec == 2, f"lane_rebase={rebase} {case}")
        src, dirs, _cell, dist = eng.export_rays()
        ci = eng.cull_info() if options["raycast_variant"] == 4 else None
        crafted = eng.cast_rays(*_crafted_rays(src, dirs)).cpu().numpy()
        res.append((out, dist.cpu().numpy(), crafted, ci, dirs.cpu().numpy()))
    eng.close()
    return res


@functools.lru_cache(maxsize=None)
def _reference(case):
    return _run(case, {"raycast_variant": 2 if case[5] == 2 else 1}, (None,))[0]


def _same(got, ref, label):
    for key in ref[0]:
        np.testing.assert_array_equal(got[0][key], ref[0][key], err_msg=f"{key} {label}")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"distances {label}")
    np.testing.assert_array_equal(got[2], ref[2], err_msg=f"crafted rays {label}")


# (kind, cells, K, envs, heightmap rays, ray_precision, lane_env_order, rovers on the border, lane_pair_rows, lane_box)
CASES = [
    ("grid", 24, 40, 64, "37", 0, 0, False, 1, 1),
    ("grid", 25, 200, 257, "120", 0, 0, False, 1, 0),
    ("grid", 25, 200, 64, "37", 0, 0, True, 0, 1),
    ("grid", 25, 200, 257, "37", 0, 0, True, 1, 1),
    ("grid", 24, 200, 64, "37", 0, 1, False, 1, 0),
    ("grid", 24, 200, 257, "37", 2, 0, False, 1, -1),
    ("grid", 25, 40, 64, "120", 2, 1, False, 0, -1),
    ("irregular", 40, 64, 64, "37", 0, 0, False, -1, -1),
    ("irregular", 40, 64, 64, "37", 2, 1, False, 1, -1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_rebase_changes_no_bit(case):
    kind, cells, k, envs, rays, prec, env_order, border, pair_rows, box = case
    ref = _reference(case)
    assert (ref[1] < 11.0).mean() > 0.1 and (ref[2][0:6] < 11.0).mean() > 0.1      # the rays do meet triangles (a 2.4 m map: the outer rings, the lifted and the flipped rovers miss it)
    dz = ref[4][:, 26:, 2]
    cosb = np.abs(dz[30:46]).min(axis=1)
    assert (dz > 0).any() and (dz < 0).any(), "heightmap rays of either d_z sign"
    assert (cosb < 0.9).any() and (cosb > 0.9).any(), "the lifted rovers sit on both sides of the steep limit"
    dflt, off, on = _run(case, {"raycast_variant": 4, "lane_env_order": env_order, "lane_rocks": 1}, (None, 0, 1), oracle=True)
    for rebase, got in ((0, off), (1, on)):
        ci = got[3]
        print(f"lane_rebase={rebase} {case}: bins {ci['bins']}, items {ci['lane_items']}, pairs per ray {ci['pairs_per_ray']:.3f}")
        assert ci["rays"] == envs * (int(rays) + 26) and ci["candidate_pairs"] > 0
        _same(got, ref, f"lane_rebase={rebase} {case}")
    _same(on, off, f"lane_rebase 1 against 0 {case}")
    assert on[3]["rays"] == off[3]["rays"] and on[3]["bins"] == off[3]["bins"]
    assert on[3]["lane_items"] != off[3]["lane_items"], "the option reaches the kernel: some ray's level moves"
    assert dflt[3]["lane_items"] == on[3]["lane_items"], "the default is 1"


def test_the_option_takes_0_and_1_only():
    from isaac_rover_amd import _lib
    eng = _lib.Engine(8, device=0)
    eng.set_option("lane_rebase", 0)
    eng.set_option("lane_rebase", 1)
    for bad in (-1, 2):
        with pytest.raises(_lib.RoverError):
            eng.set_option("lane_rebase", bad)
    eng.close()
