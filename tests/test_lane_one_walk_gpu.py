"""The staged ray cast's one walk over its item list — a round of 64 items runs test (A) in every lane and then, only in a round that reaches
into the (A) + (B) part of the list, test (B) in the lanes whose item lies there — against a kernel that evaluates every triangle of a ray's
cell (the env-order kernel, variant 1, in f32; the binned one, variant 2, for the as-shipped arithmetic) and, on the device's own rays,
against the oracle: obs, reward, done flags, collisions and all 26 + P distances identical by IEEE equality.  One engine per case.  The
smallest shapes that take every path of the loop:
  * a few (A) + (B) items beside many (A) items (grid scene, level rovers beside tilted and flipped ones): mixed rounds, waves without any;
  * many (A) + (B) items beside few (A) items (the irregular mesh): rounds wholly in the (A) + (B) part, waves without (A) items;
  * env order: a wave holds both maps, box and sphere tables in one walk (one pass per form), padding slots, a short last wave;
  * as shipped (16-byte (B) records), rows shared or per cell, boxes or spheres;
  * the hand-made rays of tests/test_lane_box_gpu.py in every case: a wild ray has no items and every pair as a candidate, a flat ray has
    all its chunks as (A) + (B) items.
The item list itself is what it was before the walks were merged: every case's `lane_items` is the count the library reported then."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (kind, cells, K, envs, heightmap rays, ray_precision, lane_env_order, rovers on the border, lane_pair_rows, lane_box)
TERRAIN = [
    ("grid", 24, 40, 257, "37", 0, 0, False, -1, -1),
    ("grid", 25, 200, 257, "37", 0, 0, True, -1, -1),
]
IRREGULAR = [                                                             # ("tilted": every rover of the batch well off the vertical)
    ("irregular-tilted", 40, 64, 64, "37", 0, 0, False, -1, -1),
    ("irregular-tilted", 40, 64, 257, "37", 0, 0, False, -1, -1),
]
ENV_ORDER = [
    ("mixed", 40, 200, 64, "37", 0, 1, False, -1, -1),
    ("grid", 24, 200, 64, "37", 0, 1, False, -1, -1),
    ("grid", 25, 40, 64, "120", 0, 1, False, -1, -1),
]
AS_SHIPPED = [
    ("grid", 24, 200, 64, "37", 2, 0, False, -1, -1),
    ("irregular", 40, 64, 64, "37", 2, 0, False, -1, -1),
    ("irregular", 40, 64, 64, "37", 2, 1, False, -1, -1),
]
FORMS = [("grid", 24, 40, 64, "37", 0, 0, False, pair_rows, box) for pair_rows in (0, 1) for box in (0, 1)]
TILT = (0.8, 1.2)                                                         # rad off the vertical, about a horizontal axis of any azimuth
CASES = TERRAIN + IRREGULAR + ENV_ORDER + AS_SHIPPED + FORMS

# `lane_items` of every case as the library of the commit before this walk reports it on the same inputs (the list is built as it was)
PARENT_LANE_ITEMS = {
    "grid-24-40-257-37-0-0-False--1--1": 42316,
    "grid-25-200-257-37-0-0-True--1--1": 128028,
    "irregular-tilted-40-64-64-37-0-0-False--1--1": 23232,
    "irregular-tilted-40-64-257-37-0-0-False--1--1": 93270,
    "mixed-40-200-64-37-0-1-False--1--1": 26206,
    "grid-24-200-64-37-0-1-False--1--1": 45130,
    "grid-25-40-64-120-0-1-False--1--1": 31353,
    "grid-24-200-64-37-2-0-False--1--1": 48506,
    "irregular-40-64-64-37-2-0-False--1--1": 19003,
    "irregular-40-64-64-37-2-1-False--1--1": 19003,
    "grid-24-40-64-37-0-0-False-0-0": 11288,
    "grid-24-40-64-37-0-0-False-0-1": 11288,
    "grid-24-40-64-37-0-0-False-1-0": 13676,
    "grid-24-40-64-37-0-0-False-1-1": 13676,
}


def _id(case):
    return "-".join(str(x) for x in case)


def _inputs(case):
    """-> (scene, states): the scenes and poses of the existing files — level rovers, the tilted and upside-down ones of
    test_lane_pair_rows_gpu, the sixteen tilted 0.32 ... 0.52 rad and the six on their backs of test_level_rebase_gpu."""
    import test_lane_box_gpu as box_file
    from test_lane_pair_rows_gpu import _scene
    from test_level_rebase_gpu import _states
    kind, cells, k, envs, _rays, _prec, _env_order, border, _pair_rows, _box = case
    if kind == "mixed":                                                   # grid terrain (boxes) over irregular rocks (spheres)
        assert (cells, k, envs) == (box_file.CELLS, 200, box_file.E)
        return box_file._scene("mixed")[0], box_file._states("mixed")
    if kind == "irregular-tilted":
        # the level rovers of the other cases lie within their cells' cones even on this mesh (a third of the 64 envs' rays run both tests, an
        # eighth of the 257 envs'): here every rover is tilted by TILT, so that the (A) + (B) part is the longer one
        from isaac_rover_amd import synth
        st = {key: v.clone() for key, v in _states("irregular", cells, k, envs, border).items()}
        g = torch.Generator().manual_seed(17)
        tilt = TILT[0] + (TILT[1] - TILT[0]) * torch.rand(envs, generator=g)
        axis = 2.0 * math.pi * torch.rand(envs, generator=g)
        st["quat"] = synth.quat_from_euler(tilt * torch.cos(axis), tilt * torch.sin(axis), 3.0 * torch.randn(envs, generator=g))
        return _scene("irregular", cells, k)[0], st
    return _scene(kind, cells, k)[0], _states(kind, cells, k, envs, border)


def _run(case, options, oracle=False):
    """One engine, one step and one cast of the crafted rays -> (outputs, distances, crafted distances, counters, rover_info's lane_box)."""
    from hip_helpers import _oracle_maps, _rays_vs_oracle, hip_step
    from test_lane_box_gpu import _crafted_rays
    from isaac_rover_amd import _lib, synth
    _kind, _cells, _k, envs, rays, prec, _env_order, _border, pair_rows, box = case
    scene, st = _inputs(case)
    eng = _lib.Engine(envs, device=0)
    eng.set_option("lane_pair_rows", pair_rows)                           # (both read when the maps are set)
    eng.set_option("lane_box", box)
    eng.set_scene(scene, synth.ray_distribution(rays))
    eng.set_option("ray_precision", prec)
    for name, v in options.items():
        eng.set_option(name, v)
    assert eng.info().raycast_variant == options["raycast_variant"]
    out = hip_step(eng, st)
    if oracle:
        _rays_vs_oracle(eng, _oracle_maps(scene), prec == 2, _id(case))
    src, dirs, _cell, dist = eng.export_rays()
    ci = eng.cull_info() if options["raycast_variant"] == 4 else None
    crafted = eng.cast_rays(*_crafted_rays(src, dirs)).cpu().numpy()
    form = list(eng.info().lane_box)
    eng.close()
    return out, dist.cpu().numpy(), crafted, ci, form


@functools.lru_cache(maxsize=None)
def _reference(key):
    """The every-triangle kernel on a case's inputs; it reads none of the staged tables, so the cases that differ in their form share it."""
    return _run(key + (-1, -1), {"raycast_variant": 2 if key[5] == 2 else 1})


def _check(case):
    kind, _cells, _k, envs, rays, _prec, env_order, _border, _pair_rows, _box = case
    ref = _reference(case[:6] + (0,) + case[7:8])
    # the rays do meet triangles (a 2.4 - 4 m map: the outer rings and most rays of a rover tilted by a radian leave it)
    assert (ref[1] < 11.0).mean() > 0.05 and (ref[2][0:6] < 11.0).mean() > 0.1
    got = _run(case, {"raycast_variant": 4, "lane_env_order": env_order, "lane_rocks": 1}, oracle=True)
    ci = got[3]
    print(f"{_id(case)}: form {got[4]}, rays {ci['rays']}, both tests {ci['rays_both_tests']}, bins {ci['bins']}, items {ci['lane_items']}, "
          f"pairs per ray {ci['pairs_per_ray']:.3f}")
    assert ci["rays"] == envs * (int(rays) + 26) and ci["candidate_pairs"] > 0
    for key in ref[0]:
        np.testing.assert_array_equal(got[0][key], ref[0][key], err_msg=f"{key} {_id(case)}")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"distances {_id(case)}")
    np.testing.assert_array_equal(got[2], ref[2], err_msg=f"crafted rays {_id(case)}")
    assert ci["lane_items"] == PARENT_LANE_ITEMS[_id(case)], "the item list is the one the two separate walks went over"
    return got


@pytest.mark.parametrize("case", TERRAIN, ids=_id)
def test_few_ab_items_beside_many_a_items(case):
    ci = _check(case)[3]
    assert 0 < ci["rays_both_tests"] < ci["rays"]


@pytest.mark.parametrize("case", IRREGULAR, ids=_id)
def test_many_ab_items_beside_few_a_items(case):
    ci = _check(case)[3]
    assert 2 * ci["rays_both_tests"] > ci["rays"], "most rays of the irregular mesh are off their cone"


@pytest.mark.parametrize("case", ENV_ORDER, ids=_id)
def test_env_order(case):
    got = _check(case)
    if case[0] == "mixed":
        assert got[4] == [1, 0], "grid terrain in box form over irregular rocks in sphere form: a wave walks its list once per form"
    assert got[3]["rays_both_tests"] > 0


@pytest.mark.parametrize("case", AS_SHIPPED, ids=_id)
def test_as_shipped(case):
    assert _check(case)[3]["rays_both_tests"] > 0


@pytest.mark.parametrize("case", FORMS, ids=_id)
def test_forms(case):
    got = _check(case)
    assert got[4] == [case[9], case[9]]
    assert got[3]["rays_both_tests"] > 0
