"""The Mars terrain generator without a GPU: the planner (terrain_gen.plan_mars_terrain) against what the reference's own generator produced
(tests/golden/mars_*.npz, recorded by tools/gen_mars_golden.py), the numpy restatement of rover_mars_heightfield (tests/mars_ref.py) against
the same recordings bit for bit, the mesh converter, the tile lists of rover_mars_tiles by brute force, the argument checks (all made before
the ctx is looked at) and the refusals."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mars_ref  # noqa: E402

from isaac_rover_amd import _lib, assets, terrain_gen  # noqa: E402

# the table of the issue: stamps planned per class, kept
COUNTS = {"A": ([156, 19, 4, 1], 178), "B": ([156, 19, 4, 1], 178), "C": ([39, 4, 1, 0], 44), "D": ([156, 19, 4, 1], 178)}


class _Recorder(random.Random):
    """random.Random that logs what uniform() and random() return, each call once (uniform is a + (b - a) * random())."""
    log = None

    def uniform(self, a, b):
        v = a + (b - a) * super().random()
        self.log.append(v)
        return v

    def random(self):
        v = super().random()
        self.log.append(v)
        return v


def _replan(name, monkeypatch=None):
    _, z = mars_ref.fixture(name)
    log = []
    if monkeypatch is not None:
        rec = type("Rec", (_Recorder,), {"log": log})
        monkeypatch.setattr(terrain_gen.random, "Random", rec)
    plan = terrain_gen.plan_mars_terrain(float(z["width"]), float(z["horizontal_scale"]), seed=int(z["seed"]),
                                         kernel_radius=float(z["kernel_radius"]), max_height=float(z["max_height"]))
    return plan, z, np.asarray(log, dtype=np.float64)


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and bool((np.sign(a) == np.sign(b)).all())
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max()) if a.size else 0


@pytest.mark.parametrize("name", mars_ref.FIXTURES)
def test_planner_halton_draws_and_tables(name, monkeypatch):
    plan, z, draws = _replan(name, monkeypatch)
    stored, _ = mars_ref.fixture(name)
    # Halton integers: the reference's scipy sampler, recorded
    assert np.array_equal(np.stack([plan.hill_rows, plan.hill_cols], axis=1), z["ref_halton_hills"])
    assert np.array_equal(np.stack([plan.stamp_rows, plan.stamp_cols], axis=1), z["ref_halton_rocks"])
    # every random draw, in count and in bits (the Mersenne Twister and a + (b - a) * random() are machine-independent)
    assert draws.shape == z["ref_draws"].shape
    assert np.array_equal(draws.view(np.int64), z["ref_draws"].view(np.int64))
    assert np.array_equal(plan.hill_amp.view(np.int64), stored.hill_amp.view(np.int64))
    assert np.array_equal(plan.stamp_factor.view(np.int64), stored.stamp_factor.view(np.int64))
    assert np.array_equal(plan.stamp_kept, stored.stamp_kept) and np.array_equal(plan.stamp_class, stored.stamp_class)
    # the tables go through this machine's exp(): within 4 ulp of the stored ones
    assert plan.side == stored.side and plan.hill_diameter == stored.hill_diameter
    assert _ulps(plan.g, stored.g) <= 4
    assert np.array_equal(plan.class_side, stored.class_side)
    for t, u in zip(plan.class_tables, stored.class_tables):
        assert _ulps(t, u) <= 4
    assert np.array_equal(plan.hill_windows(), mars_ref.hill_windows(stored))
    assert np.array_equal(plan.rocks, z["ref_rocks"])


@pytest.mark.parametrize("name", mars_ref.FIXTURES)
def test_restatement_reproduces_the_reference(name):
    plan, z = mars_ref.fixture(name)
    hf, mask = mars_ref.apply_plan(plan)
    assert z["ref_hf"].dtype == np.float64 and hf.shape == z["ref_hf"].shape == (plan.side, plan.side)
    assert np.array_equal(mars_ref.bits(hf), mars_ref.bits(z["ref_hf"]))
    assert z["ref_rocks"].dtype == np.float32 and np.array_equal(mars_ref.rocks_of(plan), z["ref_rocks"])
    per_class, kept = COUNTS[name]
    assert np.bincount(plan.stamp_class, minlength=4).tolist() == per_class
    assert int(plan.stamp_kept.sum()) == kept == len(z["ref_rocks"])
    assert int(mask.sum()) > 0
    # every hill of the fixtures is clipped somewhere, and all four sides occur
    w = mars_ref.hill_windows(plan)
    full = int(plan.hill_diameter) - 1
    assert bool((w[:, 0] == 0).any()) and bool((w[:, 1] == plan.side).any()) and bool((w[:, 2] == 0).any()) and bool((w[:, 3] == plan.side).any())
    assert bool((((w[:, 1] - w[:, 0]) < full) | ((w[:, 3] - w[:, 2]) < full)).any())


def test_save_and_load_round_trip(tmp_path):
    plan, _ = mars_ref.fixture("A")
    path = str(tmp_path / "plan.npz")
    plan.save(path)
    back = terrain_gen.MarsPlan.load(path)
    assert back.side == plan.side and back.horizontal_scale == plan.horizontal_scale
    for name in ("hill_rows", "hill_cols", "hill_amp", "g", "stamp_rows", "stamp_cols", "stamp_class", "stamp_factor", "stamp_kept", "rocks"):
        assert np.array_equal(getattr(back, name), getattr(plan, name)), name
    assert all(np.array_equal(a, b) for a, b in zip(back.class_tables, plan.class_tables))


def _variant(plan, z, consume_dropped=True, centre_fix=True):
    """The plan of case A dealt again from its seed, optionally WRONG: a dropped stamp that does not consume its draw; the centre
    fix-up of the class tables left out."""
    rng = random.Random(int(z["seed"]))
    mh = float(z["max_height"])
    amp = np.asarray([rng.uniform(-mh, mh) for _ in plan.hill_amp])
    scale = int(max(0.10, plan.horizontal_scale) / plan.horizontal_scale)
    tables, factor = [], np.zeros(len(plan.stamp_factor))
    for k in range(len(plan.class_side)):
        tables.append(terrain_gen.rock_table(k + 1, scale, rng.uniform(0.1, 0.2), centre_fix=centre_fix))
        for s in np.flatnonzero(plan.stamp_class == k):
            if consume_dropped or plan.stamp_kept[s]:
                factor[s] = rng.random() * 0.4 + 0.6
    return terrain_gen.MarsPlan(**{**plan.__dict__, "hill_amp": amp, "class_tables": tables, "stamp_factor": factor})


def test_wrong_variants_differ_from_the_reference():
    plan, z = mars_ref.fixture("A")
    want = mars_ref.bits(z["ref_hf"])
    same = _variant(plan, z)
    assert np.array_equal(same.stamp_factor.view(np.int64), plan.stamp_factor.view(np.int64))
    assert max(_ulps(t, u) for t, u in zip(same.class_tables, plan.class_tables)) <= 4
    # dealt again with nothing wrong (and the stored tables: the end-to-end comparisons do not depend on this machine's exp()) it is the reference
    redealt = terrain_gen.MarsPlan(**{**same.__dict__, "class_tables": plan.class_tables})
    assert np.array_equal(mars_ref.bits(mars_ref.apply_plan(redealt)[0]), want)
    assert not np.array_equal(mars_ref.bits(mars_ref.apply_plan(_variant(plan, z, consume_dropped=False))[0]), want)
    assert not np.array_equal(mars_ref.bits(mars_ref.apply_plan(_variant(plan, z, centre_fix=False))[0]), want)
    assert not np.array_equal(mars_ref.bits(mars_ref.apply_plan(plan, use_last=True)[0]), want)
    assert len(mars_ref.rocks_of(plan, record_dropped=True)) == len(plan.stamp_kept) == len(z["ref_rocks"]) + 2


def test_mesh_equals_the_reference():
    _, z = mars_ref.fixture("A")
    hs = float(z["horizontal_scale"])
    v0, t0 = terrain_gen.heightfield_to_trimesh(z["ref_hf"], hs)
    v1, t1 = terrain_gen.heightfield_to_trimesh(z["ref_hf"], hs, slope_threshold=1.5)
    assert v0.dtype == np.float32 and t0.dtype == np.int32
    assert np.array_equal(v0.view(np.uint32), z["ref_mesh_vertices"].view(np.uint32))
    assert np.array_equal(v1.view(np.uint32), z["ref_mesh_vertices_slope"].view(np.uint32))
    assert np.array_equal(t0, z["ref_mesh_triangles"]) and np.array_equal(t1, t0)
    assert int((v0 != v1).any(axis=1).sum()) >= 1
    # the diagonal of synth.grid_mesh
    from isaac_rover_amd import synth
    assert np.array_equal(terrain_gen.grid_triangles(7, 7), synth.grid_mesh(7)[1])


# ---- rover_mars_tiles ---------------------------------------------------------------------------------------------------------------------
def _brute_tiles(case):
    t = _lib.MARS_TILE
    tr, tc = -(-case["rows"] // t), -(-case["cols"] // t)
    sides = [x.shape[0] for x in case["class_tables"]]
    lists = []
    for ti in range(tr):
        for tj in range(tc):
            ids = []
            for s in range(len(case["stamp_row"])):
                if not case["stamp_kept"][s]:
                    continue
                r, c, n = int(case["stamp_row"][s]), int(case["stamp_col"][s]), sides[int(case["stamp_class"][s])]
                if r < (ti + 1) * t and r + n > ti * t and c < (tj + 1) * t and c + n > tj * t:
                    ids.append(s)
            lists.append(ids)
    return lists


def _tiles_touched(case):
    t = _lib.MARS_TILE
    sides = [x.shape[0] for x in case["class_tables"]]
    out = set()
    for r, c, k, ok in zip(case["stamp_row"], case["stamp_col"], case["stamp_class"], case["stamp_kept"]):
        if ok:
            n = sides[int(k)]
            out.add(int(((r + n - 1) // t - r // t + 1) * ((c + n - 1) // t - c // t + 1)))
    return out


TILE_CASES = {"squares": dict(seed=1, rows=64, cols=64, sides=(1, 3, 6, 17, 33), n_stamps=120, n_dropped=6),
              "ragged": dict(seed=2, rows=37, cols=53, sides=(1, 5, 17), n_stamps=60, n_dropped=3),
              "empty": dict(seed=3, rows=40, cols=40, n_stamps=0, n_dropped=0),
              "all_dropped": dict(seed=4, rows=33, cols=33, sides=(2, 4), n_stamps=0, n_dropped=5)}


@pytest.mark.parametrize("name", sorted(TILE_CASES))
def test_tile_lists_by_brute_force(name):
    case = mars_ref.random_case(**TILE_CASES[name])
    desc, keep = _lib.mars_desc(**case)
    start, items = _lib.mars_tiles(desc)
    want = _brute_tiles(case)
    assert len(start) == len(want) + 1 and start[0] == 0 and start[-1] == len(items) == sum(len(w) for w in want)
    for t, ids in enumerate(want):
        assert items[start[t]:start[t + 1]].tolist() == ids, t
    if name == "squares":
        assert {1, 2, 4, 9} <= _tiles_touched(case)
    if name in ("empty", "all_dropped"):
        assert len(items) == 0 and not start.any()


def test_tiles_capacity_and_nulls():
    lib = _lib.load()
    desc, keep = _lib.mars_desc(**mars_ref.random_case(5, 48, 48))
    n = C.c_int64(-1)
    assert lib.rover_mars_tiles(C.byref(desc), None, None, 0, C.byref(n)) == 0 and n.value > 0
    start, items = np.zeros(10, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
    assert lib.rover_mars_tiles(C.byref(desc), start.ctypes.data, items.ctypes.data, n.value - 1, C.byref(n)) == -1
    assert "capacity" in lib.rover_last_error(None).decode()
    assert lib.rover_mars_tiles(C.byref(desc), None, None, 0, None) == -1
    assert lib.rover_mars_tiles(None, None, None, 0, C.byref(n)) == -1
    assert lib.rover_last_error(None).decode().startswith("mars_tiles:")


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_exported():
    for name in ("rover_mars_heightfield", "rover_mars_tiles"):
        assert name in _lib.SYMBOLS
    _lib.build()
    _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"rover_mars_heightfield", "rover_mars_tiles"} <= exported
    assert os.path.exists(os.path.join(ROOT, "isaac_rover_2.0_amd", "csrc", "rover_mars.hip"))
    assert any(s.endswith("rover_mars.hip") for s in _lib._sources())


def _base(**kw):
    a = dict(rows=32, cols=40, hill_window=[[0, 8, 2, 10, 0, 0]], hill_amp=[1.0], g=np.ones(8), class_tables=[np.ones((3, 3)), np.ones((5, 5))],
             stamp_row=[1, 27], stamp_col=[2, 35], stamp_class=[0, 1], stamp_factor=[0.7, 0.9], stamp_kept=[1, 1])
    a.update(kw)
    return a


def _call(fields=None, hf=16, **kw):
    lib = _lib.load()
    desc, keep = _lib.mars_desc(**_base(**kw))
    for k, v in (fields or {}).items():
        setattr(desc, k, v)
    rc = lib.rover_mars_heightfield(None, C.byref(desc), hf, None, None)
    return rc, lib.rover_last_error(None).decode()


INVALID = {
    "rows=0": (dict(fields=dict(rows=0)), "rows"),
    "cols=0": (dict(fields=dict(cols=0)), "cols"),
    "rows=131073": (dict(fields=dict(rows=131073)), "rows"),
    "cols=131073": (dict(fields=dict(cols=131073)), "cols"),
    "n_hills<0": (dict(fields=dict(n_hills=-1)), "n_hills"),
    "n_stamps<0": (dict(fields=dict(n_stamps=-1)), "n_stamps"),
    "n_classes=17": (dict(class_tables=[np.ones((1, 1))] * 17), "n_classes"),
    "side=130": (dict(class_tables=[np.ones((130, 130))], rows=200, cols=200, stamp_class=[0, 0]), "class_side"),
    "g_len=0": (dict(fields=dict(g_len=0)), "g_len"),
    "g=NULL": (dict(fields=dict(g=None)), "g "),
    "stamp_past_last_row": (dict(stamp_row=[1, 28]), "stamp_row"),
    "stamp_past_last_col": (dict(stamp_col=[2, 36]), "stamp_col"),
    "stamp_row<0": (dict(stamp_row=[-1, 27]), "stamp_row"),
    "stamp_col<0": (dict(stamp_col=[-1, 35]), "stamp_col"),
    "class=2": (dict(stamp_class=[0, 2]), "stamp_class"),
    "class<0": (dict(stamp_class=[-1, 1]), "stamp_class"),
    "amp=nan": (dict(hill_amp=[float("nan")]), "hill_amp"),
    "amp=inf": (dict(hill_amp=[float("inf")]), "hill_amp"),
    "factor=nan": (dict(stamp_factor=[0.7, float("nan")]), "stamp_factor"),
    "factor=-inf": (dict(stamp_factor=[float("-inf"), 0.9]), "stamp_factor"),
    "window_past_rows": (dict(hill_window=[[25, 33, 2, 10, 0, 0]]), "hill_window"),
    "window_past_cols": (dict(hill_window=[[0, 8, 33, 41, 0, 0]]), "hill_window"),
    "window_reversed": (dict(hill_window=[[8, 0, 2, 10, 0, 0]]), "hill_window"),
    "window_past_g": (dict(hill_window=[[0, 8, 2, 10, 1, 0]]), "hill_window"),
    "window_before_g": (dict(hill_window=[[0, 8, 2, 10, 0, -1]]), "hill_window"),
    "hf=NULL": (dict(hf=None), "hf"),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_arguments_with_a_null_ctx(name):
    """Every ROVER_E_INVALID of the descriptor is reported before the ctx is looked at: a NULL ctx, no device, and a message that names
    the argument and not the ctx."""
    kw, word = INVALID[name]
    rc, msg = _call(**kw)
    assert rc == -1
    assert msg.startswith("mars_heightfield:") and word in msg and "null ctx" not in msg, msg


def test_valid_arguments_reach_the_ctx_check():
    # a dropped stamp is not looked at: it may overrun the field, name no class and hold no finite factor
    for kw in (dict(), dict(stamp_row=[1, 999], stamp_class=[0, 7], stamp_factor=[0.7, float("nan")], stamp_kept=[1, 0]),
               dict(hill_window=np.zeros((0, 6)), hill_amp=[]), dict(stamp_row=[], stamp_col=[], stamp_class=[], stamp_factor=[], stamp_kept=[]),
               dict(class_tables=[np.ones((129, 129))], rows=129, cols=129, stamp_row=[0], stamp_col=[0], stamp_class=[0], stamp_factor=[1.0],
                    stamp_kept=[1], hill_window=np.zeros((0, 6)), hill_amp=[]),
               dict(fields=dict(rows=131072, cols=1), hill_window=np.zeros((0, 6)), hill_amp=[], stamp_kept=[0, 0])):
        rc, msg = _call(**kw)
        assert rc == -1 and msg == "mars_heightfield: null ctx", msg
    lib = _lib.load()
    assert lib.rover_mars_heightfield(None, None, 16, None, None) == -1 and "desc" in lib.rover_last_error(None).decode()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_planner_refusals():
    with pytest.raises(ValueError, match="horizontal_scale"):
        terrain_gen.plan_mars_terrain(12.8, 0.2)
    with pytest.raises(ValueError, match="horizontal_scale"):
        terrain_gen.plan_mars_terrain(12.8, 0.1000001)
    for width in (0.0, -3.0):
        with pytest.raises(ValueError, match="width"):
            terrain_gen.plan_mars_terrain(width, 0.1)
    terrain_gen.plan_mars_terrain(12.8, 0.1, kernel_radius=3.0)       # the limit itself is accepted


class _HostEngine:
    """Stands in for Engine.mars_heightfield with tests/mars_ref.py."""

    def mars_heightfield(self, plan, rock_mask=True):
        hf, mask = mars_ref.apply_plan(plan)
        return torch.from_numpy(hf), torch.from_numpy(mask)


    def build_knn_map(self, vertices, triangles, n_x, n_y, res=0.1, k=200, ranking="exact_f32", cell_x_f16=None, cell_y_f16=None):
        from isaac_rover_amd import synth
        return synth.knn_map_bruteforce(np.asarray(vertices), np.asarray(triangles), n_x, n_y, k, res)

    def build_heightfield(self, vertices, triangles, n0, n1, horizontal_scale=0.025, shift=(0.0, 0.0), fill=0.0):
        import raster_ref
        hm, uncovered, skipped = raster_ref.build_heightfield(vertices, triangles, n0, n1, horizontal_scale, shift, fill)
        return torch.from_numpy(hm), uncovered, skipped


def test_build_scene_tool_generates_the_meshes(tmp_path, capsys):
    """tools/build_scene.py --mars SEED writes map.ply and big_stones.ply, then continues as for any two meshes."""
    import importlib.util
    sp = importlib.util.spec_from_file_location("build_scene_tool_mars", os.path.join(ROOT, "tools", "build_scene.py"))
    tool = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(tool)
    d = tmp_path / "terrain"
    assert tool.main([str(d), "--mars", "7", "--width", "3.2", "--cells", "32", "--k", "4", "--hscale", "0.05"], make_engine=_HostEngine) == 0
    assert "mars seed 7: 32^2 nodes" in capsys.readouterr().out
    plan = terrain_gen.plan_mars_terrain(3.2, 0.1, seed=7)
    hf, mask = mars_ref.apply_plan(plan)
    verts, tris = assets.load_ply(str(d / "map.ply"))
    want_v, want_t = terrain_gen.heightfield_to_trimesh(hf, 0.1)
    assert np.array_equal(verts.view(np.uint32), want_v.view(np.uint32)) and np.array_equal(tris, want_t)
    rock_v, rock_t = assets.load_ply(str(d / "big_stones.ply"))
    assert len(rock_t) == int((mask.reshape(-1) != 0)[want_t].any(axis=1).sum()) >= 4
    for name in ("knn_terrain/map_indices.pt", "knn_rocks/map_indices.pt", "heightmap_tensor.pt", "stone_info.npy"):
        assert (d / name).exists(), name


def test_scene_refuses_too_few_rock_triangles():
    with pytest.raises(ValueError, match=r"fewer than k = 200"):
        assets.build_mars_scene(_HostEngine(), seed=10, n_cells=32, k=200, width=3.2, kernel_radius=0.8, max_height=0.5)
    plan = terrain_gen.plan_mars_terrain(3.2, 0.1, kernel_radius=0.8, max_height=0.5)
    verts, tris, rock_tris = assets.mars_meshes(_HostEngine(), plan, k=4)
    mask = mars_ref.apply_plan(plan)[1].reshape(-1) != 0
    assert 4 <= len(rock_tris) < 200 and bool(mask[rock_tris].any(axis=1).all())
    assert len(rock_tris) == int(mask[tris].any(axis=1).sum())
