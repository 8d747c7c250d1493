"""GPU: rover_mars_heightfield (csrc/rover_mars.hip) against the numpy restatement of its definition (tests/mars_ref.py), bit for bit: the
four recordings of the reference's own generator (tests/golden/mars_*.npz) from their stored plans, seeded random plans at the shapes
where a tiled gather can go wrong, determinism, and a whole scene from one seed (assets.build_mars_scene) under a fused step."""
import numpy as np
import pytest
import torch

import mars_ref
from conftest import assert_step_close
from hip_helpers import _oracle_maps, hip_step, make_engine

from isaac_rover_amd import _lib, assets, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(1, device=0)
    yield e
    e.close()


def check(eng, hf, mask, want_hf, want_mask):
    assert hf.dtype == torch.float64 and hf.is_cuda and tuple(hf.shape) == want_hf.shape
    assert mask.dtype == torch.uint8 and mask.is_cuda and tuple(mask.shape) == want_mask.shape
    got = hf.cpu().numpy()
    diff = np.argwhere(mars_ref.bits(got) != mars_ref.bits(want_hf))
    assert len(diff) == 0, f"{len(diff)} nodes differ, first {diff[0]}: {got[tuple(diff[0])]!r} != {want_hf[tuple(diff[0])]!r}"
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    return got


@pytest.mark.parametrize("name", mars_ref.FIXTURES)
def test_fixtures_bit_for_bit(eng, name):
    """From the plan stored next to the recording (its tables were made where the recording was made: no dependence on this machine's
    exp()) the kernel gives the reference's heightfield, to the bit."""
    plan, z = mars_ref.fixture(name)
    want_hf, want_mask = mars_ref.apply_plan(plan)
    hf, mask = eng.mars_heightfield(plan)
    got = check(eng, hf, mask, want_hf, want_mask)
    assert np.array_equal(mars_ref.bits(got), mars_ref.bits(z["ref_hf"]))
    again, mask2 = eng.mars_heightfield(plan)
    assert torch.equal(again.view(torch.int64), hf.view(torch.int64)) and torch.equal(mask2, mask)      # the same bits on every run


def _one_stamp(rows, cols, side, row=0, col=0, seed=0):
    rng = np.random.default_rng(seed)
    return dict(rows=rows, cols=cols, hill_window=np.zeros((0, 6), dtype=np.int32), hill_amp=[], g=[1.0], class_tables=[rng.random((side, side)) + 0.1],
                stamp_row=[row], stamp_col=[col], stamp_class=[0], stamp_factor=[0.8125], stamp_kept=[True])


def _borders(rows=37, cols=53):
    """Stamps of three sizes flush with all four borders and in all four corners, on top of clipped hills."""
    case = mars_ref.random_case(11, rows, cols, n_hills=4, g_len=40, sides=(1, 4, 17), n_stamps=0, n_dropped=0)
    sr, sc, sk = [], [], []
    for k, s in enumerate((1, 4, 17)):
        for r, c in ((0, 0), (0, cols - s), (rows - s, 0), (rows - s, cols - s), (0, 20), (rows - s, 9), (13, 0), (7, cols - s)):
            sr.append(r), sc.append(c), sk.append(k)
    rng = np.random.default_rng(12)
    case.update(stamp_row=np.asarray(sr, dtype=np.int32), stamp_col=np.asarray(sc, dtype=np.int32), stamp_class=np.asarray(sk, dtype=np.int32),
                stamp_factor=rng.uniform(0.6, 1.0, len(sr)), stamp_kept=np.ones(len(sr), dtype=bool))
    return case


def _pile(n=300):
    """``n`` stamps that all cover node (20, 21): one tile's list runs through several LDS chunks; the sum depends on the order."""
    case = mars_ref.random_case(13, 48, 40, n_hills=2, sides=(1, 3, 6), n_stamps=0, n_dropped=0)
    rng = np.random.default_rng(14)
    sk = rng.integers(0, 3, n)
    side = np.asarray([1, 3, 6])[sk]
    sr = 20 - rng.integers(0, side)
    sc = 21 - rng.integers(0, side)
    case.update(stamp_row=sr.astype(np.int32), stamp_col=sc.astype(np.int32), stamp_class=sk.astype(np.int32), stamp_factor=rng.uniform(0.6, 1.0, n),
                stamp_kept=rng.random(n) > 0.05)
    return case


def _long_g():
    """A hill table longer than the field's side: windows start deep inside g."""
    case = mars_ref.random_case(15, 20, 24, n_hills=0, n_stamps=10)
    case.update(g=np.random.default_rng(16).random(300) + 0.2, hill_amp=np.asarray([-1.5, 0.75, -0.25]),
                hill_window=np.asarray([[0, 20, 0, 24, 270, 3], [3, 19, 5, 24, 0, 281], [10, 20, 0, 7, 150, 149]], dtype=np.int32))
    return case


CASES = {
    "one_17x17_stamp_fills_17x17": lambda: _one_stamp(17, 17, 17),
    "rectangle_37x53": lambda: mars_ref.random_case(21, 37, 53, n_hills=5, g_len=30, sides=(1, 3, 6, 17), n_stamps=80, n_dropped=5),
    "borders_and_corners": _borders,
    "pile_of_300": _pile,
    "no_stamps": lambda: mars_ref.random_case(22, 50, 34, n_hills=6, n_stamps=0, n_dropped=0),
    "no_hills": lambda: mars_ref.random_case(23, 33, 65, n_hills=0, n_stamps=60),
    "nothing_at_all": lambda: mars_ref.random_case(24, 16, 16, n_hills=0, n_stamps=0, n_dropped=0),
    "long_hill_table": _long_g,
    "negative_amplitudes": lambda: dict(mars_ref.random_case(25, 64, 48, n_hills=8, n_stamps=30), hill_amp=-np.linspace(0.5, 3.0, 8)),
    "one_node": lambda: _one_stamp(1, 1, 1),
    "largest_table": lambda: _one_stamp(140, 131, 129, row=11, col=2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_plans_bit_for_bit(eng, name):
    case = CASES[name]()
    want_hf, want_mask = mars_ref.apply_case(case)
    desc, keep = _lib.mars_desc(**case)
    hf, mask = eng.mars_heightfield(desc)
    check(eng, hf, mask, want_hf, want_mask)
    if name == "pile_of_300":
        start, items = _lib.mars_tiles(desc)
        assert int(np.diff(start).max()) > 2 * 128                  # more than two LDS chunks in one tile
        assert int(want_mask.sum()) >= 36
    if name == "nothing_at_all":
        assert not want_hf.any() and not want_mask.any()
    again, _ = eng.mars_heightfield(desc, rock_mask=False)
    assert _ is None and torch.equal(again.view(torch.int64), hf.view(torch.int64))


def test_refusal_through_the_engine(eng):
    case = _one_stamp(16, 16, 3, row=14, col=0)
    desc, keep = _lib.mars_desc(**case)
    with pytest.raises(_lib.RoverError, match="mars_heightfield: stamp 0"):
        eng.mars_heightfield(desc)


def test_scene_from_one_seed():
    """assets.build_mars_scene: the terrain map's vertices are the fp16 rounding of the generated nodes, every recorded rock lies inside a
    stone's bounding box, and one fused step of 256 envs on the scene agrees with the CPU oracle under conftest's tolerances."""
    from oracle import oracle as orc
    from isaac_rover_amd import terrain_gen
    e, cells = 256, 128
    eng = _lib.Engine(e, device=0)
    scene, plan = assets.build_mars_scene(eng, seed=10, n_cells=cells, k=16, width=12.8)
    stored, z = mars_ref.fixture("A")
    assert plan.side == cells and np.array_equal(plan.rocks, z["ref_rocks"])
    hf, _ = mars_ref.apply_plan(plan)
    verts, tris = terrain_gen.heightfield_to_trimesh(hf, 0.1)
    v16 = torch.from_numpy(verts).to(torch.float16)
    assert scene.terrain.vertices.dtype == torch.float16 and torch.equal(scene.terrain.vertices.view(torch.int16), v16.view(torch.int16))
    assert np.array_equal(scene.terrain.triangles.numpy(), tris)
    assert tuple(scene.terrain.map_indices.shape) == (cells, cells, 16) and tuple(scene.rocks.map_indices.shape) == (cells, cells, 16)
    assert tuple(scene.heightmap.shape) == (cells * 4, cells * 4) and scene.vertical_scale == 1.0
    # stone rows: [bbox centre x, y, min z, 2 width x, 2 width y, height]
    s = scene.stone_info_raw
    for x, y, _z, _r in plan.rocks.astype(np.float64):
        inside = (np.abs(x - s[:, 0]) <= s[:, 3] / 4 + 1e-6) & (np.abs(y - s[:, 1]) <= s[:, 4] / 4 + 1e-6)
        assert bool(inside.any()), (x, y)
    eng.close()
    distn = synth.ray_distribution("37")
    st = synth.make_states(e, cells * 0.1, seed=9)
    want = orc.step(*_oracle_maps(scene), st, *distn)
    step_eng = make_engine(scene, distn, e)
    got = hip_step(step_eng, st)
    assert_step_close(got, {"out_" + k: v for k, v in want.items()}, "mars scene")
    for k in ("rock_collision", "reset_buf", "progress_buf"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    step_eng.close()
