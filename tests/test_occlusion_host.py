"""CPU: the line-of-sight occlusion as DEFINED (tests/occlusion_ref.py) on hand-built fields where the answer is known without it, the
column order of rover_occlusion_order, every refusal of rover_obs_occlusion and rover_set_occlusion that needs no device (the C layer
validates before it looks at the ctx, so a NULL ctx will do) and HeightmapOcclusion's own checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import occlusion_ref as R

F32 = np.float32
INFO = {"proprioceptive": 4, "sparse": 20, "dense": 30, "actions": 2}
IDENT = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=F32)
H_S = 0.025                                              # node spacing of the hand-built fields
CAM_UP = 0.7


def test_symbols_declared_and_exported():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for name in ("rover_set_occlusion", "rover_obs_occlusion", "rover_occlusion_order"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert [f for f, _ in _lib.OcclusionCfg._fields_] == ["camera", "step", "clearance", "max_steps", "miss"]
    assert [f for f, _ in _lib.ObsOcclusionDesc._fields_] == ["pos3", "quat4", "clean", "clean_stride", "in_", "in_stride", "out", "out_stride", "M", "F",
                                                              "first", "drop_value", "hidden_u8", "hidden_stride", "target3"]


# ---- hand-built scenes: identity attitude, the rover at (px, py, ride), flat ground at 0, body points on the x axis -------------------
def _flat(nodes=400):
    return np.zeros((nodes, nodes), dtype=F32)


def _scene(bx, px=2.0, py=5.0, ride=0.35, bz=-0.25):
    """Body points (bx_i, 0, bz), one env at (px, py, ride) with the identity attitude, clean such that every target lies at z = 0
    exactly: S_z = ride + bz in f32, v = S_z / 2, d = 2 v = S_z, T_z = S_z - S_z."""
    body = np.array([[b, 0.0, bz] for b in bx], dtype=F32)
    pos = np.array([[px, py, ride]], dtype=F32)
    sz = pos[0, 2] + ((F32(0) * body[:, 0] + F32(0) * body[:, 1]) + F32(1) * body[:, 2])
    clean = (sz * F32(0.5))[None, :]
    return body, pos, clean


def _line_at_node(pos, body_x, wall_ix, step=0.05, clearance=0.03):
    """The definition for ONE column of _scene, written out in scalar float32: -> (n, the smallest (Cam_z + t dz) + clearance among the
    samples whose x node is wall_ix or wall_ix + 1, or None when no sample lands there)."""
    camx, camz = pos[0, 0] + F32(0.0), pos[0, 2] + F32(CAM_UP)
    tx = pos[0, 0] + F32(body_x)
    dx, dz = tx - camx, F32(0.0) - camz
    u = np.ceil(np.sqrt(dx * dx + F32(0.0)) / F32(step))
    n = int(u)
    best = None
    for k in range(1, n):
        t = F32(k) / F32(n)
        if int(np.rint((camx + t * dx) / F32(H_S))) in (wall_ix, wall_ix + 1):
            line = (camz + t * dz) + F32(clearance)
            best = line if best is None or line < best else best
    return n, best


def test_flat_ground_hides_nothing():
    body, pos, clean = _scene(np.linspace(0.3, 3.3, 40))
    o = R.occlude(R.Field(_flat(), H_S), body, pos, IDENT, clean)
    assert not o["hidden"].any() and o["has_point"].all() and np.array_equal(R.bits(o["out"]), R.bits(clean))
    assert np.array_equal(o["target"][0, :, 2], np.zeros(40, dtype=F32)) and np.array_equal(o["target"][0, :, 0], pos[0, 0] + body[:, 0])
    assert float(o["margin"].min()) >= 0.03                                        # the line ends at the ground: never below the clearance


def test_wall_between_camera_and_target_at_the_threshold():
    """A wall two nodes thick at x = 3.0 m (nodes 120 and 121: 0.05 m, so that no line steps over it), 1 m in front of the camera.  A
    farther target's line passes the wall higher: the wall hides exactly the targets whose line, plus the clearance, is below its top at
    one of the line's samples there.  Both sides of one column's threshold, one ulp apart in the wall's height."""
    bx = np.array([1.3, 1.5, 1.7, 2.0, 2.3, 2.6, 2.9, 3.2], dtype=F32)               # targets at 3.3 .. 5.2 m: all beyond the wall
    body, pos, clean = _scene(bx)
    wall = 120
    lines = [_line_at_node(pos, b, wall)[1] for b in bx]
    assert all(v is not None for v in lines) and lines[0] < lines[2] < lines[5] < lines[7]         # every line meets the wall; farther = higher
    for pick in (2, 5):
        for top, hides_pick in ((lines[pick], False), (np.nextafter(lines[pick], F32(np.inf)), True)):
            hm = _flat()
            hm[wall:wall + 2, :] = top
            o = R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean, drop_value=-1.0)
            want = np.array([top > v for v in lines])
            assert want[pick] == hides_pick and want[0] and not want[7]
            assert np.array_equal(o["hidden"][0].astype(bool), want), (pick, top)
            assert np.array_equal(o["out"][0], np.where(want, F32(-1.0), clean[0]))
            assert (o["margin"][0, pick] < 0) == hides_pick and (hides_pick or o["margin"][0, pick] == 0)


def test_wall_beyond_the_target_hides_nothing():
    body, pos, clean = _scene(np.array([0.4, 0.8, 1.2, 1.6], dtype=F32))             # targets up to x = 3.6 m
    hm = _flat()
    hm[150:154, :] = 3.0                                                               # x = 3.75 m and beyond
    o = R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)
    assert not o["hidden"].any()
    hm[100:104, :] = 3.0                                                               # ... and the same wall at x = 2.5 m: behind the first target, in front of the others
    assert R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)["hidden"][0].tolist() == [0, 1, 1, 1]


def test_miss_and_nan_pass_through():
    body, pos, clean = _scene(np.full(6, 2.0, dtype=F32))
    hm = _flat()
    hm[100:104, :] = 3.0                                                               # hides every column that has a point
    clean = np.tile(clean, (1, 1))
    clean[0, 1], clean[0, 2], clean[0, 3], clean[0, 4] = 5.0, -5.0, np.nan, np.nextafter(F32(5.0), F32(0.0))
    noisy = clean + F32(0.125)
    o = R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean, in_=noisy, drop_value=7.0)
    assert o["hidden"][0].tolist() == [1, 0, 0, 0, 1, 1] and o["has_point"][0].tolist() == [True, False, False, False, True, True]
    assert o["n"][0, 1:4].tolist() == [0, 0, 0] and np.isnan(o["target"][0, 1:4]).all()
    assert np.array_equal(R.bits(o["out"][0, 1:4]), R.bits(noisy[0, 1:4])) and (o["out"][0, [0, 4, 5]] == 7.0).all()


def test_interval_count_at_an_integer_and_one_ulp_above():
    """step = 0.25 (exact): with the rover at x = 0 the line's length is the body point's x; 2.0 / 0.25 = 8 exactly, one ulp more gives 9."""
    up = np.nextafter(F32(2.0), F32(3.0))
    assert np.sqrt(up * up + F32(0.0)) > F32(2.0) and np.sqrt(F32(2.0) * F32(2.0)) == F32(2.0)
    body, pos, clean = _scene(np.array([2.0, up, 0.25, np.nextafter(F32(0.25), F32(0.0)), 0.5], dtype=F32), px=0.0)
    o = R.occlude(R.Field(_flat(), H_S), body, pos, IDENT, clean, step=0.25)
    assert o["n"][0].tolist() == [8, 9, 1, 1, 2]
    assert np.isinf(o["margin"][0, 2:4]).all() and np.isfinite(o["margin"][0, 4])     # n <= 1: no sample, visible
    assert _line_at_node(pos, 2.0, 0, step=0.25)[0] == 8


def test_max_steps_reached():
    body, pos, clean = _scene(np.array([3.0, 0.79, 0.81], dtype=F32))
    o = R.occlude(R.Field(_flat(), H_S), body, pos, IDENT, clean, max_steps=16)        # 3.0 / 0.05 = 60 intervals wanted
    assert o["n"][0].tolist() == [16, 16, 16]
    assert R.occlude(R.Field(_flat(), H_S), body, pos, IDENT, clean, max_steps=17)["n"][0].tolist() == [17, 16, 17]
    hm = _flat()
    hm[143:145, :] = 3.0                              # x = 3.575 and 3.6 m: the 16 coarse samples of the first column (every 0.1875 m) step over both nodes
    xs = [int(np.rint((pos[0, 0] + F32(k) / F32(16) * (body[0, 0])) / F32(H_S))) for k in range(1, 16)]
    assert 143 not in xs and 144 not in xs and 140 in xs
    assert R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean, max_steps=16)["hidden"][0, 0] == 0
    assert R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean, max_steps=256)["hidden"][0, 0] == 1


def test_camera_outside_the_map_is_clamped():
    """The rover 2 m outside the map's low-x edge, looking in: every sample left of the edge reads node row 0."""
    body, pos, clean = _scene(np.array([2.5, 3.0], dtype=F32), px=-2.0)
    hm = _flat()
    assert not R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)["hidden"].any()
    hm[0, :] = 2.0
    assert R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)["hidden"].all()
    hm[0, :] = 0.0
    hm[1:3, :] = 2.0                                   # nodes 1 and 2 cover x in [0.0125, 0.0625]: the edge clamp cannot reach them, a sample inside can
    o = R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)
    want = [_line_at_node(pos, b, 1)[1] is not None for b in body[:, 0]]
    assert o["hidden"][0].astype(bool).tolist() == want
    body, pos, clean = _scene(np.array([1.0], dtype=F32), px=2.0, py=-30.0)            # y far outside: iy clamps to 0 on a narrow map
    hm = np.zeros((400, 8), dtype=F32)
    hm[100:104, 0] = 3.0
    assert R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)["hidden"][0, 0] == 1
    hm[100:104, 0], hm[100:104, 1:] = 0.0, 3.0
    assert R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)["hidden"][0, 0] == 0


def test_nan_node_never_hides():
    body, pos, clean = _scene(np.array([1.5, 2.5], dtype=F32))
    hm = _flat()
    hm[100:104, :] = np.nan
    o = R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)
    assert not o["hidden"].any() and np.isfinite(o["margin"]).all()
    hm[110, :] = 3.0
    assert R.occlude(R.Field(hm, H_S), body, pos, IDENT, clean)["hidden"].all()


# ---- the column order -------------------------------------------------------------------------------------------------------------------
def _distributions():
    from isaac_rover_amd import synth
    from isaac_rover_amd.tasks.utils.heightmap_distribution import generate_native
    return {"native": generate_native(), "37": synth.ray_distribution("37")}


@pytest.mark.parametrize("name", ["native", "37"])
@pytest.mark.parametrize("camera", [(0.0, 0.0, 0.7), (0.3, -0.2, 1.0)])
def test_order_is_a_stable_far_first_permutation(name, camera):
    from isaac_rover_amd import _lib
    pts, sp, de = _distributions()[name]
    got = _lib.occlusion_order(pts, sp, de, camera)
    c = len(sp) + len(de)
    assert got.dtype == np.int32 and sorted(got.tolist()) == list(range(c))
    b = R.body_points(pts, sp, de).astype(np.float64)
    cam = np.asarray(camera, dtype=F32).astype(np.float64)
    key = ((b[:, 0] - cam[0]) ** 2 + (b[:, 1] - cam[1]) ** 2)[got]
    assert (np.diff(key) <= 0).all()                                                   # far first
    ties = np.diff(key) == 0
    assert (np.diff(got)[ties] > 0).all()                                              # equal distances keep their column order
    if tuple(camera[:2]) == (0.0, 0.0):
        assert ties.sum() > 0                                                          # (both distributions are symmetric in y: the stable rule is exercised)
    assert np.array_equal(got, R.order(pts, sp, de, camera))


def test_order_refusals():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    pts = np.zeros((4, 3)); idx = np.arange(4, dtype=np.int64); cam = np.zeros(3, dtype=F32); out = np.zeros(8, dtype=np.int32)
    P = lambda a: a.ctypes.data
    bad_idx, nan_cam = np.array([0, 4], dtype=np.int64), np.array([0, np.nan, 0], dtype=F32)
    for args in ((None, 4, P(idx), 4, None, 0, P(cam), P(out)), (P(pts), 0, P(idx), 4, None, 0, P(cam), P(out)), (P(pts), 4, None, 4, None, 0, P(cam), P(out)),
                 (P(pts), 4, P(idx), 4, None, 2, P(cam), P(out)), (P(pts), 4, P(idx), -1, None, 0, P(cam), P(out)), (P(pts), 4, P(idx), 4, None, 0, None, P(out)),
                 (P(pts), 4, P(idx), 4, None, 0, P(cam), None), (P(pts), 4, P(bad_idx), 2, None, 0, P(cam), P(out)), (P(pts), 4, P(idx), 4, None, 0, P(nan_cam), P(out))):
        assert lib.rover_occlusion_order(*args) == -1 and lib.rover_last_error(None).decode().startswith("occlusion_order:"), args
    assert lib.rover_occlusion_order(P(pts), 4, P(idx), 2, P(idx), 4, P(cam), P(out)) == 0 and out[:6].tolist() == [0, 1, 2, 3, 4, 5]
    assert _lib.occlusion_order(pts, [], []).shape == (0,)


def test_lane_slot_ratio_falls_under_the_order():
    """The property the order exists for: with the columns far first a wave of 64 lanes spends fewer lane-slots per useful sample than in
    obs order (the n are the restatement's, on a seeded case with the native distribution)."""
    pts, sp, de = _distributions()["native"]
    body = R.body_points(pts, sp, de)
    field = R.make_field(0)
    case = R.make_case(field, body, 8, seed=0)
    n = R.occlude(field, body, case["pos"], case["quat"], case["clean"], first=4)["n"]
    ident, ordered = R.lane_slot_ratio(n), R.lane_slot_ratio(n, R.order(pts, sp, de))
    print(f"lane-slots per useful sample: obs order {ident:.3f}, far first {ordered:.3f}")
    assert 1.0 <= ordered < ident
    assert R.lane_slot_ratio(n, np.arange(n.shape[1])) == ident


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------------
def _rc(d):
    from isaac_rover_amd import _lib
    lib = _lib.load()
    rc = lib.rover_obs_occlusion(None, None if d is None else C.byref(d), None)
    return rc, lib.rover_last_error(None).decode()


def test_obs_occlusion_refusals_without_a_device():
    from isaac_rover_amd import _lib
    D = _lib.obs_occlusion_desc
    inf, nan, A, B, K = float("inf"), float("nan"), 1 << 20, 1 << 30, 1 << 40     # fake bases far apart; 8 rows of 10 floats take 320 bytes
    need = "pos3, quat4, clean, in and out"
    bad = {
        "null descriptor": (None, "null descriptor"),
        "M < 0": (D(-1, 10, 4), "negative"), "F < 0": (D(8, -1, 0), "negative"),
        "first < 0": (D(8, 10, -1), "first"), "first > F": (D(8, 10, 11), "first"),
        "drop_value inf": (D(8, 10, 4, drop_value=inf), "drop_value"), "drop_value nan": (D(8, 10, 4, drop_value=nan), "drop_value"),
        "null pos3": (D(8, 10, 4, pos3=None), need), "null quat4": (D(8, 10, 4, quat4=None), need), "null clean": (D(8, 10, 4, clean=None), need),
        "null in": (D(8, 10, 4, in_=None), need), "null out": (D(8, 10, 4, out=None), need),
        "clean stride": (D(8, 10, 4, clean_stride=9), "row stride"), "in stride": (D(8, 10, 4, in_stride=9), "row stride"),
        "out stride": (D(8, 10, 4, out_stride=9), "row stride"), "hidden stride": (D(8, 10, 4, hidden_u8=K, hidden_stride=5), "row stride"),
        "out is clean": (D(8, 10, 4, clean=A, in_=B, out=A), "out overlaps clean"),
        "out is clean is in": (D(8, 10, 4, clean=A, in_=A, out=A), "out overlaps clean"),
        "out in clean's last row": (D(8, 10, 4, clean=A, in_=B, out=A + 4 * 79), "out overlaps clean"),
        "out shifted from in": (D(8, 10, 4, clean=A, in_=B, out=B + 4, in_stride=12, out_stride=12), "out overlaps in"),
        "out is in, other stride": (D(8, 10, 4, clean=A, in_=B, out=B, in_stride=10, out_stride=12), "out overlaps in"),
        "out over pos3": (D(8, 10, 4, pos3=K + 4 * 23, out=K), "out overlaps pos3"), "out over quat4": (D(8, 10, 4, quat4=K + 4 * 79, out=K), "out overlaps quat4"),
        "hidden in out": (D(8, 10, 4, out=K, hidden_u8=K + 319), "hidden_u8 overlaps out"),
        "target in out": (D(8, 10, 4, out=K, target3=K - 4 * 8 * 18 + 4), "target3 overlaps out"),
        "target over hidden": (D(8, 10, 4, hidden_u8=K, target3=K + 47), "target3 overlaps hidden_u8"),
    }
    for what, (d, word) in bad.items():
        rc, msg = _rc(d)
        assert rc == -1 and msg.startswith("obs_occlusion:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    ok = [D(8, 10, 4), D(8, 10, 4, clean=A, in_=A, out=B), D(8, 10, 4, clean=A, in_=B, out=B), D(8, 10, 4, clean=A, in_=B, out=B, in_stride=12, out_stride=12),
          D(8, 10, 4, clean=A, in_=B, out=A + 4 * 80), D(8, 10, 0), D(8, 10, 10), D(8, 10, 4, out=K, hidden_u8=K + 320, target3=K - 4 * 8 * 18),
          D(8, 10, 4, hidden_u8=K, hidden_stride=6, target3=K + 48), D(8, 10, 4, drop_value=-5.0),
          D(0, 10, 4, pos3=None, quat4=None, clean=None, in_=None, out=None), D(8, 0, 0, pos3=None, quat4=None, clean=None, in_=None, out=None)]
    for i, d in enumerate(ok):
        rc, msg = _rc(d)
        assert rc == -1 and msg == "obs_occlusion: null ctx", (i, rc, msg)          # past every check of the descriptor


def test_set_occlusion_refusals_without_a_device():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    inf, nan = float("inf"), float("nan")
    call = lambda cfg: (lib.rover_set_occlusion(None, None if cfg is None else C.byref(cfg)), lib.rover_last_error(None).decode())
    K = _lib.occlusion_cfg
    bad = {"null cfg": (None, "null cfg"), "camera nan": (K(camera=(0.0, nan, 0.7)), "finite"), "camera inf": (K(camera=(inf, 0.0, 0.7)), "finite"),
           "step nan": (K(step=nan), "finite"), "step inf": (K(step=inf), "finite"), "step 0": (K(step=0.0), "step"), "step < 0": (K(step=-0.05), "step"),
           "clearance nan": (K(clearance=nan), "finite"), "clearance inf": (K(clearance=-inf), "finite"), "max_steps 1": (K(max_steps=1), "max_steps"),
           "max_steps 4097": (K(max_steps=4097), "max_steps"), "max_steps < 0": (K(max_steps=-5), "max_steps"), "miss 0": (K(miss=0.0), "miss"),
           "miss < 0": (K(miss=-5.0), "miss"), "miss nan": (K(miss=nan), "finite"), "miss inf": (K(miss=inf), "finite")}
    for what, (cfg, word) in bad.items():
        rc, msg = call(cfg)
        assert rc == -1 and msg.startswith("set_occlusion:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    for cfg in (K(), K(clearance=-0.5), K(max_steps=2), K(max_steps=4096), K(camera=(-1.0, 2.0, -3.0), step=1e-3, miss=1e-6)):
        assert call(cfg) == (-1, "set_occlusion: null ctx")
    with pytest.raises(_lib.RoverError):
        K(camera=(0.0, 0.7))


def test_heightmap_occlusion_constructor_and_state_dict_on_cpu():
    from isaac_rover_amd.learning.noise import HeightmapOcclusion
    nan, inf = float("nan"), float("inf")
    for kw in (dict(camera=(0.0, 0.7)), dict(camera=(0.0, nan, 0.7)), dict(step=0.0), dict(step=-1.0), dict(step=nan), dict(clearance=inf), dict(max_steps=1),
               dict(max_steps=4097), dict(max_steps=2.5), dict(miss=0.0), dict(miss=nan), dict(drop_value=inf), dict(drop_value=nan)):
        with pytest.raises(ValueError):
            HeightmapOcclusion(None, INFO, **kw)
    with pytest.raises(KeyError):
        HeightmapOcclusion(None, {"sparse": 20, "dense": 30})
    a = HeightmapOcclusion(None, INFO)
    assert (a.camera, a.step, a.clearance, a.max_steps, a.miss, a.drop_value) == ((0.0, 0.0, 0.7), 0.05, 0.03, 256, 5.0, 0.0) and a.columns == 50
    for call in (lambda: a.apply(torch.zeros(5, 54)), a.configure):
        with pytest.raises(RuntimeError):
            call()
    b = HeightmapOcclusion(None, INFO, camera=(0.1, -0.2, 0.9), step=0.1, clearance=0.0, max_steps=64, miss=4.0, drop_value=-1.0)
    sd = b.state_dict()
    assert list(sd) == ["camera", "step", "clearance", "max_steps", "miss", "drop_value"]                # the parameters only: no counters
    a.load_state_dict(sd)
    assert a.state_dict() == sd and a.camera == (0.1, -0.2, 0.9) and a.max_steps == 64
    sd.pop("miss")
    with pytest.raises(KeyError):
        a.load_state_dict(sd)
