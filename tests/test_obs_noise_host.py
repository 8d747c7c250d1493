"""CPU: the exteroception noise as DEFINED (tests/obs_noise_ref.py) — its counter layouts pinned through the library's host Philox, its
dropout threshold, its statistics and its error bound —, every refusal of rover_obs_noise (the C layer validates the descriptor
before it looks at the ctx, so a NULL ctx will do) and HeightmapNoise's constructor and state_dict.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import gauss_ref as G
import obs_noise_ref as R

N_STAT = 1 << 17
INFO = {"proprioceptive": 4, "sparse": 20, "dense": 30, "actions": 2}


def test_symbol_declared_and_exported():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for name in ("rover_obs_noise", "rover_obs_noise_threshold"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert [f for f, _ in _lib.ObsNoiseDesc._fields_] == ["in_", "in_stride", "out", "out_stride", "M", "F", "first", "sigma_point", "sigma_offset",
                                                          "dropout", "drop_value", "row_scale", "episode", "seed", "step", "step_dev", "row_offset"]


def test_counter_layouts_match_the_library_philox():
    """The restatement's two counter layouts, word for word, against rover_philox4x32 — g = 2^32 - 1, t and e past 2^32 included."""
    from isaac_rover_amd import _lib
    seed = 0x9E3779B97F4A7C15
    key = (seed & 0xffffffff, seed >> 32)
    for g, t, p in ((0, 0, 0), (1, 1, 1), (2 ** 32 - 1, 7, 3), (12345, 2 ** 32, 872), (2 ** 32 - 1, 2 ** 64 - 1, 2 ** 20 - 1), (77, 2 ** 40 + 5, 0)):
        w = R.point_words(seed, t, [g], p + 1)
        assert tuple(int(v[0, p]) for v in w) == _lib.philox4x32((g, t & 0xffffffff, t >> 32, 0x60000000 | p), key), (g, t, p)
        e = t if t < 2 ** 63 else t - 2 ** 64                                   # the episode count is an int64 taken mod 2^64
        wo = R.offset_words(seed, e, [g])
        assert tuple(int(v[0]) for v in wo) == _lib.philox4x32((g, t & 0xffffffff, t >> 32, 0x70000000), key), (g, t)
    # the streams are disjoint under one seed: word 3 separates them from the goal draws (0) and the action noise (0x50000000 | pair)
    assert (R.WORD3_POINT | (2 ** 20 - 1)) < R.WORD3_OFFSET and R.WORD3_POINT > (0x50000000 | 0xfffffff)


def test_dropout_threshold():
    from isaac_rover_amd import _lib
    assert _lib.obs_noise_threshold(0.0) == 0 == R.threshold(0.0)
    assert _lib.obs_noise_threshold(1.0) == 2 ** 24 == R.threshold(1.0)
    want = int(np.rint(0.1 * 2 ** 24))                                          # llrint rounds as np.rint does: to nearest, ties to even
    assert _lib.obs_noise_threshold(0.1) == want == R.threshold(0.1) == 1677722
    for p in (0.5, 2.0 ** -25, 3.0 * 2.0 ** -25, 1.0 - 2.0 ** -26):             # 2^-25 2^24 = 0.5 -> 0 and 1.5 -> 2: ties to even
        assert _lib.obs_noise_threshold(p) == R.threshold(p)
    assert (R.threshold(2.0 ** -25), R.threshold(3.0 * 2.0 ** -25)) == (0, 2)
    lib = _lib.load()
    out = C.c_uint32()
    for bad in (-0.1, 1.5, float("nan")):
        assert lib.rover_obs_noise_threshold(bad, C.byref(out)) == -1 and b"obs_noise_threshold" in lib.rover_last_error(None)


def test_definition_statistics():
    """One fixed seed (obs_noise_ref.SEED_STAT), 2^17 draws.  The caps are gauss_ref's, restated for N = 2^17: the KS threshold is
    test_policy_act_host's 1e-9 critical value sqrt(ln(2 / 1e-9) / (2 N)), |corr| its 6 / sqrt(N) for independent streams."""
    seed, n = R.SEED_STAT, N_STAT
    cap_ks, cap_corr = math.sqrt(math.log(2.0 / 1e-9) / (2.0 * n)), 6.0 / math.sqrt(n)
    rows = np.arange(n // 2)
    eps, rad, u = R.point_draws(seed, 3, rows, 2)                                # 2^16 rows x 2 columns = 2^17 draws
    flat = eps.reshape(-1)
    assert flat.shape == (n,) and np.isfinite(flat).all() and float(np.abs(flat).max()) <= G.EPS_MAX
    ks = G.ks_distance(flat)
    print(f"eps: KS {ks:.5f} (cap {cap_ks:.5f}) mean {flat.mean():+.5f} var-1 {flat.var() - 1:+.5f}")
    assert ks <= cap_ks
    # dropout at p = 0.1: the fraction of 24-bit words below thr
    p = 0.1
    frac = float((u.reshape(-1) < R.threshold(p)).mean())
    print(f"dropped fraction {frac:.5f} at p = {p}")
    assert abs(frac - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n)
    # against the action stream under the same seed, call counter and rows
    act, _ = G.noise(seed, 3, rows, 2)
    for j in range(2):
        cr = G.corr(eps[:, j], act[:, j])
        print(f"corr(obs, action) component {j}: {cr:+.5f} (cap {6.0 / math.sqrt(n // 2):.5f})")
        assert abs(cr) <= 6.0 / math.sqrt(n // 2)                                # n / 2 pairs per component
    assert abs(G.corr(flat, act.reshape(-1))) <= cap_corr
    assert not np.array_equal(eps, act)
    # the offset draw: one value per (row, episode) — no column, no call counter enters it — and it changes with e
    eo0, _ = R.offset_draws(seed, 0, rows[:4096])
    eo1, _ = R.offset_draws(seed, 1, rows[:4096])
    x = np.zeros((4096, 9), dtype=np.float32)
    for t in (0, 1, 2 ** 32 + 1):
        want, _, _ = R.reference(x, 1, sigma_offset=1.0, seed=seed, t=t)
        assert np.array_equal(want[:, 1:], np.repeat(eo0[:, None], 8, axis=1))  # constant over columns and steps
    assert not np.any(eo0 == eo1) and abs(G.corr(eo0, eo1)) <= 6.0 / math.sqrt(4096)
    mixed = np.where(np.arange(4096) % 3 == 0, 1, 0)
    eom, _ = R.offset_draws(seed, mixed, rows[:4096])
    assert np.array_equal(eom, np.where(mixed == 1, eo1, eo0))
    assert G.ks_distance(eo0) <= math.sqrt(math.log(2.0 / 1e-9) / (2.0 * 4096))


def test_f32_evaluation_is_inside_the_bound():
    """The formula in numpy float32 stays inside the derived bound (and the bound is tight enough to mean something: below 1e-5 of
    the values' scale); the dropout mask and the untouched columns are exact; all-off returns the input with -0.0 -> +0.0."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((333, 41)) * 3.0).astype(np.float32)
    s = rng.uniform(0.0, 2.0, 333).astype(np.float32)
    ep = rng.integers(0, 5, 333)
    worst = 0.0
    for kw in (dict(sigma_point=0.05), dict(sigma_offset=0.02), dict(sigma_point=0.05, sigma_offset=0.02, dropout=0.1, drop_value=-1.0),
               dict(sigma_point=0.2, sigma_offset=0.2, row_scale=s, episode=ep, row_offset=2 ** 32 - 333), dict(dropout=1.0, drop_value=7.0)):
        kw.update(seed=11, t=2 ** 33 + 3)
        want, bound, dropped = R.reference(x, 4, **kw)
        got = R.evaluate_f32(x, 4, **kw)
        assert np.array_equal(got[:, :4], x[:, :4]) and np.array_equal(got[dropped], want[dropped].astype(np.float32))
        live = ~dropped
        live[:, :4] = False
        if live.any():
            ratio = np.abs(got.astype(np.float64) - want)[live] / bound[live]
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 1.0 and float((bound[live] / (np.abs(want[live]) + 1.0)).max()) < 1e-5
    print(f"f32 numpy evaluation: worst error / bound {worst:.3f}")
    z = np.array([[-0.0, 1.0, -0.0, 0.0, np.inf, -2.5]], dtype=np.float32)
    off = R.evaluate_f32(z, 1)
    assert np.array_equal(off, z) and np.signbit(off[0, 0]) and not np.signbit(off[0, 2])      # copied column keeps its sign; -0.0 -> +0.0


def _rc(d):
    from isaac_rover_amd import _lib
    lib = _lib.load()
    rc = lib.rover_obs_noise(None, None if d is None else C.byref(d), None)
    return rc, lib.rover_last_error(None).decode()


def test_refusals_without_a_device():
    """Every refusal of the header's list is ROVER_E_INVALID with a message naming it; a valid descriptor gets as far as the NULL ctx."""
    from isaac_rover_amd import _lib
    D = _lib.obs_noise_desc
    inf, nan, A = float("inf"), float("nan"), 4096                   # A: a fake base address; in = out = 16 by default (in place)
    bad = {
        "null descriptor": (None, "null descriptor"),
        "null in": (D(8, 10, 4, in_=None), "in and out"), "null out": (D(8, 10, 4, out=None), "in and out"),
        "in stride": (D(8, 10, 4, in_stride=9), "row stride"), "out stride": (D(8, 10, 4, out_stride=9), "row stride"),
        "M < 0": (D(-1, 10, 4), "negative"), "F < 0": (D(8, -1, 0), "negative"),
        "first < 0": (D(8, 10, -1), "first"), "first > F": (D(8, 10, 11), "first"),
        "C > 2^21": (D(1, 2 ** 21 + 5, 4), "2^21"),
        "sigma_point < 0": (D(8, 10, 4, sigma_point=-0.1), "sigma"), "sigma_point inf": (D(8, 10, 4, sigma_point=inf), "sigma"),
        "sigma_point nan": (D(8, 10, 4, sigma_point=nan), "sigma"), "sigma_offset < 0": (D(8, 10, 4, sigma_offset=-1.0), "sigma"),
        "sigma_offset nan": (D(8, 10, 4, sigma_offset=nan), "sigma"), "sigma_offset inf": (D(8, 10, 4, sigma_offset=inf), "sigma"),
        "dropout < 0": (D(8, 10, 4, dropout=-1e-9), "dropout"), "dropout > 1": (D(8, 10, 4, dropout=1.0 + 1e-9), "dropout"),
        "dropout nan": (D(8, 10, 4, dropout=nan), "dropout"),
        "drop_value inf": (D(8, 10, 4, drop_value=inf), "drop_value"), "drop_value nan": (D(8, 10, 4, drop_value=nan), "drop_value"),
        "row_offset < 0": (D(8, 10, 4, row_offset=-1), "row_offset"), "rows past 2^32": (D(8, 10, 4, row_offset=2 ** 32 - 7), "row_offset"),
        "out shifted by one float": (D(8, 10, 4, in_=A, out=A + 4, in_stride=12, out_stride=12), "overlaps in"),
        "same pointer, other stride": (D(8, 10, 4, in_=A, out=A, in_stride=10, out_stride=12), "overlaps in"),
        "out starts in in's last row": (D(8, 10, 4, in_=A, out=A + 4 * 79), "overlaps in"),
        "row_scale in out": (D(8, 10, 4, in_=A, out=8 * A, row_scale=8 * A + 40), "overlaps out"),
        "episode in out": (D(8, 10, 4, in_=A, out=8 * A, episode=8 * A + 4 * 79), "overlaps out"),
        "step_dev in out": (D(8, 10, 4, in_=A, out=8 * A, step_dev=8 * A), "overlaps out"),
        "episode ends in out": (D(8, 10, 4, in_=A, out=8 * A, episode=8 * A - 8), "overlaps out"),
    }
    for what, (d, word) in bad.items():
        rc, msg = _rc(d)
        assert rc == -1 and msg.startswith("obs_noise:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    ok = [D(8, 10, 4), D(8, 10, 4, in_=A, out=A, in_stride=12, out_stride=12), D(8, 10, 4, in_=A, out=A + 4 * 80), D(8, 10, 0), D(8, 10, 10),
          D(1, 2 ** 21 + 4, 4), D(8, 10, 4, dropout=0.0), D(8, 10, 4, dropout=1.0), D(8, 10, 4, row_offset=2 ** 32 - 8),
          D(8, 10, 4, in_=A, out=8 * A, row_scale=8 * A - 32, episode=8 * A + 320, step_dev=8 * A - 40),
          D(8, 10, 4, sigma_point=0.0, sigma_offset=3.0, drop_value=-5.0, seed=2 ** 64 - 1, step=2 ** 64 - 1),
          D(0, 10, 4, in_=None, out=None, in_stride=0, out_stride=0), D(8, 0, 0, in_=None, out=None)]
    for i, d in enumerate(ok):
        rc, msg = _rc(d)
        assert rc == -1 and msg == "obs_noise: null ctx", (i, rc, msg)          # past every check of the descriptor


def test_heightmap_noise_constructor_and_state_dict_on_cpu():
    from isaac_rover_amd.learning.noise import HeightmapNoise
    nan, inf = float("nan"), float("inf")
    for kw in (dict(sigma_point=-1.0), dict(sigma_point=nan), dict(sigma_offset=-0.5), dict(sigma_offset=inf), dict(dropout=-0.1), dict(dropout=1.1),
               dict(dropout=nan), dict(drop_value=inf), dict(drop_value=nan), dict(env_offset=-1), dict(row_scale=[0.0, 1.0]),
               dict(row_scale=torch.zeros(4, dtype=torch.float64)), dict(row_scale=torch.zeros(2, 2))):
        with pytest.raises(ValueError):
            HeightmapNoise(None, INFO, **kw)
    with pytest.raises(KeyError):
        HeightmapNoise(None, {"sparse": 20, "dense": 30})
    sweep = HeightmapNoise.noise_sweep(0.2, 5)
    assert sweep.dtype == torch.float32 and sweep.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    with pytest.raises(ValueError):
        HeightmapNoise.noise_sweep(-0.2, 5)
    a = HeightmapNoise(None, INFO, sigma_point=0.05, sigma_offset=0.02, dropout=0.1, drop_value=-1.0, seed=2 ** 64 - 3, row_scale=sweep, env_offset=40)
    assert a.columns == 50 and a.device.type == "cpu"
    with pytest.raises(RuntimeError):
        a.apply(torch.zeros(5, 54))
    a.counter += 7
    a.episode = torch.tensor([0, 3, 1, 0, 2])
    sd = a.state_dict()
    a.counter += 1                                                               # the state_dict is a copy
    assert int(sd["counter"]) == 7
    b = HeightmapNoise(None, INFO)
    addr = b.counter.data_ptr()
    b.load_state_dict(sd)
    assert b.counter.data_ptr() == addr and int(b.counter) == 7 and b.episode.tolist() == [0, 3, 1, 0, 2]
    assert torch.equal(b.row_scale, sweep)
    assert (b.sigma_point, b.sigma_offset, b.dropout, b.drop_value, b.seed, b.env_offset) == (0.05, 0.02, 0.1, -1.0, 2 ** 64 - 3, 40)
    ep_addr = b.episode.data_ptr()
    b.load_state_dict(a.state_dict())                                            # same shapes: the counters keep their addresses
    assert b.episode.data_ptr() == ep_addr and int(b.counter) == 8
    sd.pop("episode")
    with pytest.raises(KeyError):
        b.load_state_dict(sd)
