"""CPU: the running standard scaler as DEFINED (tests/scaler_ref.py) against torch.mean / torch.var in float64 and a pinned 4 x 2 case,
rover_scaler_plan on both sides of every threshold it has, every refusal of rover_scaler_update / rover_scaler_apply (the C layer
validates the descriptor before it looks at the ctx, so a NULL ctx will do), KLAdaptiveRL's rule at its ties and caps, PPO's new
constructor refusals and RunningStandardScaler's state_dict.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import scaler_ref as R


def test_symbols_declared_and_exported():
    from isaac_rover_amd import _lib
    lib = _lib.load()
    for name in ("rover_scaler_plan", "rover_scaler_update", "rover_scaler_apply"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert [f for f, _ in _lib.ScalerPlanDesc._fields_] == ["route", "rows_per_chunk", "n_chunks", "scratch_bytes"]
    assert [f for f, _ in _lib.ScalerUpdateDesc._fields_] == ["x", "x_stride", "M", "N", "mean", "var", "count", "scratch", "scratch_bytes", "skip_if"]
    assert [f for f, _ in _lib.ScalerApplyDesc._fields_] == ["x", "x_stride", "y", "y_stride", "M", "N", "mean", "var", "epsilon", "clip", "inverse"]
    assert C.sizeof(_lib.ScalerPlanDesc) == 24 and C.sizeof(_lib.ScalerUpdateDesc) == 72 and C.sizeof(_lib.ScalerApplyDesc) == 80


def test_plan_on_both_sides_of_every_threshold():
    from isaac_rover_amd import _lib
    plan = _lib.scaler_plan
    W, NARROW = _lib.SCALER_WIDE, _lib.SCALER_NARROW
    # the route switch in N
    assert [plan(100, n)["route"] for n in (1, 7, 8, 9, 1750, 4096)] == [NARROW, NARROW, NARROW, W, W, W]
    # the chunk size in M: narrow 16 384 rows whatever M; wide 32 rows up to M = 8 192, 128 beyond
    assert [plan(m, 8)["rows_per_chunk"] for m in (2, 16384, 16385, 10 ** 6)] == [16384] * 4
    assert [plan(m, 9)["rows_per_chunk"] for m in (2, 8191, 8192, 8193, 10 ** 6)] == [32, 32, 32, 128, 128]
    # the chunk count: ceil(M / rows_per_chunk), on both sides of one chunk and of the chunk-size switch
    assert [plan(m, 1)["n_chunks"] for m in (0, 1, 16383, 16384, 16385, 3 * 16384 + 5)] == [0, 1, 1, 1, 2, 4]
    assert [plan(m, 1750)["n_chunks"] for m in (31, 32, 33, 130, 8192, 8193)] == [1, 1, 2, 5, 256, 65]
    for m, n in ((0, 1), (2, 1), (4097, 1), (130, 1750), (8193, 9), (65536, 1750)):
        p = plan(m, n)
        assert p["scratch_bytes"] == 8 + 24 * p["n_chunks"] * n, (m, n, p)
    # the M N limit and the range of N
    assert plan((2 ** 31 - 1) // 1750, 1750)["route"] == W and plan(2 ** 31 - 1, 1)["n_chunks"] == 2 ** 17
    lib = _lib.load()
    out = _lib.ScalerPlanDesc()
    for m, n, word in (((2 ** 31 - 1) // 1750 + 1, 1750, "2^31"), (2 ** 30, 2, "2^31"), (-1, 4, "negative"), (4, 0, "N = 0"), (4, 4097, "N = 4097")):
        assert lib.rover_scaler_plan(m, n, C.byref(out)) == -1 and word in lib.rover_last_error(None).decode(), (m, n)
    assert lib.rover_scaler_plan(4, 4, None) == -1 and "null" in lib.rover_last_error(None).decode()


def _call(fn, d):
    from isaac_rover_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, fn)(None, None if d is None else C.byref(d), None)
    return rc, lib.rover_last_error(None).decode()


def test_update_refusals_through_a_null_ctx():
    from isaac_rover_amd import _lib
    D = _lib.scaler_update_desc
    x = 1 << 36
    cases = [
        ("no descriptor", None, "null descriptor"),
        ("x", D(64, 4, x=None), "null pointer"), ("mean", D(64, 4, mean=None), "null pointer"), ("var", D(64, 4, var=None), "null pointer"),
        ("count", D(64, 4, count=None), "null pointer"), ("scratch", D(64, 4, scratch=None), "null pointer"),
        ("N = 0", D(64, 0, scratch_bytes=8), "N = 0"), ("N = 4097", D(64, 4097, scratch_bytes=8), "N = 4097"),
        ("M < 0", D(-1, 4, scratch_bytes=8), "negative"), ("M N = 2^31", D(2 ** 29, 4, scratch_bytes=8), "2^31"),
        ("M = 0", D(0, 4), "at least 2"), ("M = 1", D(1, 4), "at least 2"),
        ("short stride", D(64, 4, x_stride=3), "row stride"), ("huge stride", D(64, 4, x_stride=2 ** 40 + 1), "row stride"),
        ("mean misaligned", D(64, 4, mean=20), "aligned"), ("var misaligned", D(64, 4, var=(1 << 15) + 4), "aligned"),
        ("count misaligned", D(64, 4, count=(1 << 16) + 2), "aligned"), ("scratch misaligned", D(64, 4, scratch=(1 << 20) + 4), "aligned"),
        ("scratch one byte short", D(64, 4, scratch_bytes=_lib.scaler_plan(64, 4)["scratch_bytes"] - 1), "plan needs"),
        ("mean inside x", D(64, 4, mean=x + 64), "mean overlaps x"), ("var at the end of x", D(64, 4, var=x + 64 * 16 - 8), "var overlaps x"),
        ("count inside scratch", D(64, 4, count=(1 << 20) + 8), "count overlaps scratch"),
        ("mean inside scratch", D(64, 4, mean=(1 << 20) + _lib.scaler_plan(64, 4)["scratch_bytes"] - 8), "mean overlaps scratch"),
        ("var on mean", D(64, 4, var=16 + 24), "var overlaps mean"), ("count on var", D(64, 4, count=16 + (1 << 15) + 24), "count overlaps var"),
        ("scratch on x", D(64, 4, scratch=x + 8), "scratch overlaps x"),
        ("skip_if on count", D(64, 4, skip_if=16 + (1 << 16) + 4), "skip_if overlaps count"), ("skip_if in scratch", D(64, 4, skip_if=(1 << 20) + 4), "skip_if overlaps scratch"),
        ("skip_if misaligned", D(64, 4, skip_if=2), "skip_if"),
    ]
    for what, d, word in cases:
        rc, msg = _call("rover_scaler_update", d)
        assert rc == -1 and msg.startswith("scaler_update:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    legal = [D(2, 1), D(64, 4), D(64, 4, x_stride=7, skip_if=4), D(130, 1750), D(64, 4, var=16 + 32, count=16 + 64),      # state packed tightly
             D(64, 4, mean=x + 64 * 16)]                                                                                  # right behind x
    for i, d in enumerate(legal):
        rc, msg = _call("rover_scaler_update", d)
        assert rc == -1 and msg == "scaler_update: null ctx", (i, rc, msg)          # past every check of the descriptor


def test_apply_refusals_through_a_null_ctx():
    from isaac_rover_amd import _lib
    D = _lib.scaler_apply_desc
    x = 1 << 36
    cases = [
        ("no descriptor", None, "null descriptor"),
        ("x", D(64, 4, x=None), "null pointer"), ("y", D(64, 4, y=None), "null pointer"), ("mean", D(64, 4, mean=None), "null pointer"),
        ("var", D(0, 4, var=None), "null pointer"),
        ("N = 0", D(64, 0), "N = 0"), ("N = 4097", D(64, 4097), "N = 4097"), ("M < 0", D(-1, 4), "negative"), ("M N = 2^31", D(2 ** 29, 4), "2^31"),
        ("short x stride", D(64, 4, x_stride=3), "row stride"), ("short y stride", D(64, 4, y=x + (1 << 20), y_stride=3), "row stride"),
        ("mean misaligned", D(64, 4, mean=20), "aligned"), ("var misaligned", D(64, 4, var=(1 << 15) + 4), "aligned"),
        ("epsilon < 0", D(64, 4, epsilon=-1e-8), "epsilon"), ("epsilon NaN", D(64, 4, epsilon=math.nan), "epsilon"),
        ("epsilon Inf", D(64, 4, epsilon=math.inf), "epsilon"), ("clip < 0", D(64, 4, clip=-5.0), "clip"), ("clip NaN", D(64, 4, clip=math.nan), "clip"),
        ("clip Inf", D(64, 4, clip=math.inf), "clip"),
        ("y one float into x", D(64, 4, y=x + 4), "without being the same array"), ("y = x, other stride", D(64, 4, x_stride=8, y_stride=4), "without being"),
        ("y's last row on x's first", D(64, 4, y=x - 63 * 16 - 4), "without being the same array"),
        ("mean inside x", D(64, 4, mean=x + 8), "mean overlaps x"), ("var inside y", D(64, 4, y=x + (1 << 20), var=x + (1 << 20) + 8), "var overlaps y"),
    ]
    for what, d, word in cases:
        rc, msg = _call("rover_scaler_apply", d)
        assert rc == -1 and msg.startswith("scaler_apply:") and word in msg and "null ctx" not in msg, (what, rc, msg)
    legal = [D(64, 4), D(0, 4, x=None, y=None), D(64, 4, x_stride=8, y_stride=8), D(64, 4, y=x + 64 * 16), D(64, 4, inverse=True, epsilon=0.0, clip=0.0)]
    for i, d in enumerate(legal):
        rc, msg = _call("rover_scaler_apply", d)
        assert rc == -1 and msg == "scaler_apply: null ctx", (i, rc, msg)


def test_restatement_against_torch_float64():
    g = torch.Generator().manual_seed(5)
    state = R.fresh(6)
    mean_t, var_t, count_t = torch.zeros(6, dtype=torch.float64), torch.ones(6, dtype=torch.float64), 1.0
    for m in (2, 7, 300):
        x = (torch.randn(m, 6, generator=g) * torch.tensor([0.1, 1, 8, 1, 1, 3]) + torch.tensor([0, 100, -3, 0, 1e-3, 5])).float()
        state = R.update(state, x.numpy())
        xd = x.double()
        mb, vb = torch.mean(xd, dim=0), torch.var(xd, dim=0)                        # unbiased, as skrl calls it
        delta, total = mb - mean_t, count_t + m
        m2 = var_t * count_t + vb * m + delta ** 2 * count_t * m / total
        mean_t, var_t, count_t = mean_t + delta * m / total, m2 / total, total
        assert state[2] == count_t
        np.testing.assert_allclose(state[0], mean_t.numpy(), rtol=1e-14, atol=0)
        np.testing.assert_allclose(state[1], var_t.numpy(), rtol=1e-13, atol=0)
    # [T, E, size] flattens into rows
    x3 = torch.randn(3, 5, 6, generator=g).numpy()
    a, b = R.update(R.fresh(6), x3), R.update(R.fresh(6), x3.reshape(15, 6))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 16.0
    with pytest.raises(ValueError):
        R.update(R.fresh(6), x3[0, :1])


def test_pinned_four_by_two_and_the_two_halves():
    """x = [[1, 10], [2, 10], [3, 10], [6, 14]] from skrl's initial state (mean 0, var 1, count 1), by hand:
    whole: mb = (3, 11), vb = (14 / 3, 4); total = 5; mean = 4 mb / 5 = (2.4, 8.8);
           m2 = 1 + 4 vb + mb^2 4 / 5 = (1 + 56 / 3 + 7.2, 1 + 16 + 96.8); var = m2 / 5 = (5.3733.., 22.76).
    halves: first [[1, 10], [2, 10]]: mb = (1.5, 10), vb = (0.5, 0), total 3: mean = (1, 20 / 3), var = (1 + 1 + 1.5, 1 + 0 + 200 / 3) / 3;
            then [[3, 10], [6, 14]]: mb = (4.5, 12), vb = (4.5, 8), total 5: mean = (1 + 3.5 * 2 / 5, 20 / 3 + (16 / 3) * 2 / 5) = (2.4, 8.8),
            var = (3.5 + 9 + 12.25 * 6 / 5, 203 / 3 + 16 + (256 / 9) * 6 / 5) / 5 = (5.44, 23.56).
    The means agree, the variances do not: the pseudo-sample (count 1, var 1, mean 0) and the unbiased batch variance make the start
    asymmetric — each train call weighs its UNBIASED variance by M, not M - 1."""
    x = np.array([[1, 10], [2, 10], [3, 10], [6, 14]], dtype=np.float32)
    mean, var, count = R.update(R.fresh(2), x)
    assert count == 5.0
    np.testing.assert_allclose(mean, [2.4, 8.8], rtol=1e-15)
    np.testing.assert_allclose(var, [(1 + 56 / 3 + 7.2) / 5, 22.76], rtol=1e-15)
    h = R.update(R.update(R.fresh(2), x[:2]), x[2:])
    assert h[2] == 5.0
    np.testing.assert_allclose(h[0], [2.4, 8.8], rtol=1e-15)
    np.testing.assert_allclose(h[1], [5.44, 23.56], rtol=1e-15)
    # from a state that already holds many samples the two ways agree up to the pseudo-sample's O(1 / count) effect on the weights
    g = np.random.default_rng(3)
    big = R.update(R.fresh(2), g.normal(size=(10 ** 5, 2)).astype(np.float32))
    y = g.normal(size=(4000, 2)).astype(np.float32)
    w, hh = R.update(big, y), R.update(R.update(big, y[:2000]), y[2000:])
    np.testing.assert_allclose(w[0], hh[0], rtol=0, atol=1e-12)
    assert np.all(np.abs(w[1] - hh[1]) <= 2.0 / 104000) and np.all(w[1] != hh[1])
    # forward and inverse under the pinned statistics: float32, one rounding per operation
    f = np.float32
    s = np.sqrt(var.astype(f)) + f(1e-8)
    want = np.clip((x - mean.astype(f)) / s, f(-5), f(5))
    assert np.array_equal(R.forward(x, mean, var), want) and want.dtype == np.float32
    assert np.array_equal(R.inverse(want, mean, var), np.sqrt(var.astype(f)) * want + mean.astype(f))
    edge = np.array([[np.nan, np.inf], [-np.inf, 1e30]], dtype=f)
    fw, iv = R.forward(edge, mean, var), R.inverse(edge, mean, var)
    assert np.isnan(fw[0, 0]) and fw[0, 1] == 5 and fw[1, 0] == -5 and fw[1, 1] == 5
    assert np.isnan(iv[0, 0]) and iv[0, 1] == f(np.sqrt(var.astype(f))[1] * f(5) + mean.astype(f)[1])


def test_bound_covers_the_two_halves_error_of_the_restatement():
    """The bound is a bound: two evaluation orders of the same batch moments (whole against pairwise halves merged by Chan) differ by less."""
    g = np.random.default_rng(11)
    x = (g.uniform(-8, 8, size=(4097, 5))).astype(np.float32)
    x[:, 1] = 7.75
    x[:, 2] = np.where(np.arange(4097) % 2 == 0, 8.0, -8.0)
    xd = x.astype(np.float64)
    mb, vb = R.batch_moments(x)
    h = 2048
    (ma, va), (mc, vc) = R.batch_moments(x[:h]), R.batch_moments(x[h:])
    na, nc = float(h), float(4097 - h)
    d = mc - ma
    merged_mean = ma + d * nc / (na + nc)
    merged_m2 = va * (na - 1) + vc * (nc - 1) + d * d * na * nc / (na + nc)
    d_mb, d_m2 = R.moment_bound(4097, np.abs(xd).sum(0), (xd * xd).sum(0), 1, mb)
    assert np.all(np.abs(merged_mean - mb) <= d_mb) and np.all(np.abs(merged_m2 - vb * 4096) <= d_m2)
    # and it is tight enough to mean something: far inside the cap the GPU tests put on it
    assert np.all(d_m2 / 4097 <= 1e-3 * R.CAP * (vb + mb ** 2))


def test_kl_adaptive_rule_at_its_ties_and_caps():
    from isaac_rover_amd.learning.ppo import KLAdaptiveRL

    class Opt:
        lr = 1e-4
    hi, lo = 0.008 * 2, 0.008 / 2
    up, down = math.nextafter, lambda v: math.nextafter(v, -math.inf)
    for kl, want in ((hi, 1e-4), (lo, 1e-4), (up(hi, math.inf), 1e-4 / 1.5), (down(hi), 1e-4), (down(lo), 1e-4 * 1.5), (up(lo, math.inf), 1e-4),
                     (0.0, 1e-4 * 1.5), (1.0, 1e-4 / 1.5), (math.nan, 1e-4)):
        o = Opt()
        assert KLAdaptiveRL(o).step(kl) == want == R.kl_adaptive(1e-4, kl) == o.lr, kl
    # both caps: a step that would pass one lands on it, and at it nothing moves
    for lr, kl, want in ((1.2e-6, 1.0, 1e-6), (1e-6, 1.0, 1e-6), (9e-3, 0.0, 1e-2), (1e-2, 0.0, 1e-2)):
        o = Opt()
        o.lr = lr
        assert KLAdaptiveRL(o).step(kl) == want == R.kl_adaptive(lr, kl), (lr, kl)
    # the scheduler's own threshold and factors; a torch optimiser's param groups
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.Adam([p], lr=1e-3)
    s = KLAdaptiveRL(topt, kl_threshold=0.01, kl_factor=4, lr_factor=2, min_lr=1e-5, max_lr=1.5e-3)
    assert s.step(0.0401) == 5e-4 and s.step(0.04) == 5e-4 and s.step(0.0024) == 1e-3 and s.step(0.0) == 1.5e-3
    assert topt.param_groups[0]["lr"] == 1.5e-3
    with pytest.raises(ValueError):
        KLAdaptiveRL(None, min_lr=1e-2, max_lr=1e-3)
    with pytest.raises(RuntimeError):
        KLAdaptiveRL().step(0.0)


class _Net:
    """What PPO's constructor reads of a HeightmapNet."""
    device = "cpu"
    reduction = "sum"
    num_proprioception, num_sparse, num_dense = 4, 37, 0

    def __init__(self, stochastic):
        self.log_std_parameter = torch.zeros(2) if stochastic else None

    def parameters(self):
        return [torch.zeros(3)]


class _Mem:
    memory_size, num_envs = 4, 64


def test_ppo_constructor_refusals():
    from isaac_rover_amd.learning.ppo import PPO, KLAdaptiveRL
    from isaac_rover_amd.learning.preprocess import RunningStandardScaler
    mk = lambda **kw: PPO(None, _Net(True), _Net(False), _Mem(), {"mini_batches": 2}, **kw)
    sp, vp = RunningStandardScaler(None, 41, device="cpu"), RunningStandardScaler(None, 1, device="cpu")
    ok = mk(state_preprocessor=sp, value_preprocessor=vp, lr_scheduler=KLAdaptiveRL())
    assert ok.state_preprocessor is sp and ok.value_preprocessor is vp and ok.lr_scheduler.optimizer is ok.optimizer
    assert mk().state_preprocessor is None and mk().lr_scheduler is None
    x = torch.zeros(3, 41)
    assert mk().preprocess_states(x) is x and mk().denormalize_values(x) is x
    for kw, word in ((dict(state_preprocessor=RunningStandardScaler(None, 40, device="cpu")), "size 40"),
                     (dict(value_preprocessor=RunningStandardScaler(None, 2, device="cpu")), "size 2"),
                     (dict(state_preprocessor="RunningStandardScaler"), "RunningStandardScaler instance"),
                     (dict(value_preprocessor=object()), "RunningStandardScaler instance"),
                     (dict(lr_scheduler="kl"), "KLAdaptiveRL instance"),
                     (dict(lr_scheduler=KLAdaptiveRL(), native_step=True, kl_stop="device"), "kl_stop='device'")):
        with pytest.raises(ValueError, match=word):
            mk(**kw)
    with pytest.raises(ValueError, match="unknown cfg keys"):                     # the cfg's key check is as it was
        PPO(None, _Net(True), _Net(False), _Mem(), {"state_preprocessor": None})


def test_scaler_constructor_and_state_dict_round_trip():
    from isaac_rover_amd.learning.preprocess import RunningStandardScaler
    for kw in (dict(size=0), dict(size=4097), dict(size=4, epsilon=-1.0), dict(size=4, clip_threshold=math.inf), dict(size=4, epsilon=math.nan)):
        with pytest.raises(ValueError):
            RunningStandardScaler(None, device="cpu", **kw)
    with pytest.raises(ValueError):
        RunningStandardScaler(None, 4)                                            # neither an engine nor a device
    a = RunningStandardScaler(None, 3, device="cpu")
    sd = a.state_dict()
    assert set(sd) == {"running_mean", "running_variance", "current_count"} and all(v.dtype == torch.float64 for v in sd.values())
    assert torch.equal(sd["running_mean"], torch.zeros(3, dtype=torch.float64)) and torch.equal(sd["running_variance"], torch.ones(3, dtype=torch.float64))
    assert sd["current_count"].shape == () and float(sd["current_count"]) == 1.0                # skrl's: a 0-dim tensor
    # a skrl checkpoint's entry: float64 tensors under the same three keys
    skrl = {"running_mean": torch.tensor([0.5, -2.0, 1e3], dtype=torch.float64), "running_variance": torch.tensor([4.0, 0.25, 1e-6], dtype=torch.float64),
            "current_count": torch.tensor(12345.0, dtype=torch.float64)}
    ptr = a.running_mean.data_ptr()
    a.load_state_dict(skrl)
    assert a.running_mean.data_ptr() == ptr                                       # in place
    back = a.state_dict()
    assert all(torch.equal(back[k], skrl[k]) for k in skrl)
    back["running_mean"][0] = 7.0                                                 # a copy, not the live state
    assert float(a.running_mean[0]) == 0.5
    b = RunningStandardScaler(None, 3, device="cpu")
    b.load_state_dict(a.state_dict())
    assert all(torch.equal(b.state_dict()[k], skrl[k]) for k in skrl)
    for bad in ({"running_mean": skrl["running_mean"]}, {**skrl, "running_mean": torch.zeros(4, dtype=torch.float64)},
                {**skrl, "current_count": torch.zeros(2, dtype=torch.float64)}):
        with pytest.raises(ValueError):
            b.load_state_dict(bad)
    with pytest.raises(RuntimeError):
        a(torch.zeros(2, 3))                                                      # built without an engine
