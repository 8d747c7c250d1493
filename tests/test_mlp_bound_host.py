"""CPU: the float64 error bound of tests/mlp_ref.py holds for float32 emulations of every summation order the policy-net kernels use
(a sequential fmaf chain, up to 16 chunk partials added in a fixed order, any permutation), and the data it is used with makes a
tail bug (the last input column dropped, a neighbouring row, a neighbouring bias) break it."""
import numpy as np
import pytest
import torch

import mlp_ref as R

F32 = np.float32


def _act32(v, act):
    if act in (None, "none"):
        return v
    if act == "leakyrelu":
        return np.where(v > 0, v, F32(0.01) * v).astype(F32)
    if act == "tanh":
        return np.tanh(v).astype(F32)
    if act == "relu":
        return np.where(v > 0, v, F32(0.0)).astype(F32)
    return np.where(v > 0, v, np.expm1(np.minimum(v, F32(0)))).astype(F32)


def _dot_f32(x, w, order, fused):
    """[M, N] float32 sums of x[:, k] w[:, k] over k in ``order``, one at a time: fmaf (the product exact, one rounding per step) or
    a rounded product then a rounded add."""
    acc = np.zeros((x.shape[0], w.shape[0]), F32)
    for k in order:
        if fused:
            acc = (np.outer(x[:, k].astype(np.float64), w[:, k].astype(np.float64)) + acc).astype(F32)
        else:
            acc = (acc + np.outer(x[:, k], w[:, k]).astype(F32)).astype(F32)
    return acc


def _layer_f32(x, w, b, act, mode, rng):
    k = w.shape[1]
    if mode == "sequential":
        z = _dot_f32(x, w, range(k), fused=True)
    elif mode == "unfused":
        z = _dot_f32(x, w, range(k), fused=False)
    elif mode == "permuted":
        z = _dot_f32(x, w, rng.permutation(k), fused=True)
    else:                               # chunked: S <= 16 chunk partials (split-k's partition), added in order after a zero
        s, c = R.splitk_chunks(1, k)
        parts = [_dot_f32(x, w, range(i * c, min(k, (i + 1) * c)), fused=True) for i in range(s)]
        z = np.zeros_like(parts[0])
        for p in parts + [np.zeros_like(z)] * (16 - s):
            z = (z + p).astype(F32)
    return _act32((z + b).astype(F32), act)


def _emulate(x, layers, mode, rng):
    h = x.numpy()
    for w, b, act in layers:
        h = _layer_f32(h, w.numpy(), b.numpy(), act, mode, rng)
    return torch.from_numpy(h)


def _cancelling(m, k, n, seed):
    """x, W whose products cancel in pairs (x[:, j + k/2] = x[:, j], W[:, j + k/2] = -W[:, j]) at magnitudes up to 1e3, the bias
    small: the exact sums are a thousandth of the sums of |products|."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(m, k, generator=g) * 2 - 1) * 1e3
    w = torch.rand(n, k, generator=g) * 2 - 1
    h = k // 2
    x[:, h:2 * h] = x[:, :h]
    w[:, h:2 * h] = -w[:, :h]
    return x, [(w, (torch.rand(n, generator=g) * 2 - 1) * 1e-3, "none")]


KS = (1, 3, 16, 17, 127, 634, 1112, 4099)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mode", ["sequential", "unfused", "chunked", "permuted"])
def test_bound_holds_for_every_summation_order(k, mode):
    rng = np.random.default_rng(k)
    m = 6 if k > 1000 else 12
    for i, act in enumerate(R.ACTS):
        x, layers = R.make_data(m, k, (5, 3), (act, R.ACTS[(i + 2) % 5]), seed=k + i, device="cpu")
        want, bound = R.reference(x, layers)
        R.check(_emulate(x, layers, mode, rng), want, bound, f"{mode} K={k} {act}")
    x, layers = _cancelling(m, k, 4, seed=k)
    want, bound = R.reference(x, layers)
    got = _emulate(x, layers, mode, rng)
    R.check(got, want, bound, f"{mode} K={k} cancelling")
    if k >= 127:                           # the data really cancels, and the rounding error is real: the bound is not vacuous
        assert float((got.double() - want).abs().max()) > 0.0


def test_bound_rejects_a_one_percent_error():
    """The bound is a few gamma_K: at K = 634 a result off by 1 % of its value is outside it on most elements."""
    x, layers = R.make_data(16, 634, (8,), ("none",), seed=3, device="cpu")
    want, bound = R.reference(x, layers)
    assert float((bound / want.abs().clamp_min(1e-3)).median()) < 1e-3
    with pytest.raises(AssertionError):
        R.check((want * 1.01).float(), want, bound)


@pytest.mark.parametrize("m,k0,widths,acts", [
    (1, 1, (1,), ("none",)), (33, 33, (31,), ("tanh",)), (17, 1105, (80, 17), ("relu", "elu")), (64, 124, (17, 33, 15, 2), ("leakyrelu", "relu", "none", "tanh")),
    (1, 124, (1, 1, 1, 1), ("relu", "relu", "relu", "tanh")), (20, 634, (96, 1), ("elu", "none"))])
def test_guard_rejects_tail_row_and_bias_bugs(m, k0, widths, acts):
    """sensitive_data() finds data on which every mutation is rejected, and a float32 emulation of each mutated net then fails
    check() against the unmutated reference."""
    x, layers, want, bound = R.sensitive_data(m, k0, widths, acts, seed=5, device="cpu")
    muts = R.mutations(x, layers)
    assert "drop_last_column" in muts and ("row_neighbour" in muts) == (m > 1) and ("bias0_neighbour" in muts) == (widths[0] > 1)
    rng = np.random.default_rng(0)
    R.check(_emulate(x, layers, "sequential", rng), want, bound, "unmutated")
    for name, (xm, lm) in muts.items():
        with pytest.raises(AssertionError):
            R.check(_emulate(xm, lm, "sequential", rng), want, bound, name)


def test_traps():
    x = torch.arange(12.0).view(3, 4)
    t = R.trapped_input(x, 3)
    assert t.stride(0) % 2 == 1 and torch.equal(t, x)
    base = t.storage_offset()
    full = torch.as_strided(t, (4, t.stride(0)), (t.stride(0), 1), base - 3)
    assert bool(full[3].isnan().all()) and bool(full[:3, :3].isnan().all())
    w = R.nan_head(torch.ones(2, 3))
    assert bool(torch.as_strided(w, (1,), (1,), 6).isnan().all())
    c = R.Canary(3, 2, "cpu")
    assert c.buf.stride(0) % 2 == 1 and c.intact()
    c.y.fill_(1.0)
    assert c.intact()
    c.buf[3, 0] = 0.0
    assert not c.intact()


@pytest.mark.parametrize("m,k,s,last", [(1, 1105, 14, 65), (1, 4099, 16, 19), (16, 634, 10, 58), (2048, 1112, 14, 72)])
def test_splitk_partition(m, k, s, last):
    """The split-k partitions the GPU cases are chosen for: a last chunk that is not a multiple of 4 or 16, and the 16-chunk cap."""
    S, c = R.splitk_chunks(m, k)
    assert (S, k - (S - 1) * c) == (s, last)
