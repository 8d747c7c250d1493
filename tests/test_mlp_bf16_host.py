"""CPU: the pieces the bf16 chain kernels are tested with (tests/bf16_ref.py) and the host-only entry points of the bf16 path —
rover_bf16_round (the rounding the kernels apply, one definition shared with them) and the bf16 route queries."""
import numpy as np
import pytest
import torch

import bf16_ref as B
import mlp_ref as R

SHAPES2 = [(634, (80, 60)), (1112, (80, 60)), (33, (96, 64)), (1, (17, 3))]
SHAPES4 = [(124, (256, 160, 128, 2)), (124, (256, 160, 128, 1)), (31, (100, 50, 20, 1))]
M = 37                                           # rows 2, 7, ... all zero, rows 4, 11, ... at +-64


def _lib():
    from isaac_rover_amd import _lib
    return _lib


def _lattice_acts(widths, last="none"):
    return tuple(("relu", "none")[i % 2] for i in range(len(widths) - 1)) + (last,)


# ---- rover_bf16_round ---------------------------------------------------------------------------------------------------------
def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), want.numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan]))


def test_bf16_round_special_values():
    L = _lib()
    f = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)
    ties = f([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7F8000])      # exactly half way: to even, down and up; the last to Inf
    near = f([0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF807FFF, 0xBF808001])
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float32).max, -np.finfo(np.float32).max], dtype=np.float32)
    x = np.concatenate([ties, near, special])
    got = L.bf16_round(x)
    _same(got, B.rd(torch.from_numpy(x.astype(np.float64))))
    assert list(got[:5].view(np.uint32)) == [0x3F800000, 0x3F820000, 0xBF800000, 0xBF820000, 0x7F800000]
    assert list(got[5:11].view(np.uint32)) == [0x3F800000, 0x3F810000, 0x3F810000, 0x3F820000, 0xBF800000, 0xBF810000]
    assert np.isinf(got[-1]) and np.isinf(got[-2]) and got[-2] > 0 > got[-1]
    assert bool((got.view(np.uint32)[~np.isnan(got)] & 0xFFFF == 0).all())


def test_bf16_round_random_values():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)        # every exponent, subnormals included
    x = x[np.isfinite(x)]
    _same(_lib().bf16_round(x), B.rd(torch.from_numpy(x.astype(np.float64))))
    y = (rng.standard_normal(100000) * 3).astype(np.float32)
    _same(_lib().bf16_round(y), B.rd(torch.from_numpy(y.astype(np.float64))))
    assert _lib().bf16_round(np.zeros((0,), dtype=np.float32)).shape == (0,)


# ---- the route queries --------------------------------------------------------------------------------------------------------
def test_bf16_routes():
    E = _lib().Engine
    enc, mlp = ("leakyrelu", "leakyrelu"), ("leakyrelu", "leakyrelu", "leakyrelu", "tanh")
    for m in (1, 128, 65536):
        assert E.chain_route(m, 634, (80, 60), enc, precision="bf16") == "chain_bf16<5,4,0,0>"
        assert E.chain_route(m, 1112, (80, 60), enc, precision="bf16") == "chain_bf16<5,4,0,0>"
        assert E.chain_route(m, 634, (96, 64), ("elu", "tanh"), precision="bf16") == "chain_bf16<6,4,0,0>"
        assert E.chain_route(m, 124, (256, 160, 128, 2), mlp, precision="bf16") == "chain_bf16<16,10,8,1>"
        assert E.chain_route(m, 0, (80, 60), enc, precision="bf16") == "chain_bf16<5,4,0,0>"          # an empty obs slice: bf16 only
        assert E.chain_route(m, 0, (80, 60), enc) is None
        assert E.chain_act_route(m, 124, (256, 160, 128, 2), mlp, precision="bf16") == "chain_bf16<16,10,8,1>+gauss"
        assert E.chain_act_route(m, 124, (256, 160, 128, 16), mlp, precision="bf16") == "chain_bf16<16,10,8,1>;gauss"
        assert E.chain_act_route(m, 634, (80, 4), enc, precision="bf16") == "chain_bf16<5,4,0,0>;gauss"
        # refused exactly where the f32 chains are refused (one fit rule)
        for k0, widths, acts in ((634, (97, 60), enc), (634, (80, 65), enc), (124, (257, 160, 128, 2), mlp), (124, (256, 161, 128, 2), mlp),
                                 (124, (256, 160, 129, 2), mlp), (124, (256, 160, 128, 17), mlp),
                                 (124, (256, 160, 128, 2), ("leakyrelu", "tanh", "leakyrelu", "tanh")), (124, (80, 60, 2), mlp[1:])):
            assert E.chain_route(m, k0, widths, acts, precision="bf16") is None, (k0, widths, acts)
            assert E.chain_route(m, k0, widths, acts) is None
        assert E.chain_act_route(m, 124, (257, 160, 128, 2), mlp, precision="bf16") is None
    assert E.chain_route(0, 634, (80, 60), enc, precision="bf16") == "none"
    assert E.chain_act_route(0, 124, (256, 160, 128, 2), mlp, precision="bf16") == "none"
    assert E.chain_route(128, 634, (80, 60), enc) == "splitk<5,1>"                      # the f32 queries answer as before
    with pytest.raises(ValueError):
        E.chain_route(128, 634, (80, 60), enc, precision="fp16")


# ---- the lattice builder's self-checks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0,widths", SHAPES2 + SHAPES4, ids=str)
def test_lattice_is_exact_in_any_order_and_sees_truncation_and_mutations(k0, widths):
    x, layers, want = B.lattice(M, k0, widths, _lattice_acts(widths), seed=k0 + len(widths))
    fwd = B.emulate(x, layers)
    assert torch.equal(fwd, want)
    assert torch.equal(B.emulate(x, layers, chunk=7, reverse=True), want)               # a reversed, chunked f32 summation order: the same bits
    differ = int((B.emulate(x, layers, truncate=True) != want).sum())
    print(f"{k0} -> {widths}: a truncating rounding differs on {differ} of {want.numel()} outputs")
    assert differ > 0 or k0 == 1                                                        # (K0 = 1: too few distinct hidden values)
    for name, (xm, lm) in R.mutations(x, layers).items():
        assert not torch.equal(B.emulate(xm, lm), want), name


def test_lattice_tanh_and_leakyrelu_heads():
    for last in ("tanh", "leakyrelu"):
        x, layers, want = B.lattice(M, 124, (256, 160, 128, 2), _lattice_acts((256, 160, 128, 2), last), seed=3)
        got = B.emulate(x, layers, chunk=5, reverse=True)
        B.check_exact(got, want, last, last)
        if last == "tanh":
            assert float(want.abs().max()) <= 1.0 and float(want.abs().min()) < 0.99    # not everything saturated


# ---- the interval bound for arbitrary data -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0,widths", SHAPES2 + SHAPES4, ids=str)
def test_emulation_lies_inside_the_interval_bound(k0, widths):
    acts = ("leakyrelu",) * (len(widths) - 1) + ("tanh" if len(widths) == 4 else "leakyrelu",)
    x, layers = R.make_data(M, k0, widths, acts, seed=k0, device="cpu")
    want, bound = B.reference(x, layers)
    for kw in (dict(), dict(chunk=7, reverse=True)):
        ratio = B.check(B.emulate(x, layers, **kw), want, bound, str(kw))
        print(f"{k0} -> {widths} {kw}: worst error / bound = {ratio:.3g}")
    rej = B.rejected(x, layers, want, bound)
    print(f"{k0} -> {widths}: mutation distance / (2 bound): " + ", ".join(f"{k} {v:.3g}" for k, v in rej.items()))
    if len(widths) == 2 and k0 > 1:
        assert all(v > 1.0 for v in rej.values()), rej                                  # the 4-layer shapes: printed, not asserted


def test_rd_is_round_to_nearest_even_without_double_rounding():
    # 1 + 2^-8 + 2^-40 is above the tie: through float32 (which drops the 2^-40) it would round down to 1
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** -133 * 1.5, 2.0 ** -133 * 0.5], dtype=torch.float64)
    assert B.rd(v).tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, 2.0 ** -132, 0.0]
    assert B.rd(v, truncate=True).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7, 2.0 ** -133, 0.0]
