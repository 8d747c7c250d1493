"""Host-side checks of the rollout feature (no GPU): the float64 reference of rover_gae against a literal transcription and a hand-worked
case, the derived bound against float32 evaluations in two operation orders, RolloutMemory on the CPU, and the moments' combine."""
import numpy as np
import pytest
import torch

import gae_ref as G


def torch_loop(rewards, values, dones, last_values, gamma=0.99, lam=0.95, normalize=True):
    """The literal transcription of the definition (include/rover_step.h) in torch, in the dtype and on the device of its inputs: the loop
    a user of this package writes without rover_gae (seven elementwise launches per time step, about 430 at T = 60).  -> (returns, advantages)."""
    T = rewards.shape[0]
    adv = torch.zeros_like(last_values)
    A = torch.zeros_like(rewards)
    not_dones = dones.logical_not()
    for t in reversed(range(T)):
        nv = values[t + 1] if t < T - 1 else last_values
        adv = rewards[t] - values[t] + gamma * not_dones[t] * (nv + lam * adv)
        A[t] = adv
    returns = A + values
    if normalize:
        A = (A - A.mean()) / (A.std() + 1e-8)
    return returns, A


@pytest.mark.parametrize("T,E,pattern", [(1, 2, "none"), (7, 5, "random"), (60, 33, "random"), (13, 4, "all"), (9, 3, "last"), (9, 3, "first")])
def test_reference_equals_literal_transcription(T, E, pattern):
    r, v, d, lv = G.make_case(T, E, pattern, seed=T * 100 + E, rate=0.2)
    ref = G.reference(r, v, d, lv, 0.99, 0.95)
    t64 = lambda a: torch.from_numpy(a).double()
    ret, adv = torch_loop(t64(r), t64(v), torch.from_numpy(d), t64(lv), G.f32_param(0.99), G.f32_param(0.95), normalize=True)
    ret_raw, raw = torch_loop(t64(r), t64(v), torch.from_numpy(d), t64(lv), G.f32_param(0.99), G.f32_param(0.95), normalize=False)
    np.testing.assert_allclose(ref["A"], raw.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref["returns"], ret.numpy(), rtol=1e-13, atol=1e-13)
    out, _ = G.normalized(ref["A"], ref["bA"])
    np.testing.assert_allclose(out, adv.numpy(), rtol=1e-11, atol=1e-11)


def test_reference_hand_worked_case():
    """T = 3, E = 2, gamma = 0.5, lam = 0.5 (exact in float32), env 1 done at t = 1.
    env 0: A2 = 1 - 0.5 + 0.5 (2)              = 1.5      A1 = 2 - 1 + 0.5 (0.5 + 0.5 * 1.5)  = 1.625
           A0 = 0 - 2 + 0.5 (1 + 0.5 * 1.625)  = -1.09375
    env 1: A2 = 4 - 1 + 0.5 (-2)               = 2        A1 = 1 - 3 + 0 = -2 (done)          A0 = 2 - 0 + 0.5 (3 + 0.5 * -2) = 3
    returns = A + values."""
    r = np.array([[0, 2], [2, 1], [1, 4]], dtype=np.float32)
    v = np.array([[2, 0], [1, 3], [0.5, 1]], dtype=np.float32)
    d = np.array([[0, 0], [0, 1], [0, 0]], dtype=bool)
    lv = np.array([2, -2], dtype=np.float32)
    ref = G.reference(r, v, d, lv, 0.5, 0.5)
    want = np.array([[-1.09375, 3.0], [1.625, -2.0], [1.5, 2.0]])
    np.testing.assert_array_equal(ref["A"], want)
    np.testing.assert_array_equal(ref["returns"], want + v)
    a = want.reshape(-1)
    m = a.sum() / 6
    std = np.sqrt(((a - m) ** 2).sum() / 5)
    np.testing.assert_allclose(G.normalized(ref["A"], ref["bA"])[0], (want - m) / (std + 1e-8), rtol=1e-15)


def _f32_eval(r, v, d, lv, gamma, lam, order):
    """The recursion in float32 numpy, every operation rounded once.  order 0: r - v + g (nv + lam adv); order 1: (r + (g nv + (g lam) adv)) - v."""
    f = np.float32
    T, E = r.shape
    A = np.empty((T, E), dtype=f)
    adv = np.zeros(E, dtype=f)
    gamma, lam = f(gamma), f(lam)
    for t in range(T - 1, -1, -1):
        nv = v[t + 1] if t < T - 1 else lv
        g = gamma * np.where(d[t], f(0), f(1)).astype(f)
        if order == 0:
            adv = (r[t] - v[t]) + g * (nv + lam * adv)
        else:
            adv = (r[t] + (g * nv + (g * lam) * adv)) - v[t]
        assert adv.dtype == f
        A[t] = adv
    return A, A + v


@pytest.mark.parametrize("T", [1, 60, 257])
@pytest.mark.parametrize("rate", [0.0, 0.02, 1.0])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_bound_admits_float32_evaluations(T, rate, scale):
    """Before any GPU visit: a correct float32 implementation, in either operation order, is inside the derived bound — raw advantages,
    returns and the normalised advantages (moments in float64, as the kernel keeps them)."""
    E = 96
    r, v, d, lv = G.make_case(T, E, "random", scale=scale, seed=int(T * 7 + rate * 100 + scale), rate=rate)
    ref = G.reference(r, v, d, lv)
    out, b_norm = G.normalized(ref["A"], ref["bA"])
    for order in (0, 1):
        A, ret = _f32_eval(r, v, d, lv, 0.99, 0.95, order)
        G.check(A, ref["A"], ref["bA"], f"A order {order}")
        G.check(ret, ref["returns"], ref["b_returns"], f"returns order {order}")
        n, m, m2 = G.moments(A)
        mean_f, den_f = np.float32(m), np.float32(np.sqrt(m2 / (n - 1)) + 1e-8)
        assert np.isfinite(b_norm).all()
        G.check((A - mean_f) / den_f, out, b_norm, f"normalised order {order}")


def test_bound_is_not_vacuous():
    """One rounding error too many is outside it: a float32 evaluation with gamma off by 2^-18 relative fails the raw bound."""
    r, v, d, lv = G.make_case(60, 96, "none", seed=3)
    ref = G.reference(r, v, d, lv)
    A, _ = _f32_eval(r, v, d, lv, 0.99 * (1 + 2.0 ** -18), 0.95, 0)
    assert (np.abs(A.astype(np.float64) - ref["A"]) > ref["bA"]).any()


# ---- RolloutMemory on the CPU ------------------------------------------------------------------------------------------------------------
def _memory(ms=4, ne=3, **kw):
    from isaac_rover_amd.learning.rollout import RolloutMemory
    return RolloutMemory(ms, ne, device="cpu", **kw)


def test_memory_index_wrap_filled_and_len():
    m = _memory()
    m.create_tensor("rewards", 1)
    m.create_tensor("states", 5)
    assert len(m) == 0 and not m.filled and m.memory_index == 0
    for i in range(4):
        m.add_samples(rewards=torch.full((3,), float(i)), states=torch.full((3, 5), 10.0 + i))
        assert m.filled == (i == 3) and m.memory_index == (i + 1) % 4
        assert len(m) == (12 if i == 3 else 3 * (i + 1))
    assert m.get_tensor_by_name("rewards").shape == (4, 3, 1) and m.get_tensor_by_name("states", keepdim=False).shape == (12, 5)
    assert m.get_tensor_by_name("rewards")[:, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0]
    m.add_samples(rewards=torch.full((3, 1), 9.0), states=torch.zeros(3, 5))          # wraps: row 0 is overwritten
    assert m.memory_index == 1 and m.filled and m.get_tensor_by_name("rewards")[:, 0, 0].tolist() == [9.0, 1.0, 2.0, 3.0]
    m.reset()
    assert len(m) == 0 and not m.filled and m.memory_index == 0


def test_memory_checks_dtype_and_shape():
    m = _memory()
    m.create_tensor("actions", 2)
    m.create_tensor("terminated", 1, torch.bool)
    with pytest.raises(ValueError):
        m.add_samples(actions=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        m.add_samples(actions=torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        m.add_samples(terminated=torch.zeros(3, dtype=torch.float32))
    with pytest.raises(KeyError):
        m.add_samples(nothing=torch.zeros(3))
    with pytest.raises(ValueError):
        m.create_tensor("actions", 3)
    with pytest.raises(ValueError):
        m.set_tensor_by_name("actions", torch.zeros(4, 3, 1))
    assert m.memory_index == 0                                                         # a refused row stores nothing
    m.set_tensor_by_name("terminated", torch.ones(4, 3, dtype=torch.bool))
    assert bool(m.get_tensor_by_name("terminated").all())
    assert m.create_tensor("actions", 2) is m.get_tensor_by_name("actions")


def test_memory_reports_bytes():
    from isaac_rover_amd.learning.rollout import RolloutMemory
    lines = []
    m = _memory(report=lines.append)
    m.create_tensor("states", 5)
    m.create_tensor("terminated", 1, torch.bool)
    assert m.nbytes == 4 * 3 * 5 * 4 + 4 * 3 and "240 bytes" in lines[0] and "252 in all" in lines[1]
    assert RolloutMemory.bytes_for(60, 65536, {"states": (1750, torch.float32)}) == 60 * 65536 * 1750 * 4      # 27.5 GB


@pytest.mark.parametrize("mini_batches", [1, 2, 5, 7, 12])
def test_sample_all_partitions(mini_batches):
    m = _memory()
    n = 12
    m.create_tensor("ids", 1)
    m.create_tensor("pair", 2)
    m.set_tensor_by_name("ids", torch.arange(n, dtype=torch.float32).view(4, 3, 1))
    m.set_tensor_by_name("pair", torch.arange(2 * n, dtype=torch.float32).view(4, 3, 2))
    size = n // mini_batches
    plain = m.sample_all(["ids", "pair"], mini_batches)
    assert len(plain) == mini_batches and all(len(b) == 2 and b[0].shape == (size, 1) and b[1].shape == (size, 2) for b in plain)
    seen = torch.cat([b[0].view(-1) for b in plain]).tolist()
    assert seen == [float(i) for i in range(size * mini_batches)]                      # in order, no overlap, n % (mini_batches size) dropped
    assert n - len(seen) == n - mini_batches * size
    base = m.get_tensor_by_name("ids").untyped_storage().data_ptr()
    for i, b in enumerate(plain):                                                      # views: same storage, at the slice's offset
        assert b[0].untyped_storage().data_ptr() == base and b[0].storage_offset() == i * size and b[0].is_contiguous()
    g = lambda: torch.Generator().manual_seed(11)
    sh = m.sample_all(["ids", "pair"], mini_batches, shuffle=True, generator=g())
    again = m.sample_all(["ids", "pair"], mini_batches, shuffle=True, generator=g())
    ids = torch.cat([b[0].view(-1) for b in sh])
    assert len(set(ids.tolist())) == size * mini_batches and set(ids.tolist()) <= set(float(i) for i in range(n))
    assert ids.tolist() == torch.randperm(n, generator=g())[:size * mini_batches].float().tolist()
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(sh, again))
    assert all(torch.equal(b[1][:, 0], 2 * b[0][:, 0]) for b in sh)                    # rows stay together across names
    assert all(b[0].untyped_storage().data_ptr() != base for b in sh)


# ---- the moments' combine -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 500, 999])
def test_combine_moments_against_numpy(split):
    from isaac_rover_amd._lib import combine_moments
    x = np.random.default_rng(split).standard_normal(1000) * 3 + 100
    a, b = G.moments(x[:split]), G.moments(x[split:])
    for got in (combine_moments(a, b), combine_moments(torch.from_numpy(a), torch.from_numpy(b)).numpy(), combine_moments(list(b), tuple(a))):
        assert got[0] == 1000
        np.testing.assert_allclose(got[1], x.mean(), rtol=1e-14)
        np.testing.assert_allclose(got[2] / 999, x.var(ddof=1), rtol=1e-12)
    empty = np.zeros(3)
    np.testing.assert_array_equal(combine_moments(empty, a), a)
    np.testing.assert_array_equal(combine_moments(a, empty), a)
