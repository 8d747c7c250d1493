"""GPU: rover_ppo_loss and rover_linear_backward (csrc/rover_train.hip) AT their decision boundaries, past their grid caps and on
non-finite rows — where tests/test_ppo_gpu.py stays away from them on purpose.

The threshold table (ppo_ref.ppo_threshold_case) holds rows built to be fragile: q exactly 0 in f32, |value - old| at value_clip and one
step outside it, adv = +-0.  Their judge is the float32 restatement ppo_ref.ppo_row_f32, not the float64 closed form: float64 finds
q ~ 1e-7 on the same f32 inputs and takes the other branch.  d_value has no transcendental function in it and the library is built with
-ffp-contract=off: the restatement predicts its bits on every row of every case here.  Everything else is held to the derived bounds
of ppo_ref.ppo_loss, told which rows have q = 0.

Inputs sit in NaN-trapped buffers, outputs in CANARY-trapped ones; every call runs twice and must give the same bits."""
import numpy as np
import pytest
import torch

import mlp_ref as R
import ppo_ref as P
from test_ppo_gpu import DEV, Guarded, _bits, _ppo_case, _ratio

pytestmark = pytest.mark.gpu

# PPO_BLOCK and PPO_MAX_BLOCKS as they stand in csrc/rover_train.hip and csrc/rover_internal.h: the sizes of test_ppo_loss_past_the_grid_cap
# are placed round these numbers.  A change of either constant must move the sizes with it.
PPO_BLOCK, PPO_MAX_BLOCKS = 256, 1024
PPO_CAP_ROWS = PPO_BLOCK * PPO_MAX_BLOCKS                              # 262 144 rows: the most one trip of the row loop covers
KEYS = ("mean", "log_std", "actions", "old_log_prob", "advantages", "value", "old_values", "returns")


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(8, device=0)
    yield e
    e.close()


def _ibits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _run_loss(eng, d, cfg):
    """One rover_ppo_loss on trapped inputs and guarded outputs, twice: intact guards, the same bits -> {name: tensor} (clones)."""
    m, A = d["mean"].shape
    t = {k: d[k].to(DEV) for k in KEYS}
    t["mean"], t["actions"] = R.trapped_input(t["mean"], 1), R.trapped_input(t["actions"], 3)
    for k in KEYS:
        if k not in ("mean", "actions"):
            t[k] = R.nan_head(t[k])
    out = {"d_mean": R.Canary(m, A, DEV), "d_value": Guarded((m,)), "d_log_std": Guarded((A,)), "stats": Guarded((4,), torch.float64)}
    call = lambda: eng.ppo_loss(*[t[k] for k in KEYS], out["d_mean"].y, out["d_value"].y, out["d_log_std"].y, out["stats"].y, **cfg)
    call()
    torch.cuda.synchronize()
    first = {k: o.y.clone() for k, o in out.items()}
    for o in out.values():
        assert o.intact(), "a write outside an output"
        o.y.fill_(float("nan"))
    call()
    torch.cuda.synchronize()
    for k, o in out.items():
        assert torch.equal(_ibits(o.y), _ibits(first[k])), f"{k} differs on the second run"
        assert o.intact()
    return first


def _same_bits(got, want32):
    """A float32 device tensor against a numpy float32 array, bit for bit -> the number of differing elements."""
    return int((got.cpu().numpy().view(np.int32) != np.ascontiguousarray(want32).view(np.int32)).sum())


# ---- the threshold table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 16])
def test_ppo_loss_threshold_table(eng, A):
    cfgs = {"ratio_clip=0": dict(P.THRESHOLD_CFG, ratio_clip=0.0), "ratio_clip=0.2": dict(P.THRESHOLD_CFG),
            "no_value_clip": dict(P.THRESHOLD_CFG, clip_predicted_values=False), "value_clip=0": dict(P.THRESHOLD_CFG, value_clip=0.0)}
    exact_bits = {}
    for name, cfg in cfgs.items():
        d, info = P.ppo_threshold_case(A, cfg)
        r32 = P.ppo_row_f32(d, cfg)
        want, bound, fragile = P.ppo_loss(d, cfg, zero_q=info["zero_q"])
        assert np.array_equal(fragile.numpy(), info["fragile"])          # exactly the rows built to be
        got = _run_loss(eng, d, cfg)
        exact, zq = r32["exact"], info["zero_q"].numpy()
        assert np.array_equal(exact, zq)
        dv = (d["value"] - d["old_values"]).numpy()
        vc = np.float32(cfg["value_clip"])
        print(f"table A={A} {name}: rows {len(zq)}; q == 0: {int(zq.sum())}; ratio passes {int(r32['rpass'].sum())} / blocked {int((~r32['rpass']).sum())}; "
              f"value passes {int(r32['vpass'].sum())} / blocked {int((~r32['vpass']).sum())}; dv == +vc: {int((dv == vc).sum())}, dv == -vc: {int((dv == -vc).sum())}, "
              f"one step outside: {int(((np.abs(dv) > vc) & (np.abs(dv) <= vc + np.float32(2.0 ** -24))).sum())}; adv +0: {int((info['adv_kind'] == 2).sum())}, "
              f"adv -0: {int((info['adv_kind'] == 3).sum())}; fragile {int(info['fragile'].sum())}")
        # d_value: the restatement's bits on every row
        assert _same_bits(got["d_value"], r32["d_value"]) == 0, f"{name}: d_value differs from the f32 restatement"
        # d_mean on the q == 0 rows: the restatement's number (-0 equals +0)
        dm = got["d_mean"].cpu().numpy()
        assert not np.isnan(r32["d_mean"][exact]).any() and np.array_equal(dm[exact], r32["d_mean"][exact]), f"{name}: d_mean on the q == 0 rows"
        exact_bits[name] = dm[exact].view(np.int32).copy()
        # off them, under ratio_clip = 0: +-0 where adv r >= adv clamp(r), within the bound elsewhere
        if name == "ratio_clip=0":
            blocked = ~exact & ~r32["rpass"]
            assert int(blocked.sum()) == 42 and bool((dm[blocked] == 0).all())
            assert int((~exact & r32["rpass"]).sum()) == 14
        ratios = {k: _ratio(got[k].cpu(), want[k], bound[k]) for k in ("d_mean", "d_log_std", "stats")}
        print(f"table A={A} {name}: error / bound " + " ".join(f"{a} {b:.3f}" for a, b in ratios.items()) + "; d_value: bit-equal")
    # r = 1 passes on the edge exactly as it passes inside: the same d_mean bits on the q == 0 rows
    assert np.array_equal(exact_bits["ratio_clip=0"], exact_bits["ratio_clip=0.2"])


def test_ppo_loss_log_std_clamp_edges(eng):
    m = 65
    d, edges, outside = P.ppo_logstd_case(m, DEV)
    cfg = P.LOGSTD_CFG
    want, bound, fragile = P.ppo_loss(d, cfg)
    assert not bool(fragile.any())
    got = _run_loss(eng, d, cfg)
    ratios = {k: _ratio(got[k], want[k], bound[k]) for k in ("d_mean", "d_value", "d_log_std", "stats")}
    dl = got["d_log_std"].cpu().numpy()
    print(f"log_std clamp M={m} A=16: on the edges {[float(dl[j]) for j in edges]}, one ulp outside {[float(dl[j]) for j in outside]}; error / bound "
          + " ".join(f"{a} {b:.3f}" for a, b in ratios.items()))
    assert all(dl[j] == 0.0 and not np.signbit(dl[j]) for j in outside)
    assert all(dl[j] != 0.0 for j in edges) and bool((dl[4:] != 0.0).all())
    assert _same_bits(got["d_value"], P.ppo_row_f32(d, cfg)["d_value"]) == 0


# ---- past the grid caps ----------------------------------------------------------------------------------------------------------------
BIG = [(65536, 2), (65537, 2), (65537, 1), (PPO_CAP_ROWS, 2), (PPO_CAP_ROWS + 1, 2), (PPO_CAP_ROWS + 1, 16), (3 * PPO_CAP_ROWS + 5, 2)]


@pytest.mark.parametrize("m,A", BIG, ids=lambda v: str(v))
def test_ppo_loss_past_the_grid_cap(eng, m, A):
    """256 / 257 partials (the finishing kernel's second trip), the row loop at its cap, one row past it, and three trips with a ragged
    tail — through the existing _ppo_case, and d_value bit for bit against the restatement."""
    blocks = min(-(-m // PPO_BLOCK), PPO_MAX_BLOCKS)
    print(f"ppo_loss M={m} A={A}: {blocks} blocks = {blocks} partials, {-(-m // PPO_CAP_ROWS)} trip(s) of the row loop, "
          f"{-(-blocks // PPO_BLOCK)} trip(s) of the finishing kernel's partial loop")
    cfg = dict(P.PPO_CFG)
    if m % 2:
        cfg.update(entropy_loss_scale=0.01, value_loss_scale=0.5)
    # ppo_data draws value - old from a continuous range across value_clip: among hundreds of thousands of rows a seed now and then puts
    # one within 4 u of the edge.  As backward_data does, take the first seed from m + A on whose data has no fragile row; _ppo_case
    # asserts that again on the same data (its log_std table, restated here).
    ls = {1: [0.3 if m % 2 else 2.5], 2: [-0.4, 2.5], 16: [-21.0] + [0.1 * (j - 8) for j in range(15)]}[A]
    for seed in range(m + A, m + A + 40):
        d = P.ppo_data(m, A, seed, DEV, log_std=ls, cfg=cfg)
        if not bool(P.ppo_loss(d, cfg)[2].any()):
            break
    else:
        raise AssertionError(f"no seed in [{m + A}, {m + A + 40}) gives M={m} A={A} without a fragile row")
    print(f"ppo_loss M={m} A={A}: seed {seed}")
    _ppo_case(eng, m, A, cfg, seed=seed)
    got = _run_loss(eng, d, cfg)
    bad = _same_bits(got["d_value"], P.ppo_row_f32(d, cfg)["d_value"])
    print(f"ppo_loss M={m} A={A}: d_value differs from the restatement on {bad} rows")
    assert bad == 0


# ---- non-finite rows -------------------------------------------------------------------------------------------------------------------
def test_ppo_loss_nonfinite_rows_stay_in_their_rows(eng):
    m, A, i_nan, i_inf = 65, 2, 13, 40
    cfg = dict(P.PPO_CFG)
    clean = P.ppo_data(m, A, 5, "cpu", cfg=cfg)
    clean["advantages"][i_nan], clean["advantages"][i_inf] = 0.5, -0.75
    d = {k: v.clone() for k, v in clean.items()}
    d["advantages"][i_nan] = float("nan")
    d["old_log_prob"][i_inf] = float("-inf")
    got, ref = _run_loss(eng, d, cfg), _run_loss(eng, clean, cfg)
    other = torch.ones(m, dtype=torch.bool)
    other[[i_nan, i_inf]] = False
    for k in ("d_mean", "d_value"):
        assert torch.equal(_bits(got[k].cpu()[other]), _bits(ref[k].cpu()[other])), f"{k}: a non-finite row leaked into another row"
    assert bool(torch.isnan(got["d_mean"][i_nan]).all())
    assert bool(torch.isfinite(got["d_value"]).all()) and bool(torch.isfinite(ref["stats"]).all())
    # the same expressions in float64 torch on the CPU say which outputs are NaN and which +-Inf
    D = {k: v.double() for k, v in d.items()}
    mean, ls, value = (D[k].clone().requires_grad_(True) for k in ("mean", "log_std", "value"))
    pol, val, ent, kl = P.ppo_loss_expr(mean, ls, value, D, cfg)
    (pol + val + ent).backward()
    pat = lambda t: torch.where(torch.isnan(t), 3, torch.where(torch.isinf(t), torch.where(t > 0, 1, 2), 0)).tolist()
    stats64 = torch.stack((pol, val, ent, kl)).detach()
    print(f"non-finite rows: stats {got['stats'].tolist()} (float64 torch: {stats64.tolist()}); d_mean[NaN adv] {got['d_mean'][i_nan].tolist()}, "
          f"d_mean[old_log_prob -Inf] {got['d_mean'][i_inf].tolist()} (autograd: {mean.grad[i_inf].tolist()})")
    assert pat(got["stats"].cpu()) == pat(stats64)
    assert pat(stats64)[0] == 3 and pat(stats64)[3] in (1, 3) and pat(stats64)[1] == 0
    want, _, _ = P.ppo_loss(d, cfg)
    assert pat(got["d_mean"].cpu()) == pat(want["d_mean"])               # and the closed form of the header, element for element


# ---- the backward's derivative at y = 0, |y| = 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", R.ACTS)
def test_linear_backward_branch_points(eng, act):
    """x = W = the 33 x 33 identity: dW[n][k] = dz[k][n] and dx = dz exactly, whatever the summation order (every other term is a finite
    value times 0), so the f32 restatement of dy * act'(y) is the expected number on all 1 089 entries."""
    n = 33
    y, dy = P.branch_point_case(n)
    dz = P.branch_point_dz(y, dy, act)
    eye = torch.eye(n, device=DEV)
    yt, dyt = torch.from_numpy(y).to(DEV), torch.from_numpy(dy).to(DEV)
    want, bound = P.linear_backward(eye, yt, dyt, eye, act)
    xt, ytr, dytr, wt = R.trapped_input(eye, 1), R.trapped_input(yt, 3), R.trapped_input(dyt, 1), R.nan_head(eye)
    dx, dw, db = R.Canary(n, n, DEV), Guarded((n, n)), Guarded((n,))
    call = lambda: eng.linear_backward(xt, ytr, dytr, wt, act, dx=dx.y, dweight=dw.y, dbias=db.y)
    call()
    torch.cuda.synchronize()
    first = [o.y.clone() for o in (dx, dw, db)]
    for o in (dx, dw, db):
        assert o.intact()
        o.y.fill_(float("nan"))
    call()
    torch.cuda.synchronize()
    for o, f in zip((dx, dw, db), first):
        assert torch.equal(_bits(o.y), _bits(f)) and o.intact()
    gx, gw = first[0].cpu().numpy(), first[1].cpu().numpy()
    at0, at1 = y == 0, np.abs(y) == 1
    print(f"branch points {act} ({eng.linear_backward_route(n, n, n, True)}): y = +0: {int((at0 & ~np.signbit(y)).sum())}, y = -0: {int((at0 & np.signbit(y)).sum())}, "
          f"|y| = 1: {int(at1.sum())}; dx != dz on {int((gx != dz).sum())}, dW != dz^T on {int((gw != dz.T).sum())} of {dz.size}; "
          f"db error / bound {_ratio(first[2], want['db'], bound['db']):.3f}")
    assert np.array_equal(gx, dz), f"{act}: dx is not dy * act'(y)"
    assert np.array_equal(gw, dz.T), f"{act}: dW is not (dy * act'(y))^T"
