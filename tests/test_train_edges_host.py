"""CPU: the training kernels' decision boundaries, on the references alone (tests/ppo_ref.py, tests/gae_ref.py).

The threshold table of ppo_ref.ppo_threshold_case holds rows that are FRAGILE on purpose: q exactly 0 in f32 (old_log_prob = the row's
own f32 log-probability), so that with ratio_clip = 0 the ratio r = 1 sits on both clip edges; |value - old| exactly at value_clip and
one step outside it; adv = +-0, which ties adv r with adv clamp(r).  The float64 closed form cannot judge those rows from the f32
inputs — its q is ~1e-7, not 0 — so the judge of every decision is the float32 restatement ppo_row_f32, and the closed form is told
which rows have q = 0 (ppo_loss(zero_q=...)).  Here: (a) the closed form with that replacement equals float64 autograd with the same
replacement; (b) the table tells every comparison from its slip (< for <=, <= for <) — the five of ppo_loss_kernel on the table, the
two of ppo_finish_kernel on the log-std case; (c) the fragile rows are exactly the built ones."""
import numpy as np
import pytest
import torch

import gae_ref as G
import ppo_ref as P

TABLE_CFGS = {"ratio_clip=0": dict(P.THRESHOLD_CFG, ratio_clip=0.0), "ratio_clip=0.2": dict(P.THRESHOLD_CFG),
              "no_value_clip": dict(P.THRESHOLD_CFG, clip_predicted_values=False), "value_clip=0": dict(P.THRESHOLD_CFG, value_clip=0.0)}
ROW_FLIPS = ("lo<=r", "r<=hi", "s1<s2", "-vc<=dv", "dv<=vc")
ROW_KEYS = ("q", "r", "rpass", "vpass", "d_value", "d_mean")


def _same(a, b):
    """Two results of ppo_row_f32 hold the same flags and the same float bits."""
    for k in ROW_KEYS + ("ls_pass",):
        x, y = a[k], b[k]
        if x.dtype == np.float32:
            x, y = x.view(np.int32), y.view(np.int32)
        if not np.array_equal(x, y):
            return False
    return True


def test_threshold_values_are_what_the_table_says():
    v, old, vc = np.asarray(P.THRESHOLD_VALUES), np.float32(0.5), np.float32(0.25)
    dv = v - old
    assert dv.dtype == np.float32
    # one ulp of 0.75 (2^-24) above the edge: exact, two f32 steps past 0.25
    assert dv[0] == vc and float(dv[1]) == 0.25 + 2.0 ** -24 and dv[2] == -vc and dv[4] == np.float32(0.6) - old and dv[5] == 0
    assert dv[6] == np.nextafter(-vc, np.float32(-1))
    # nextafter(0.25, 0) - 0.5 is a tie in f32 and rounds to -0.25: ON the edge for the kernel, one step outside for float64
    assert dv[3] == -vc and float(v[3]) - 0.5 == -(0.25 + 2.0 ** -26)
    adv = P.ppo_threshold_case(1, TABLE_CFGS["ratio_clip=0"])[0]["advantages"].numpy()
    kinds = P.ppo_threshold_case(1, TABLE_CFGS["ratio_clip=0"])[1]["adv_kind"]
    assert (adv[kinds == 0] > 0).all() and (adv[kinds == 1] < 0).all()
    assert (adv[kinds == 2] == 0).all() and not np.signbit(adv[kinds == 2]).any() and (adv[kinds == 3] == 0).all() and np.signbit(adv[kinds == 3]).all()


@pytest.mark.parametrize("name", list(TABLE_CFGS))
@pytest.mark.parametrize("A", [1, 2, 16])
def test_threshold_table_closed_form_matches_autograd(A, name):
    """(a) and (c): float64 autograd of ppo_loss_expr with the forced-zero rows' old_log_prob replaced by the float64 lp, against the
    closed form given the same rows, to 1e-12 relative; fragile() marks exactly the constructed rows."""
    cfg = TABLE_CFGS[name]
    d, info = P.ppo_threshold_case(A, cfg)
    want, _, fragile = P.ppo_loss(d, cfg, zero_q=info["zero_q"])
    assert np.array_equal(fragile.numpy(), info["fragile"]), (np.flatnonzero(fragile.numpy()), np.flatnonzero(info["fragile"]))
    assert int(info["zero_q"].sum()) == 28
    D = {k: v.double() for k, v in d.items()}
    D["old_log_prob"] = torch.where(info["zero_q"], P.ppo_lp64(d, cfg), D["old_log_prob"])
    mean, ls, value = (D[k].clone().requires_grad_(True) for k in ("mean", "log_std", "value"))
    pol, val, ent, kl = P.ppo_loss_expr(mean, ls, value, D, cfg)
    (pol + val + ent).backward()
    for key, got, ref in (("d_mean", want["d_mean"], mean.grad), ("d_value", want["d_value"], value.grad), ("d_log_std", want["d_log_std"], ls.grad),
                          ("stats", want["stats"], torch.stack((pol, val, ent, kl)).detach())):
        scale = float(ref.abs().max())
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12 * scale), (key, float((got - ref).abs().max()), scale)
    # without the replacement float64 takes another branch on the q = 0 rows with ratio_clip = 0: that is why it is not their judge
    if name == "ratio_clip=0":
        plain, _, _ = P.ppo_loss(d, cfg)
        r32 = P.ppo_row_f32(d, cfg)
        rows = info["zero_q"].numpy() & (info["adv_kind"] < 2)
        assert bool(r32["rpass"][rows].all())
        zeroed = (plain["d_mean"].numpy()[rows] == 0).all(1)
        print(f"A={A}: float64 without the replacement zeroes d_mean on {int(zeroed.sum())} of {int(rows.sum())} q = 0 rows that f32 passes")
        assert zeroed.any()


@pytest.mark.parametrize("A", [1, 2, 16])
def test_threshold_table_tells_every_comparison_from_its_slip(A):
    """(b): each comparison of the restatement evaluated with the other operator changes its output on at least one row."""
    cfg = TABLE_CFGS["ratio_clip=0"]
    d, info = P.ppo_threshold_case(A, cfg)
    base = P.ppo_row_f32(d, cfg)
    assert _same(base, P.ppo_row_f32(d, cfg))
    for flip in ROW_FLIPS:
        got = P.ppo_row_f32(d, cfg, flip=flip)
        rows = np.flatnonzero((got["rpass"] != base["rpass"]) | (got["vpass"] != base["vpass"]))
        print(f"A={A} {flip}: {len(rows)} rows change")
        assert len(rows) > 0 and not _same(base, got), flip
        assert bool(info["fragile"][rows].all()) or flip == "s1<s2"      # the s1 = s2 ties are the adv = +-0 rows: a tie, not fragile
    # with ratio_clip = 0.2 every row of the table is inside the clip range: the ratio's comparisons are out of reach there
    cfg2 = TABLE_CFGS["ratio_clip=0.2"]
    d2, _ = P.ppo_threshold_case(A, cfg2)
    base2 = P.ppo_row_f32(d2, cfg2)
    assert bool(base2["rpass"].all())
    for flip in ("lo<=r", "r<=hi", "s1<s2"):
        assert _same(base2, P.ppo_row_f32(d2, cfg2, flip=flip))
    # value_clip = 0: dv = 0 sits on both value edges at once
    cfg0 = TABLE_CFGS["value_clip=0"]
    d0, _ = P.ppo_threshold_case(A, cfg0)
    for flip in ("-vc<=dv", "dv<=vc"):
        assert not _same(P.ppo_row_f32(d0, cfg0), P.ppo_row_f32(d0, cfg0, flip=flip))


def test_log_std_case_reaches_both_edges():
    d, edges, outside = P.ppo_logstd_case(65)
    cfg = P.LOGSTD_CFG
    want, _, fragile = P.ppo_loss(d, cfg)
    assert not bool(fragile.any())
    base = P.ppo_row_f32(d, cfg)
    assert base["ls_pass"].tolist() == [True, True, False, False] + [True] * 12
    assert P.ppo_row_f32(d, cfg, flip="min<=ls")["ls_pass"].tolist() == [False, True, False, False] + [True] * 12
    assert P.ppo_row_f32(d, cfg, flip="ls<=max")["ls_pass"].tolist() == [True, False, False, False] + [True] * 12
    dl = want["d_log_std"]
    assert all(float(dl[j]) == 0.0 for j in outside) and all(float(dl[j]) != 0.0 for j in edges)
    D = {k: v.double() for k, v in d.items()}
    ls = D["log_std"].clone().requires_grad_(True)
    pol, val, ent, _ = P.ppo_loss_expr(D["mean"], ls, D["value"], D, cfg)
    (pol + val + ent).backward()
    assert torch.allclose(dl, ls.grad, rtol=1e-12, atol=1e-12 * float(ls.grad.abs().max()))


def test_restatement_agrees_with_float64_off_the_edges():
    """On ppo_data (no fragile rows) the restatement's decisions are the closed form's, its d_value within the closed form's bound."""
    for A, m in ((1, 257), (2, 300), (16, 129)):
        d = P.ppo_data(m, A, seed=m + A, device="cpu")
        want, bound, fragile = P.ppo_loss(d, P.PPO_CFG)
        assert not bool(fragile.any())
        r = P.ppo_row_f32(d, P.PPO_CFG)
        assert bool((np.abs(r["d_value"].astype(np.float64) - want["d_value"].numpy()) <= bound["d_value"].numpy()).all())
        assert np.array_equal(r["vpass"], ((d["value"].double() - d["old_values"].double()).abs() <= P.F32(0.2)).numpy())
        assert np.array_equal(r["rpass"] | (d["advantages"].numpy() == 0), (want["d_mean"].numpy() != 0).any(1) | (d["advantages"].numpy() == 0))


def test_f64_summation_term_is_unchanged_at_the_old_sizes():
    for m in (1, 4097, 7892):
        assert max(2.0 ** -40, (m + 300) * 2.0 ** -53) == 2.0 ** -40
    assert (65536 + 300) * 2.0 ** -53 > 2.0 ** -40


# ---- the backward's derivative at y = 0, |y| = 1 ---------------------------------------------------------------------------------------
def test_branch_point_table_and_flip():
    y, dy = P.branch_point_case()
    assert np.isfinite(y).all() and np.isfinite(dy).all()
    tiny = np.finfo(np.float32).tiny
    assert ((y == 0) | (np.abs(y) >= tiny)).all()                       # no subnormal input
    pairs = {(float(a), bool(np.signbit(a)), float(b)) for a, b in zip(y.ravel(), dy.ravel())}
    assert len(pairs) == len(P.BRANCH_Y) * len(P.BRANCH_DY)             # +0 and -0 both occur, with every dy
    for act in ("none", "leakyrelu", "tanh", "relu", "elu"):
        dz, flipped = P.branch_point_dz(y, dy, act), P.branch_point_dz(y, dy, act, flip=True)
        assert dz.dtype == np.float32 and ((dz == 0) | (np.abs(dz) >= tiny)).all()
        # against the float64 derivative of ppo_ref.act_grad64: the same numbers wherever f32 is exact
        ref = dy.astype(np.float64) * P.act_grad64(torch.from_numpy(y), act).numpy()
        assert np.allclose(dz, ref, rtol=4 * 2.0 ** -24, atol=2 * 2.0 ** -24 * np.abs(dy).max())
        changed = int((dz != flipped).sum())
        print(f"{act}: y > 0 -> y >= 0 changes {changed} of {dz.size} dz")
        if act in ("leakyrelu", "relu"):
            assert changed > 0 and ((y == 0) | (dz == flipped)).all()
        else:
            assert changed == 0                                        # ELU: y + 1 = 1 at y = +-0, no visible branch there
    at0 = y == 0
    assert (P.act_grad_f32(y, "elu")[at0] == 1).all() and (P.act_grad_f32(y, "leakyrelu")[at0] == np.float32(0.01)).all()
    assert (P.act_grad_f32(y, "relu")[at0] == 0).all() and (P.act_grad_f32(y, "tanh")[np.abs(y) == 1] == 0).all()
    assert (P.act_grad_f32(y, "elu")[y == -1] == 0).all()


# ---- GAE: the non-finite case's float64 prediction --------------------------------------------------------------------------------------
def test_gae_nonfinite_case_reference():
    r, v, d, lv, cols = G.nonfinite_case(5, 130, seed=3)
    ref = G.reference_nonfinite(r, v, d, lv)
    A, ret = ref["A"], ref["returns"]
    ci, cn = cols["inf"], cols["nan"]
    other = np.ones(130, dtype=bool)
    other[[ci, cn]] = False
    assert np.isfinite(A[:, other]).all() and np.isfinite(ret[:, other]).all()
    # +Inf reward at t = 3 (done set): A = +Inf at t = 3, 2; the done at t = 1 multiplies by 0: NaN at t = 1, 0; t = 4 is clean
    assert np.isfinite(A[4, ci]) and A[3, ci] == np.inf and A[2, ci] == np.inf and np.isnan(A[1, ci]) and np.isnan(A[0, ci])
    # NaN value at t = 2: A NaN at t = 2 (its own value) and from there down (nv of t = 1); returns too
    assert np.isfinite(A[3:, cn]).all() and np.isnan(A[:3, cn]).all() and np.isnan(ret[:3, cn]).all()
    clean = G.reference(*G.cleaned(r, v, d, lv, cols)[:4])
    assert np.array_equal(clean["A"][:, other], A[:, other]) and np.array_equal(clean["returns"][:, other], ret[:, other])
