"""Float64 references and derived error bounds for the training kernels (csrc/rover_train.hip): the backward of one Layer, the PPO
minibatch loss with its gradients, and a torch-autograd restatement of both nets.  Torch, on the CPU or the GPU alike.

linear_backward.  The kernel forms dz = fl(dy * fl(act'(y))) in f32 and sums exact f32 products in f32 in some fixed order (an
f32-input MFMA is an fmaf chain; up to 64 split partials are added in order).  With u = 2^-24, gamma_n = n u / (1 - n u), dz in
float64 from the exact f32 dy and y, per element:

    e_dz = 4 u |dz| (+ 2 u |dy| for Tanh) + 2^-120
           none / LeakyReLU / ReLU: act' is exact, one rounding of the product (u |dz|); ELU: y + 1 rounds once more (3 u |dz|);
           Tanh: 1 - y*y carries u y^2 + u |1 - y^2| <= 2 u ABSOLUTE, so 2 u |dy| that does not shrink with dz
    B_dW = e_dz^T |x| + gamma_{M+66} (|dz| + e_dz)^T |x|          any summation order over M, up to 64 partials and the zero start
    B_db = colsum(e_dz) + gamma_{M+66} colsum(|dz| + e_dz)
    B_dx = e_dz |W| + gamma_{N+2} (|dz| + e_dz) |W|

ppo_loss.  Per row the kernel evaluates the formulas of include/rover_step.h in f32 (expf within 2 ulp, taken as 4 u); the bounds
below follow each rounding: rel(sigma) <= 4 u, rel(z) <= 7 u, rel(z^2) <= 16 u, so |lp_j - lp_j64| <= 18 u (z_j^2 / 2 + |ls'_j| + 0.919),
E_q = sum_j of that + gamma_A sum |lp_j| + u |q|, and rel(r) <= rho = 1.01 E_q + 4 u.  Rows whose r sits within 2 rho r of a clip edge,
whose |value - old| sits within 4 u of value_clip, or whose adv r ties adv clamp(r) outside the clip range are FRAGILE: f32 may take the
other branch there; test_ppo_* use data without such rows (fragile() says which).  The sums over M are f64: S = max(2^-40, (M + 300) 2^-53)
relative: a sum of n terms in ANY order is within (n - 1) 2^-53 of the exact one relative to the sum of magnitudes, and the M row terms
pass through fewer than 300 further additions (zero starts, 6 shuffle levels, 4 waves, up to 4 partials per thread, an 8-level tree).

The threshold tests (test_train_edges_*) BUILD fragile rows on purpose.  There float64 cannot be the judge: with old_log_prob set to the
row's own f32 log-probability the kernel's q is exactly 0 and r = 1 sits on a clip edge, while float64 on the same f32 inputs finds
q ~ 1e-7 and takes the other branch.  ppo_row_f32 restates the kernel's written f32 arithmetic in numpy float32 (one rounding per
written operation, -ffp-contract=off) and is the judge of the decisions and of every output that involves no transcendental function;
ppo_loss(zero_q=rows) takes those rows' q as exactly 0 and bounds the rest.
"""
import math

import numpy as np
import torch

from mlp_ref import LEAKY_SLOPE, TINY, U, act64, gamma

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
F32 = lambda v: float(np.float32(v))


# ---- the backward of one Layer ---------------------------------------------------------------------------------------------------
def act_grad64(y, act):
    y = y.double()
    one = torch.ones_like(y)
    if act in (None, "none"):
        return one
    if act == "leakyrelu":
        return torch.where(y > 0, one, LEAKY_SLOPE * one)
    if act == "relu":
        return torch.where(y > 0, one, 0 * one)
    if act == "tanh":
        return 1 - y * y
    if act == "elu":
        return torch.where(y > 0, one, y + 1)
    raise ValueError(act)


def linear_backward(x, y, dy, w, act):
    """-> {dx, dw, db} and {dx, dw, db} bounds (float64) of the Layer backward on exact f32 inputs."""
    m, n = dy.shape
    dz = dy.double() * act_grad64(y, act)
    e = 4 * U * dz.abs() + (2 * U * dy.double().abs() if act == "tanh" else 0) + TINY
    az, ax, aw = dz.abs() + e, x.double().abs(), w.double().abs()
    want = {"dx": dz @ w.double(), "dw": dz.T @ x.double(), "db": dz.sum(0)}
    bound = {"dx": e @ aw + gamma(n + 2) * (az @ aw) + TINY, "dw": e.T @ ax + gamma(m + 66) * (az.T @ ax) + TINY,
             "db": e.sum(0) + gamma(m + 66) * az.sum(0) + TINY}
    return want, bound


def _neighbour(n, device):
    return torch.clamp(torch.arange(n, device=device) ^ 1, max=n - 1)


def backward_mutations(x, y, dy, w, act):
    """-> {name: (x, y, dy)}: the last row dropped; dy read from the neighbouring row; act' taken at the neighbouring feature.  Each only
    where it can change something (with K = 0 every row has the same y and only db is computed: a row permutation of dy leaves it)."""
    m, n = dy.shape
    out = {}
    if m > 0:
        d = dy.clone()
        d[-1] = 0
        out["drop_last_row"] = (x, y, d)
    if m > 1 and x.shape[1] > 0:
        out["dy_row_neighbour"] = (x, y, dy[_neighbour(m, dy.device)])
    if n > 1 and act not in (None, "none"):
        out["act_feature_neighbour"] = (x, y[:, _neighbour(n, dy.device)], dy)
    return out


def backward_insensitive(x, y, dy, w, act, want, bound):
    miss = []
    for name, (xm, ym, dm) in backward_mutations(x, y, dy, w, act).items():
        got, _ = linear_backward(xm, ym, dm, w, act)
        keys = [k for k in ("dw", "db", "dx") if want[k].numel()]
        if not any(bool(((got[k] - want[k]).abs() > 2 * bound[k]).any()) for k in keys):
            miss.append(name)
    return miss


def backward_data(m, k, n, act, seed, device, tries=40):
    """x [m, k], w [n, k], y = act(x w^T + b) in f32 (what a forward would have stored), dy from [-1, 1] with its last row and odd
    rows at magnitude >= 0.5 — at the first seed from ``seed`` on that rejects every mutation -> (x, y, dy, w, want, bound)."""
    for s in range(seed, seed + tries):
        g = torch.Generator(device=device).manual_seed(s)
        rnd = lambda *sh: torch.rand(*sh, generator=g, device=device)
        x = rnd(m, k) * 4 - 2
        w = (rnd(n, k) * 2 - 1) / max(k, 1) ** 0.5
        b = rnd(n) * 2 - 1
        y = act64(x.double() @ w.double().T + b.double(), act).float()
        dy = rnd(m, n) * 2 - 1
        dy = torch.where(dy.abs() < 0.25, dy + 0.5, dy)
        want, bound = linear_backward(x, y, dy, w, act)
        if not backward_insensitive(x, y, dy, w, act, want, bound):
            return x, y, dy, w, want, bound
    raise AssertionError(f"no seed in [{seed}, {seed + tries}) makes M={m} K={k} N={n} {act} reject every mutation")


# ---- the PPO loss ------------------------------------------------------------------------------------------------------------------
PPO_CFG = dict(ratio_clip=0.2, value_clip=0.2, clip_predicted_values=True, entropy_loss_scale=0.0, value_loss_scale=1.0, clip_log_std=True,
               min_log_std=-20.0, max_log_std=2.0)


def _ls_clamped(log_std, cfg):
    ls = log_std.double()
    return torch.clamp(ls, F32(cfg["min_log_std"]), F32(cfg["max_log_std"])) if cfg["clip_log_std"] else ls


def ppo_loss_expr(mean, log_std, value, d, cfg):
    """The loss expressions on torch tensors of any dtype (autograd flows through mean, log_std, value) -> (policy, value, entropy, kl)."""
    ls = torch.clamp(log_std, F32(cfg["min_log_std"]), F32(cfg["max_log_std"])) if cfg["clip_log_std"] else log_std
    sigma = torch.exp(ls)
    z = (d["actions"] - mean) / sigma
    lp = ((-0.5 * (z * z) - ls) - HALF_LOG_2PI).sum(1)
    q = lp - d["old_log_prob"]
    r = torch.exp(q)
    c = F32(cfg["ratio_clip"])
    lo, hi = F32(np.float32(1) - np.float32(c)), F32(np.float32(1) + np.float32(c))
    adv = d["advantages"]
    policy = -torch.min(adv * r, adv * torch.clamp(r, lo, hi)).mean()
    vc = F32(cfg["value_clip"])
    vp = d["old_values"] + torch.clamp(value - d["old_values"], -vc, vc) if cfg["clip_predicted_values"] else value
    vloss = F32(cfg["value_loss_scale"]) * ((d["returns"] - vp) ** 2).mean()
    ent = -F32(cfg["entropy_loss_scale"]) * (0.5 + HALF_LOG_2PI + ls).expand(mean.shape[0], -1).mean()
    kl = ((r - 1) - q).mean()
    return policy, vloss, ent, kl


def ppo_lp64(d, cfg):
    """The row's log-probability in float64 on the exact f32 inputs, as ppo_loss and ppo_loss_expr both evaluate it."""
    ls = _ls_clamped(d["log_std"], cfg)
    z = (d["actions"].double() - d["mean"].double()) / torch.exp(ls)
    return ((-0.5 * z * z - ls) - HALF_LOG_2PI).sum(1)


def ppo_loss(d, cfg, zero_q=None):
    """The closed forms of include/rover_step.h in float64 on exact f32 inputs ``d`` (mean [M, A], log_std [A], actions, and the [M]
    arrays old_log_prob, advantages, value, old_values, returns) -> (out, bound, fragile): out / bound dicts over d_mean, d_value,
    d_log_std, stats; fragile: bool [M].  ``zero_q``: rows (index list or bool mask) whose q is taken as exactly 0 — their float64
    old_log_prob is replaced by this function's own float64 lp (rows built with old_log_prob = the f32 lp of ppo_row_f32)."""
    D = {k: v.double() for k, v in d.items()}
    mean, a = D["mean"], D["actions"]
    m, A = mean.shape
    ls = _ls_clamped(d["log_std"], cfg)
    sigma = torch.exp(ls)
    z = (a - mean) / sigma
    lpj = (-0.5 * z * z - ls) - HALF_LOG_2PI
    old_lp = D["old_log_prob"]
    if zero_q is not None:
        old_lp = old_lp.clone()
        old_lp[zero_q] = lpj.sum(1)[zero_q]
    q = lpj.sum(1) - old_lp
    r = torch.exp(q)
    c = F32(cfg["ratio_clip"])
    lo, hi = F32(np.float32(1) - np.float32(c)), F32(np.float32(1) + np.float32(c))
    adv = D["advantages"]
    rc = torch.clamp(r, lo, hi)
    s1, s2 = adv * r, adv * rc
    surr = torch.minimum(s1, s2)
    inside = (r >= lo) & (r <= hi)
    g = -(adv / m) * (inside | (s1 < s2)).double()
    t = g * r
    d_mean = t[:, None] * z / sigma
    ls_raw = D["log_std"]
    ls_pass = (((ls_raw >= F32(cfg["min_log_std"])) & (ls_raw <= F32(cfg["max_log_std"]))) if cfg["clip_log_std"] else torch.ones_like(ls_raw, dtype=torch.bool)).double()
    es, vls, vc = F32(cfg["entropy_loss_scale"]), F32(cfg["value_loss_scale"]), F32(cfg["value_clip"])
    term = t[:, None] * (z * z - 1)
    d_ls = ls_pass * (term.sum(0) - es / A)
    dv = D["value"] - D["old_values"]
    dvc = torch.clamp(dv, -vc, vc) if cfg["clip_predicted_values"] else dv
    vp = D["old_values"] + dvc if cfg["clip_predicted_values"] else D["value"]
    e = vp - D["returns"]
    vpass = (dv.abs() <= vc).double() if cfg["clip_predicted_values"] else torch.ones_like(dv)
    vscale = vls * 2.0 / m
    d_value = vscale * e * vpass
    klt = (r - 1) - q
    stats = torch.stack((-surr.mean(), vls * (e * e).mean(), torch.as_tensor(-es * (0.5 + HALF_LOG_2PI + float(ls.mean())), dtype=torch.float64, device=mean.device),
                         klt.mean()))
    # ---- bounds ----
    e_q = (18 * U * (0.5 * z * z + ls.abs() + HALF_LOG_2PI)).sum(1) + gamma(A) * lpj.abs().sum(1) + U * q.abs()
    rho = 1.01 * e_q + 4 * U
    e_e = 1.01 * U * (dvc.abs() + vp.abs() + e.abs())
    S = max(2.0 ** -40, (m + 300) * 2.0 ** -53)                         # f64 sums in any order; 2^-40 up to M = 7 892
    b_mean = 1.01 * d_mean.abs() * (rho[:, None] + 16 * U) + TINY
    b_value = 1.01 * abs(vscale) * e_e + 4 * U * d_value.abs() + TINY
    e_term = t.abs()[:, None] * (16 * U * z * z + U * (z * z - 1).abs()) + term.abs() * (rho[:, None] + 3 * U)
    b_ls = 1.01 * e_term.sum(0) + 2 * U * d_ls.abs() + S * term.abs().sum(0) + TINY
    b_stats = torch.stack(((surr.abs() * (rho + 2 * U)).mean() + S * surr.abs().mean(),
                           abs(vls) * (2 * e.abs() * e_e + e_e * e_e + U * e * e).mean() * 1.01 + S * (e * e).mean(),
                           torch.as_tensor(abs(es) * S * (2 + float(ls.abs().mean())), dtype=torch.float64, device=mean.device),
                           (rho * r + U * (r - 1).abs() + e_q + U * klt.abs()).mean() * 1.01 + S * klt.abs().mean())) + TINY
    fragile = ((r - lo).abs() <= 2 * rho * r) | ((r - hi).abs() <= 2 * rho * r) | (~inside & (s1 == s2) & (adv != 0))
    if cfg["clip_predicted_values"]:
        fragile |= (dv.abs() - vc).abs() <= 4 * U * (dv.abs() + D["value"].abs() + D["old_values"].abs())
    out = {"d_mean": d_mean, "d_value": d_value, "d_log_std": d_ls, "stats": stats}
    return out, {"d_mean": b_mean, "d_value": b_value, "d_log_std": b_ls, "stats": b_stats}, fragile


def ppo_data(m, A, seed, device, log_std=None, cfg=PPO_CFG):
    """A minibatch that reaches every branch: r inside, below and above the clip range with both signs of advantage (and a zero one),
    value - old inside and outside value_clip; log_std given or drawn from [-1, 0.5]."""
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=device)
    ls = (rnd(A) * 1.5 - 1) if log_std is None else torch.as_tensor(log_std, dtype=torch.float32, device=device)
    mean = rnd(m, A) * 2 - 1
    lsc = _ls_clamped(ls, cfg)
    actions = mean + torch.exp(lsc).float() * (rnd(m, A) * 4 - 2)
    z = (actions.double() - mean.double()) / torch.exp(lsc)
    lp = ((-0.5 * z * z - lsc) - HALF_LOG_2PI).sum(1)
    row = torch.arange(m, device=device)
    shift = torch.tensor([0.0, 0.05, -0.05, 0.5, -0.5, 0.3], dtype=torch.float64, device=device)[row % 6]      # log r
    old_lp = (lp - shift - 0.01 * (rnd(m).double() - 0.5)).float()
    adv = torch.where((row // 6) % 2 == 0, 1.0, -1.0).to(device) * (0.25 + rnd(m))
    adv[row % 11 == 7] = 0.0
    old_v = rnd(m) * 2 - 1
    value = old_v + torch.tensor([0.05, -0.1, 0.35, -0.5], device=device)[row % 4] * (0.5 + 0.5 * rnd(m))
    returns = old_v + rnd(m) - 0.5
    return {"mean": mean, "log_std": ls, "actions": actions, "old_log_prob": old_lp, "advantages": adv, "value": value, "old_values": old_v,
            "returns": returns}


# ---- one loss row restated in float32, and the threshold table ---------------------------------------------------------------------------
# the comparisons of ppo_loss_kernel and ppo_finish_kernel as written: name -> strict
PPO_COMPARISONS = {"lo<=r": False, "r<=hi": False, "s1<s2": True, "-vc<=dv": False, "dv<=vc": False, "min<=ls": False, "ls<=max": False}


def _np32(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32)


def _clamp32(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))                 # ppo_clamp: a NaN stays a NaN


def ppo_row_f32(d, cfg, flip=None):
    """The arithmetic printed above ppo_loss_kernel in numpy float32: one rounding per written operation, in the written order, j summed
    in order.  -> dict of numpy arrays: lp, q, r, rpass, vpass [M]; d_value [M] (no transcendental function enters it: the kernel's bits
    on every row); exact [M]: q == 0 and every clamped log_std is 0, so that sigma = r = 1 without trusting any exp; d_mean [M, A]
    (NaN off the exact rows); ls_pass [A], the finishing kernel's decision.  ``flip`` names one comparison of PPO_COMPARISONS to evaluate
    with the other operator (<= for <, < for <=): what a kernel with that slip would decide."""
    assert flip is None or flip in PPO_COMPARISONS
    f = np.float32

    def cmp(a, b, name):
        return a < b if PPO_COMPARISONS[name] != (flip == name) else a <= b

    x = {k: _np32(v) for k, v in d.items()}
    m, A = x["mean"].shape
    fm = f(m)
    c, vc, vls = f(cfg["ratio_clip"]), f(cfg["value_clip"]), f(cfg["value_loss_scale"])
    lo, hi = f(1) - c, f(1) + c
    vscale = vls * (f(2) / fm)
    mn, mx = f(cfg["min_log_std"]), f(cfg["max_log_std"])
    with np.errstate(all="ignore"):
        ls = _clamp32(x["log_std"], mn, mx) if cfg["clip_log_std"] else x["log_std"]
        sigma = np.exp(ls)
        z = (x["actions"] - x["mean"]) / sigma
        lp = None
        for j in range(A):
            l = (f(-0.5) * (z[:, j] * z[:, j]) - ls[j]) - f(0.91893853320467274)
            lp = l if j == 0 else lp + l
        q = lp - x["old_log_prob"]
        r = np.exp(q)
        adv = x["advantages"]
        s1, s2 = adv * r, adv * _clamp32(r, lo, hi)
        rpass = (cmp(lo, r, "lo<=r") & cmp(r, hi, "r<=hi")) | cmp(s1, s2, "s1<s2")
        t = (-(adv / fm) * np.where(rpass, f(1), f(0))) * r
        d_mean = (t[:, None] * z) / sigma
        dv = x["value"] - x["old_values"]
        clipv = bool(cfg["clip_predicted_values"])
        vp = x["old_values"] + _clamp32(dv, -vc, vc) if clipv else x["value"]
        e = vp - x["returns"]
        vpass = (cmp(-vc, dv, "-vc<=dv") & cmp(dv, vc, "dv<=vc")) if clipv else np.ones(m, dtype=bool)
        d_value = (vscale * e) * np.where(vpass, f(1), f(0))
        ls_pass = (cmp(mn, x["log_std"], "min<=ls") & cmp(x["log_std"], mx, "ls<=max")) if cfg["clip_log_std"] else np.ones(A, dtype=bool)
    exact = (q == 0) & bool((ls == 0).all())
    d_mean = np.where(exact[:, None], d_mean, f("nan"))
    for v in (lp, q, r, d_value, d_mean):
        assert v.dtype == np.float32
    return {"lp": lp, "q": q, "r": r, "rpass": rpass, "vpass": vpass, "d_value": d_value, "exact": exact, "d_mean": d_mean, "ls_pass": ls_pass}


THRESHOLD_CFG = dict(PPO_CFG, value_clip=0.25)
# value - old with old = 0.5, value_clip = 0.25.  All but one difference are exact in f32: nextafter(0.25, 0) - 0.5 = -(0.25 + 2^-26) is
# a tie between two floats and rounds to -0.25, so the kernel's dv sits ON the lower edge (and passes) where float64 sees it one step
# outside; 0.25 - 2^-25 is added so that the table also holds a row whose F32 dv is one ulp outside on that side.
THRESHOLD_VALUES = (np.float32(0.75), np.nextafter(np.float32(0.75), np.float32(1)), np.float32(0.25), np.nextafter(np.float32(0.25), np.float32(0)),
                    np.float32(0.6), np.float32(0.5), np.float32(0.25) - np.float32(2.0 ** -25))
THRESHOLD_ADV = ("pos", "neg", "+0", "-0")
THRESHOLD_Q = (0, 1, -1)                                               # q exactly 0, about +2^-6, about -2^-6


def ppo_threshold_case(A, cfg, device="cpu"):
    """The threshold table: log_std = 0, rows = THRESHOLD_Q x THRESHOLD_ADV x THRESHOLD_VALUES (84 rows), old_values = 0.5.
    old_log_prob is the row's f32 lp of ppo_row_f32 (q exactly 0 in the kernel) or that -+ 2^-6.  -> (d, info): info holds per row
    qsel / adv_kind / value_kind, zero_q (bool, the rows whose q the float64 reference must take as 0), and fragile: the rows that are
    fragile BY CONSTRUCTION under ``cfg`` — q == 0 with ratio_clip = 0 (r = 1 on both clip edges at once), and, with value clipping,
    |value - old| at value_clip or one step outside it."""
    g = torch.Generator().manual_seed(100 + A)
    nq, na, nv = len(THRESHOLD_Q), len(THRESHOLD_ADV), len(THRESHOLD_VALUES)
    m = nq * na * nv
    row = np.arange(m)
    qsel, adv_kind, value_kind = np.asarray(THRESHOLD_Q)[row // (na * nv)], (row // nv) % na, row % nv
    mean = torch.rand(m, A, generator=g) * 2 - 1
    actions = mean + (torch.rand(m, A, generator=g) * 4 - 2)
    mag = (0.25 + torch.rand(m, generator=g)).numpy()
    adv = np.select([adv_kind == 0, adv_kind == 1, adv_kind == 2], [mag, -mag, np.float32(0.0)], np.float32(-0.0)).astype(np.float32)
    value = np.asarray(THRESHOLD_VALUES, dtype=np.float32)[value_kind]
    d = {"mean": mean, "log_std": torch.zeros(A), "actions": actions, "old_log_prob": torch.zeros(m), "advantages": torch.from_numpy(adv),
         "value": torch.from_numpy(value), "old_values": torch.full((m,), 0.5), "returns": torch.rand(m, generator=g)}
    lp = ppo_row_f32(d, cfg)["lp"]
    d["old_log_prob"] = torch.from_numpy((lp - qsel.astype(np.float32) * np.float32(2.0 ** -6)).astype(np.float32))
    got = ppo_row_f32(d, cfg)
    assert bool(((got["q"] == 0) == (qsel == 0)).all()) and bool((np.abs(np.abs(got["q"][qsel != 0]) - 2.0 ** -6) < 2.0 ** -16).all())
    fragile = (qsel == 0) & (F32(cfg["ratio_clip"]) == 0.0)
    if cfg["clip_predicted_values"]:
        at_edge = {0.25: (0, 1, 2, 3, 6), 0.0: (5,)}[F32(cfg["value_clip"])]
        fragile = fragile | np.isin(value_kind, at_edge)
    info = {"qsel": qsel, "adv_kind": adv_kind, "value_kind": value_kind, "zero_q": torch.from_numpy(qsel == 0).to(device),
            "fragile": fragile}
    return {k: v.to(device) for k, v in d.items()}, info


LOGSTD_CFG = dict(PPO_CFG, min_log_std=-1.0, max_log_std=0.5)


def ppo_logstd_case(m, device="cpu", seed=77):
    """ppo_data rows with A = 16 under LOGSTD_CFG: log_std components exactly min, exactly max, one ulp below min, one ulp above max, the
    other twelve inside.  -> (d, edges, outside): the component indices on the two edges and the two one ulp outside."""
    mn, mx = np.float32(-1.0), np.float32(0.5)
    ls = [mn, mx, np.nextafter(mn, np.float32(-2)), np.nextafter(mx, np.float32(1))] + [np.float32(-0.9 + 0.11 * j) for j in range(12)]
    assert all(mn < v < mx for v in ls[4:]) and ls[2] < mn and ls[3] > mx
    return ppo_data(m, 16, seed, device, log_std=[float(v) for v in ls], cfg=LOGSTD_CFG), (0, 1), (2, 3)


# ---- the backward's derivative at its branch points -----------------------------------------------------------------------------------
FLT_MIN = float(np.finfo(np.float32).tiny)
BRANCH_Y = (0.0, -0.0, FLT_MIN, -FLT_MIN, 1e-3, -1e-3, 0.5, -0.5, 1.0, -1.0, float(np.nextafter(np.float32(1), np.float32(0))),
            float(np.nextafter(np.float32(-1), np.float32(0))), 2.5)
BRANCH_DY = (1.0, -2.0, 0.375, -0.0)


def act_grad_f32(y, act, flip=False):
    """act_grad_from_y of csrc/rover_train.hip in numpy float32: 1 - y*y in two roundings, y + 1 in one.  ``flip``: y >= 0 for y > 0."""
    f = np.float32
    y = np.asarray(y, dtype=f)
    pos = (y >= 0) if flip else (y > 0)
    one = np.ones_like(y)
    if act in (None, "none"):
        return one
    if act == "leakyrelu":
        return np.where(pos, one, f(0.01))
    if act == "tanh":
        return f(1) - y * y
    if act == "relu":
        return np.where(pos, one, f(0))
    if act == "elu":
        return np.where(pos, one, y + f(1))
    raise ValueError(act)


def branch_point_case(n=33):
    """y and dy [n, n] cycling through BRANCH_Y and BRANCH_DY (13 and 4 are coprime: every pair occurs), all finite and normal or zero."""
    i = np.arange(n * n)
    y = np.asarray(BRANCH_Y, dtype=np.float32)[i % len(BRANCH_Y)].reshape(n, n)
    dy = np.asarray(BRANCH_DY, dtype=np.float32)[i % len(BRANCH_DY)].reshape(n, n)
    return y, dy


def branch_point_dz(y, dy, act, flip=False):
    """dz = fl(dy * fl(act'(y))) as dz_at forms it (act 'none': dy itself)."""
    dy = np.asarray(dy, dtype=np.float32)
    return dy.copy() if act in (None, "none") else dy * act_grad_f32(y, act, flip)


# ---- both nets restated on torch autograd ------------------------------------------------------------------------------------------
def _act(z, act):
    if act == "leakyrelu":
        return torch.nn.functional.leaky_relu(z, LEAKY_SLOPE)
    if act == "tanh":
        return torch.tanh(z)
    return z


class TorchNet:
    """model.py's HeightmapNet from a ``state_dict`` (the reference's parameter names) as leaf tensors of ``dtype`` with
    requires_grad: forward(states) -> (output, hidden pre-activations), autograd does the rest."""

    def __init__(self, sd, dtype, device="cpu", activation="leakyrelu"):
        self.p = {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in sd.items()}
        self.act = activation
        self.head = "tanh" if "log_std_parameter" in sd else None
        self.ns = sd["encoder0.encoder.0.layer.0.weight"].shape[1]
        self.nd = sd["encoder1.encoder.0.layer.0.weight"].shape[1]
        self.ef = sd["encoder0.encoder.1.layer.0.weight"].shape[0]
        self.np = sd["network.0.layer.0.weight"].shape[1] - 2 * self.ef
        self.n_mlp = sum(1 for k in sd if k.startswith("network.") and k.endswith("weight"))

    def forward(self, states):
        p, pre = self.p, []
        s = states.to(next(iter(p.values())).dtype)
        parts = [s[:, :self.np]]
        for name, lo, n in (("encoder0", self.np, self.ns), ("encoder1", self.np + self.ns, self.nd)):
            h = s[:, lo:lo + n]
            for i in range(2):
                w = p[f"{name}.encoder.{i}.layer.0.weight"]
                zz = h @ w.T + p[f"{name}.encoder.{i}.layer.0.bias"]
                if w.shape[1] > 0:
                    pre.append(zz)
                h = _act(zz, self.act)
            parts.append(h)
        h = torch.cat(parts, 1)
        for i in range(self.n_mlp - 1):
            zz = h @ p[f"network.{i}.layer.0.weight"].T + p[f"network.{i}.layer.0.bias"]
            pre.append(zz)
            h = _act(zz, self.act)
        k = self.n_mlp - 1
        return _act(h @ p[f"network.{k}.weight"].T + p[f"network.{k}.bias"], self.head), pre
