"""The student's distillation loss and its gradients: the reference (torch autograd in float64 on exact f32 inputs), the yardstick (the
same autograd in float32 on the CPU), the rule a gradient is held to, and back-propagation through time written out by hand in f32 —
the written definition of what learning/student.py's backward computes, and the host of deliberately wrong variants.  No project code.

The loss is this project's definition (learning/distill.py):
    L = mean over B, T, A of (actions - teacher_actions)^2  +  recon_scale * mean over B, T, S + D of (estimated - target)^2
on the expression of student_ref.student_step_f32, one step after the other with a carried hidden state; ``reset`` [B, T] marks rows
whose step t starts from a zero state.

The rule.  A tensor passes when
    max |got - f64| <= YARD_FACTOR * max(gap, 2^-24 * max |f64|),      gap = max |f32 yardstick - f64|
with student_ref.YARD_FACTOR (16): the project's margin for another f32 evaluation of the same expression in another summation order.
The floor keeps a one-element tensor whose yardstick happens to be exact from demanding more than one rounding.
"""
import numpy as np
import torch

import student_ref as sr

FREE = "MLP.log_std_parameter"          # takes no part in the loss: no gradient


def unroll(sd, info, x, h0, reset=None):
    """T steps of student_ref.student_step_f32 in sd's dtype: x [B, T, F], h0 [L, B, H] -> (actions [B, T, A], estimated [B, T, S + D], h list)."""
    h, acts, ests = list(h0), [], []
    for t in range(x.shape[1]):
        a, s, h = sr.student_step_f32(sd, info, x[:, t], h, reset=None if reset is None else reset[:, t])
        acts.append(a)
        ests.append(s.expand(x.shape[0], -1))
    return torch.stack(acts, 1), torch.stack(ests, 1), h


def losses(actions, estimated, teacher, target, recon_scale):
    la, lr = ((actions - teacher) ** 2).mean(), ((estimated - target) ** 2).mean()
    return la + recon_scale * lr, la, lr


def autograd(sd, info, x, h0, reset, teacher, target, recon_scale, dtype):
    """-> ({parameter name: gradient, "dh0": gradient at h0}, (L, action loss, recon loss)) by torch autograd in ``dtype``."""
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(k != FREE) for k, v in sd.items()}
    h0 = h0.detach().to(dtype).clone().requires_grad_(True)
    a, s, _ = unroll(leaf, info, x.to(dtype), h0, reset)
    ls = losses(a, s, teacher.to(dtype), target.to(dtype), recon_scale)
    ls[0].backward()
    g = {k: v.grad.detach() for k, v in leaf.items() if k != FREE}
    g["dh0"] = h0.grad.detach()
    return g, tuple(v.detach() for v in ls)


def verdict(got, want, yard):
    """The rule above -> (ok, max |got - f64|, gap, allowed)."""
    want = sr.f64(want)
    d, gap = float((sr.f64(got) - want).abs().max()), sr.yard_gap(yard, want)
    allowed = sr.YARD_FACTOR * max(gap, sr.U * float(want.abs().max()))
    return d <= allowed, d, gap, allowed


def check_all(got, want, yard, names=None, label=""):
    """Every tensor of ``names`` (default: all of ``want``) by the rule; prints each figure, -> the names that fail."""
    bad = []
    for k in (names or want):
        ok, d, gap, allowed = verdict(got[k], want[k], yard[k])
        print(f"{label}{k}: max |d| {d:.3e}  gap {gap:.3e}  allowed {allowed:.3e}  d / gap {d / gap if gap > 0 else float('inf'):.2f}{'' if ok else '   FAILS'}")
        if not ok:
            bad.append(k)
    return bad


# ---- back-propagation through time by hand, f32 --------------------------------------------------------------------------------------
VARIANTS = ("dgh_n_without_r", "dh_in_without_gz", "reset_passes_dh_in", "dw_hh_unmasked_h_in", "decoder_grad_all_rows")


def _names(sd, prefix):
    """[(weight name, bias name, activation)] of a chain, as student_ref._chain_names orders it"""
    out, i = [], 0
    while True:
        if f"{prefix}.{i}.layer.0.weight" in sd:
            out.append((f"{prefix}.{i}.layer.0.weight", f"{prefix}.{i}.layer.0.bias", "leakyrelu"))
        elif f"{prefix}.{i}.weight" in sd:
            out.append((f"{prefix}.{i}.weight", f"{prefix}.{i}.bias", "tanh"))
        else:
            return out
        i += 1


def _chain_fwd(sd, names, v):
    ys = [v]
    for w, b, act in names:
        ys.append(sr.linear(ys[-1], sd[w], sd[b], act))
    return ys


def _chain_bwd(sd, names, ys, dy, grads):
    """dz = dy act'(y) from the stored output; dW = dz^T x, db = column sums, dx = dz W -> dx at the chain's input"""
    for i in range(len(names) - 1, -1, -1):
        w, b, act = names[i]
        y = ys[i + 1]
        dz = dy * (torch.where(y > 0, torch.ones_like(y), torch.full_like(y, sr.LEAKY)) if act == "leakyrelu" else 1 - y * y)
        grads[w], grads[b] = dz.T @ ys[i], dz.sum(0)
        dy = dz @ sd[w]
    return dy


def bptt_f32(sd, info, x, h0, reset, teacher, target, recon_scale, variant=None):
    """The same gradients as autograd(), by the formulas of rover_gru_cell_backward and the stages of StudentPolicy.backward, in the
    dtype of ``sd`` (float32).  Time-major inside: row t B + b.  ``variant``: one of VARIANTS — a deliberately WRONG backward."""
    assert variant is None or variant in VARIANTS, variant
    p, ns, nd = info["proprioceptive"], info["sparse"], info["dense"]
    bsz, t_len, f = x.shape
    ex, rows = ns + nd, bsz * x.shape[1]
    n_layers, hd = h0.shape[0], h0.shape[2]
    xt = x.transpose(0, 1).reshape(rows, f)
    rs = None if reset is None else reset.bool().T                   # [T, B]
    enc1, enc2 = _names(sd, "encoder1.encoder"), _names(sd, "encoder2.encoder")
    gb, ga, mlp = _names(sd, "belief_encoder.gb"), _names(sd, "belief_encoder.ga"), _names(sd, "MLP.network")
    gate_n, dec_n = _names(sd, "belief_decoder.gate_encoder"), _names(sd, "belief_decoder.decoder")
    # ---- forward, keeping every layer's output
    prop, ext = xt[:, :p], xt[:, f - ex:]
    y1, y2 = _chain_fwd(sd, enc1, xt[:, f - ex:f - nd]), _chain_fwd(sd, enc2, xt[:, f - nd:])
    l_e = torch.cat((y1[-1], y2[-1]), 1)
    seq = torch.cat((prop, l_e), 1).view(t_len, bsz, -1)
    xs, hins, gates, outs = [], [], [], []
    for l in range(n_layers):
        w_ih, w_hh, b_ih, b_hh = (sd[f"belief_encoder.gru.{nm}_l{l}"] for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        out, hin, gt = [], [], []
        for t in range(t_len):
            h = h0[l] if t == 0 else out[-1]
            raw = h
            if rs is not None:
                h = torch.where(rs[t][:, None], torch.zeros_like(h), h)
            gi, gh = seq[t] @ w_ih.T + b_ih, h @ w_hh.T + b_hh
            r, z = torch.sigmoid(gi[:, :hd] + gh[:, :hd]), torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
            q = gh[:, 2 * hd:]
            n = torch.tanh(gi[:, 2 * hd:] + r * q)
            out.append((1 - z) * n + z * h)
            hin.append((h, raw))
            gt.append((r, z, n, q))
        xs.append(seq); hins.append(hin); gates.append(gt)
        seq = torch.stack(out)
        outs.append(seq)
    top = seq.reshape(rows, hd)
    yb, ya = _chain_fwd(sd, gb, top), _chain_fwd(sd, ga, top)
    sg = torch.sigmoid(ya[-1])
    belief = yb[-1] + l_e * sg
    ym = _chain_fwd(sd, mlp, torch.cat((prop, belief), 1))
    last = seq[:, bsz - 1]                                           # [T, H]
    yg, yd = _chain_fwd(sd, gate_n, last), _chain_fwd(sd, dec_n, last)
    e3 = ext.view(t_len, bsz, ex)
    sgate = torch.sigmoid(yg[-1])
    est = yd[-1][:, None, :] + e3 * sgate[:, None, :]                # [T, B, ex]
    actions = ym[-1].view(t_len, bsz, -1)
    ta, tg = teacher.transpose(0, 1), target.transpose(0, 1)
    ls = losses(actions, est, ta, tg, recon_scale)
    # ---- backward
    g = {}
    d_act = (2.0 / actions.numel()) * (actions - ta)
    d_est = (2.0 * recon_scale / est.numel()) * (est - tg)
    d_mlp_in = _chain_bwd(sd, mlp, ym, d_act.reshape(rows, -1), g)
    d_bel = d_mlp_in[:, p:]
    d_le = d_bel * sg
    d_xa = (d_bel * l_e) * (sg * (1 - sg))
    d_top = _chain_bwd(sd, gb, yb, d_bel, g) + _chain_bwd(sd, ga, ya, d_xa, g)
    d_dec = d_est.sum(1)
    d_gate = ((d_est * e3) * (sgate * (1 - sgate))[:, None, :]).sum(1)
    d_last = _chain_bwd(sd, dec_n, yd, d_dec, g) + _chain_bwd(sd, gate_n, yg, d_gate, g)
    d_top = d_top.view(t_len, bsz, hd).clone()
    if variant == "decoder_grad_all_rows":
        d_top += d_last[:, None, :] / bsz
    else:
        d_top[:, bsz - 1] += d_last
    dh_above, dh0 = d_top, []
    for l in range(n_layers - 1, -1, -1):
        w_ih, w_hh = sd[f"belief_encoder.gru.weight_ih_l{l}"], sd[f"belief_encoder.gru.weight_hh_l{l}"]
        dgi, dgh, dh_next = [None] * t_len, [None] * t_len, None
        for t in range(t_len - 1, -1, -1):
            (r, z, n, q), (h, _) = gates[l][t], hins[l][t]
            gr = dh_above[t] if dh_next is None else dh_above[t] + dh_next
            a_n = (gr * (1 - z)) * (1 - n * n)
            a_z = (gr * (h - n)) * (z * (1 - z))
            a_r = (a_n * q) * (r * (1 - r))
            dgi[t] = torch.cat((a_r, a_z, a_n), 1)
            dgh[t] = torch.cat((a_r, a_z, a_n if variant == "dgh_n_without_r" else a_n * r), 1)
            dh_next = dgh[t] @ w_hh
            if variant != "dh_in_without_gz":
                dh_next = dh_next + gr * z
            if rs is not None and variant != "reset_passes_dh_in":
                dh_next = torch.where(rs[t][:, None], torch.zeros_like(dh_next), dh_next)
        dh0.insert(0, dh_next)
        dgi, dgh = torch.stack(dgi).reshape(rows, -1), torch.stack(dgh).reshape(rows, -1)
        h_in = torch.stack([pair[1 if variant == "dw_hh_unmasked_h_in" else 0] for pair in hins[l]]).reshape(rows, hd)
        g[f"belief_encoder.gru.weight_ih_l{l}"], g[f"belief_encoder.gru.bias_ih_l{l}"] = dgi.T @ xs[l].reshape(rows, -1), dgi.sum(0)
        g[f"belief_encoder.gru.weight_hh_l{l}"], g[f"belief_encoder.gru.bias_hh_l{l}"] = dgh.T @ h_in, dgh.sum(0)
        dh_above = (dgi @ w_ih).view(t_len, bsz, -1)
    d_le = d_le + dh_above.reshape(rows, -1)[:, p:]
    ef = y1[-1].shape[1]
    _chain_bwd(sd, enc1, y1, d_le[:, :ef], g)
    _chain_bwd(sd, enc2, y2, d_le[:, ef:], g)
    g["dh0"] = torch.stack(dh0)
    return g, ls


# ---- the two data sets -----------------------------------------------------------------------------------------------------------------
def case_data(info, b, t_len, hd, n_layers, seed, with_resets, x=None, h0=None):
    """Seeded f32 inputs of one case: x [B, T, F] in (-1, 1), h0 at half that, teacher actions in (-1, 1), target = the row's own
    heightmap columns plus noise of 0.1 (the trainer's clean-versus-noised case), resets at two steps (rows 3 k at 2, rows 5 k + 1 at 4)."""
    g = torch.Generator().manual_seed(seed)
    f, ex = info["proprioceptive"] + info["sparse"] + info["dense"], info["sparse"] + info["dense"]
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    x = r(b, t_len, f) if x is None else torch.as_tensor(x)        # the fixture brings its own x and h0
    h0 = r(n_layers, b, hd) * 0.5 if h0 is None else torch.as_tensor(h0)
    teacher = r(b, t_len, info["actions"])
    target = (x[:, :, f - ex:] + 0.1 * r(b, t_len, ex)).contiguous()
    reset = None
    if with_resets:
        reset = torch.zeros(b, t_len, dtype=torch.bool)
        reset[torch.arange(b) % 3 == 0, min(2, t_len - 1)] = True
        reset[torch.arange(b) % 5 == 1, min(4, t_len - 1)] = True
    return dict(x=x, h0=h0, teacher=teacher, target=target, reset=reset)


def reference(sd, info, d, recon_scale):
    """-> (f64 gradients, f64 losses, f32 yardstick gradients, f32 losses) of data set ``d`` (case_data's keys)"""
    g64, l64 = autograd(sd, info, d["x"], d["h0"], d["reset"], d["teacher"], d["target"], recon_scale, torch.float64)
    g32, l32 = autograd(sd, info, d["x"], d["h0"], d["reset"], d["teacher"], d["target"], recon_scale, torch.float32)
    return g64, l64, g32, l32
