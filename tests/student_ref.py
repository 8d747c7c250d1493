"""The GRU cell, the sigmoid gate and the whole recurrent student restated in float64 torch on exact f32 inputs, and the per-element
error bound the kernels are held to.  No project code.

Meaning (tasks/utils/learning_by_cheating/student_model.py, torch.nn.GRU): gate order r, z, n;
    r = sigmoid(x W_ir^T + b_ir + h W_hr^T + b_hr);  z likewise;  n = tanh(x W_in^T + b_in + r (h W_hn^T + b_hn));  h' = (1 - z) n + z h
ga's last Layer applies LeakyReLU before the Sigmoid; the decoder is fed the GRU's output SEQUENCE out [B, T, H] and takes out[-1],
the last batch row's.

The bound.  Every function below carries a pair (value in float64, err >= |f32 result - value| per element) and is first order in
u = 2^-24 (the unit roundoff of f32), as ppo_ref.py and optim_ref.py derive theirs:
  * a sum of n products in f32, in ANY order, errs by at most gamma_n sum|a||w|, gamma_n = n u / (1 - n u); a pre-activation over the
    reduction K + H with its two bias additions: gamma_{K+H+2} (|x||W_i|^T + |h||W_h|^T + |b_i| + |b_h|);
  * an input that is itself off by err_x moves the sum by at most err_x |W|^T;
  * expf and tanhf are allowed ULP_EXP = ULP_TANH = 2 ulp (1 ulp = 2 u relative; the device library documents 1 and 2),
    sigmoid(v) = 1 / (1 + expf(-v)) adds one rounding for the sum and one for the quotient: SIG_EVAL = (2 ULP_EXP + 2) u on a value <= 1;
  * sigmoid is 1/4-Lipschitz, tanh and LeakyReLU 1-Lipschitz;
  * through n = tanh(a + r g): err_a + err_r |g| + |r| err_g, three roundings on terms bounded by |a| + |r g|, then tanhf's;
  * through h' = (1 - z) n + z h: err_z (|n| + |h|) + |1 - z| err_n + |z| err_h, and four roundings on |(1 - z) n| + |z h|;
  * across time steps err_h is the previous step's bound on h, carried through the same expression (it is NOT assumed to contract).
Second-order terms (products of two errs) are dropped; SLACK = 1 + 2^-10 covers them, since every err here is below 2^-12.
The bound is derived, not fitted: test_student_host.py asserts that an f32 torch evaluation on the CPU lies inside it on every test
case's data and prints the worst error / bound ratio.
"""
import numpy as np
import torch

U = 2.0 ** -24
ULP_EXP = 2.0
ULP_TANH = 2.0
SIG_EVAL = (2.0 * ULP_EXP + 2.0) * U
TANH_EVAL = (2.0 * ULP_TANH + 1.0) * U
SLACK = 1.0 + 2.0 ** -10
LEAKY = 0.01


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(t):
    return torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).detach().cpu().to(torch.float64)


# ---- values: the same code runs in float64 (the reference) and in float32 (the yardstick) ---------------------------------
def act_fn(v, act):
    if act == "leakyrelu":
        return torch.where(v > 0, v, LEAKY * v)
    if act == "tanh":
        return torch.tanh(v)
    assert act is None, act
    return v


def linear(x, w, b, act):
    return act_fn(x @ w.T + b, act)


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, mask=None):
    if mask is not None:
        h = torch.where(mask.bool()[:, None], torch.zeros_like(h), h)
    hd = h.shape[1]
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = torch.sigmoid(gi[:, :hd] + gh[:, :hd])
    z = torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
    n = torch.tanh(gi[:, 2 * hd:] + r * gh[:, 2 * hd:])
    return (1 - z) * n + z * h


def gated_sum(add, mul, pre):
    return add + mul * torch.sigmoid(pre)


# ---- (value, err) pairs in float64 ------------------------------------------------------------------------------------------
def linear_b(x, ex, w, b, act):
    k = x.shape[1]
    y = x @ w.T + b
    e = gamma(k + 1) * (x.abs() @ w.abs().T + b.abs()) + ex @ w.abs().T
    if act == "leakyrelu":
        e = e + U * y.abs()
    elif act == "tanh":
        e = e + TANH_EVAL
    return act_fn(y, act), e * SLACK


def gru_cell_b(x, ex, h, eh, w_ih, w_hh, b_ih, b_hh, mask=None):
    if mask is not None:
        m = mask.bool()[:, None]
        h, eh = torch.where(m, torch.zeros_like(h), h), torch.where(m, torch.zeros_like(eh), eh)
    k, hd = x.shape[1], h.shape[1]
    ax, ah, wi, wh = x.abs(), h.abs(), w_ih.abs(), w_hh.abs()
    s = lambda a: slice(a * hd, (a + 1) * hd)
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    out = {}
    for name, g in (("r", 0), ("z", 1)):
        pre = gi[:, s(g)] + gh[:, s(g)]
        e = gamma(k + hd + 2) * (ax @ wi[s(g)].T + ah @ wh[s(g)].T + b_ih[s(g)].abs() + b_hh[s(g)].abs()) + ex @ wi[s(g)].T + eh @ wh[s(g)].T
        out[name] = (torch.sigmoid(pre), e / 4 + SIG_EVAL)
    (r, er), (z, ez) = out["r"], out["z"]
    a, ea = gi[:, s(2)], gamma(k + 1) * (ax @ wi[s(2)].T + b_ih[s(2)].abs()) + ex @ wi[s(2)].T
    g, eg = gh[:, s(2)], gamma(hd + 1) * (ah @ wh[s(2)].T + b_hh[s(2)].abs()) + eh @ wh[s(2)].T
    n = torch.tanh(a + r * g)
    en = ea + er * g.abs() + r * eg + 3 * U * (a.abs() + (r * g).abs()) + TANH_EVAL
    hn = (1 - z) * n + z * h
    e = ez * (n.abs() + h.abs()) + (1 - z) * en + z * eh + 4 * U * (((1 - z) * n).abs() + (z * h).abs())
    return hn, e * SLACK


def gated_sum_b(add, eadd, mul, emul, pre, epre):
    sg = torch.sigmoid(pre)
    out = add + mul * sg
    e = eadd + emul * sg + mul.abs() * (epre / 4 + SIG_EVAL) + 2 * U * (add.abs() + (mul * sg).abs())
    return out, e * SLACK


# ---- the student ---------------------------------------------------------------------------------------------------------------
def _chain_names(sd, prefix):
    """[(weight, bias, activation-or-None)] of prefix.i.layer.0.* (LeakyReLU Layers) and a bare prefix.i.* (the Tanh head's Linear)"""
    out, i = [], 0
    while True:
        if f"{prefix}.{i}.layer.0.weight" in sd:
            out.append((sd[f"{prefix}.{i}.layer.0.weight"], sd[f"{prefix}.{i}.layer.0.bias"], "leakyrelu"))
        elif f"{prefix}.{i}.weight" in sd:
            out.append((sd[f"{prefix}.{i}.weight"], sd[f"{prefix}.{i}.bias"], "tanh"))
        else:
            return out
        i += 1


def _chain_b(x, ex, layers):
    for w, b, act in layers:
        x, ex = linear_b(x, ex, w, b, act)
    return x, ex


def student_step_b(sd, info, obs, h, eh, reset=None):
    """One time step with bounds.  sd: parameters in float64 under the reference's names; obs [E, F] float64 (exact);
    h, eh: lists per GRU layer -> (actions, e_actions, estimated, e_estimated, h', e_h')."""
    p, ns, nd = info["proprioceptive"], info["sparse"], info["dense"]
    f = obs.shape[1]
    zero = lambda t: torch.zeros_like(t)
    prop, sparse, dense = obs[:, :p], obs[:, f - ns - nd:f - nd], obs[:, f - nd:]
    e1, ee1 = _chain_b(sparse, zero(sparse), _chain_names(sd, "encoder1.encoder"))
    e2, ee2 = _chain_b(dense, zero(dense), _chain_names(sd, "encoder2.encoder"))
    l_e, el_e = torch.cat((e1, e2), 1), torch.cat((ee1, ee2), 1)
    x, ex = torch.cat((prop, l_e), 1), torch.cat((zero(prop), el_e), 1)
    hn, ehn = [], []
    for l in range(len(h)):
        g = [sd[f"belief_encoder.gru.{nm}_l{l}"] for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        x, ex = gru_cell_b(x, ex, h[l], eh[l], *g, mask=reset)
        hn.append(x)
        ehn.append(ex)
    xb, exb = _chain_b(x, ex, _chain_names(sd, "belief_encoder.gb"))
    xa, exa = _chain_b(x, ex, _chain_names(sd, "belief_encoder.ga"))
    belief, ebel = gated_sum_b(xb, exb, l_e, el_e, xa, exa)
    act, eact = _chain_b(torch.cat((prop, belief), 1), torch.cat((zero(prop), ebel), 1), _chain_names(sd, "MLP.network"))
    last, elast = x[-1:], ex[-1:]                                    # the decoder reads the last batch row's GRU output
    gate, egate = _chain_b(last, elast, _chain_names(sd, "belief_decoder.gate_encoder"))
    dec, edec = _chain_b(last, elast, _chain_names(sd, "belief_decoder.decoder"))
    ext = torch.cat((sparse, dense), 1)
    est, eest = gated_sum_b(dec.expand_as(ext), edec.expand_as(ext), ext, zero(ext), gate.expand_as(ext), egate.expand_as(ext))
    return act, eact, est, eest, hn, ehn


def student_forward_b(sd, info, x, h0):
    """Student.forward with bounds: x [B, T, F], h0 [L, B, H] -> (actions, estimated, h) each as (value, err)."""
    sd = {k: f64(v) for k, v in sd.items()}
    x, h0 = f64(x), f64(h0)
    h, eh = list(h0), [torch.zeros_like(t) for t in h0]
    acts, eacts, ests, eests = [], [], [], []
    for t in range(x.shape[1]):
        a, ea, s, es, h, eh = student_step_b(sd, info, x[:, t], h, eh)
        acts.append(a); eacts.append(ea); ests.append(s); eests.append(es)
    st = lambda ts: torch.stack(ts, 1)
    return (st(acts), st(eacts)), (st(ests), st(eests)), (torch.stack(h), torch.stack(eh))


MUTATIONS = ("ga_without_leakyrelu", "mlp_without_proprioception", "branches_from_gru_layer_0", "decoder_per_row")


def student_step_f32(sd, info, obs, h, reset=None, mutate=None):
    """The same step evaluated by torch in float32 on the CPU (the yardstick): -> (actions, estimated, h').
    ``mutate``: one of MUTATIONS — a deliberately WRONG student, for showing that a check rejects it."""
    assert mutate is None or mutate in MUTATIONS, mutate
    p, ns, nd = info["proprioceptive"], info["sparse"], info["dense"]
    f = obs.shape[1]

    def run(v, layers):
        for w, b, a in layers:
            v = linear(v, w, b, a)
        return v

    prop, sparse, dense = obs[:, :p], obs[:, f - ns - nd:f - nd], obs[:, f - nd:]
    l_e = torch.cat((run(sparse, _chain_names(sd, "encoder1.encoder")), run(dense, _chain_names(sd, "encoder2.encoder"))), 1)
    x, hn = torch.cat((prop, l_e), 1), []
    for l in range(len(h)):
        x = gru_cell(x, h[l], *[sd[f"belief_encoder.gru.{nm}_l{l}"] for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")], mask=reset)
        hn.append(x)
    top = hn[0] if mutate == "branches_from_gru_layer_0" else x
    ga = _chain_names(sd, "belief_encoder.ga")
    if mutate == "ga_without_leakyrelu":
        ga = ga[:-1] + [(ga[-1][0], ga[-1][1], None)]
    belief = gated_sum(run(top, _chain_names(sd, "belief_encoder.gb")), l_e, run(top, ga))
    act = run(torch.cat((torch.zeros_like(prop) if mutate == "mlp_without_proprioception" else prop, belief), 1), _chain_names(sd, "MLP.network"))
    last = x if mutate == "decoder_per_row" else x[-1:]
    est = gated_sum(run(last, _chain_names(sd, "belief_decoder.decoder")), torch.cat((sparse, dense), 1),
                    run(last, _chain_names(sd, "belief_decoder.gate_encoder")))
    return act, est, hn


# ---- the sharp check on composed outputs -------------------------------------------------------------------------------------------
# Carried through a dozen matrix products the worst-case bound above is orders of magnitude above any f32 evaluation's error (it
# assumes every rounding aligned), so on actions and estimated it is kept as the honesty condition only.  What bites is the
# reference's own error: ``yard`` is an f32 evaluation of the SAME expression on the SAME inputs (torch on the CPU, or the reference's
# recorded f32 outputs), gap = max |yard - float64| over the tensor.  The kernels are another f32 evaluation of that expression that
# differs in summation order and in expf / tanhf by an ulp: its error is a draw of the same size.  YARD_FACTOR = 16 is the room given
# to the maximum of a different draw (and to fused chains that round in another order); a wrong student is off by 1e-4 and more,
# four orders above a gap of about 1e-8 (test_student_host.py shows the four MUTATIONS rejected).
YARD_FACTOR = 16.0


def yard_gap(yard, want):
    return float((f64(yard) - want).abs().max())


def inside_yardstick(got, want, yard):
    """max |got - float64| <= YARD_FACTOR * max |f32 yardstick - float64| -> (ok, max |d|, gap)"""
    d, gap = float((f64(got) - want).abs().max()), yard_gap(yard, want)
    return d <= YARD_FACTOR * gap, d, gap


# ---- shared test data ------------------------------------------------------------------------------------------------------------
# gru_cell cases (M, K, H): rows {1, 31, 32, 33, 65} x hidden {1, 31, 32, 33, 44, 300} x input {0, 1, 3, 124, 125} as a covering subset
# (every value of each axis appears; (65, 125, 300) and (1, 1, 1) are required), then both sides of the route's switch point
# ceil(M / 128) ceil(H / 32) >= 512: at H = 300 (10 tiles) that is M = 6 528 | 6 529, at H = 32 (1 tile) M = 65 408 | 65 409.
CELL_CASES = [(1, 1, 1), (65, 125, 300), (31, 0, 31), (32, 3, 32), (33, 124, 33), (65, 1, 44), (1, 125, 300), (33, 0, 1), (32, 124, 44),
              (31, 3, 300), (6528, 3, 300), (6529, 3, 300), (65408, 1, 32), (65409, 1, 32)]
GATED_CASES = [(1, 1), (33, 120), (5, 37)]


def cell_data(m, k, hd, seed=0):
    """Seeded f32 inputs of one cell case, nn.GRU-like scales: weights uniform +-1/sqrt(H) (at least +-0.5), x and h in (-1, 1)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * m + 31 * k + hd)
    b = max(0.5, 1.0 / np.sqrt(hd)) if hd < 4 else 1.0 / np.sqrt(hd)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    return dict(x=r(m, k), h=r(m, hd), w_ih=r(3 * hd, k) * b, w_hh=r(3 * hd, hd) * b, b_ih=r(3 * hd) * b, b_hh=r(3 * hd) * b)


def random_state_dict(shapes, seed=0):
    """f32 parameters for name -> shape at nn.Linear / nn.GRU scales: uniform +-1/sqrt(fan_in) (nn.GRU: 1/sqrt(H)); log_std zeros."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in shapes.items():
        if name.endswith("log_std_parameter"):
            sd[name] = torch.zeros(*shape)
            continue
        if ".gru." in name:
            fan = shape[0] // 3
        else:
            fan = shape[1] if len(shape) == 2 else shapes[name[:-len("bias")] + "weight"][1]
        sd[name] = ((torch.rand(*shape, generator=g) * 2 - 1) / np.sqrt(max(fan, 1))).contiguous()
    return sd
