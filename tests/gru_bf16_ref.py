"""Reference for the bf16 GRU cell, the bf16 Layer and StudentPolicy(precision="bf16") (csrc/rover_bf16_tile.hip; the arithmetic is
stated in include/rover_step.h at rover_gru_cell_bf16).  No project code: student_ref.py's float64 cell and bound, bf16_ref.rd.

The arithmetic under test: x, h, w_ih, w_hh rounded to bf16 as they are read FOR THE PRODUCTS; products exact, summed in f32; the f32
cell's epilogue in f32, whose blend z * h takes the UNROUNDED h.

Two kinds of data, as in bf16_ref.py:

  * LATTICE cells.  x, h, the biases and the weights are dyadic rationals chosen so that every product of rounded operands, every partial
    sum in any order and both bias additions are exact in f32 (lattice_cell asserts it: every term is a multiple of a quantum q and the
    sum of magnitudes stays below 2^24 q).  The four pre-activations of the kernel then EQUAL the float64 ones, and what is left of
    student_ref.gru_cell_b's bound is SIG_EVAL, TANH_EVAL and the epilogue's roundings — about 2e-6 — against bf16 effects of 2^-9:
      family "a": x = n 2^-10 (|x| <= 2), h = n 2^-10 (|h| <= 1), biases n 2^-10 (|b| <= 0.5), weights +-0.25, 8 non-zeros per row;
      family "b": weights +-n 2^-11 with n in [256, 1024] (bf16 cannot represent most of them), 4 non-zeros per row, |x| <= 1.
    lattice_cell asserts that some x, some h and (family "b") some weights are NOT representable: a kernel that truncated, did not
    round, or blended with the rounded h would otherwise pass.
  * REAL-valued cells (student_ref.cell_data): cell_bound() is gru_cell_b on the rounded operands with zero input error — a sum of
    exact products errs by gamma_n sum |a||w| as in the f32 case — with the blend on the unrounded h.

emulate_cell() evaluates the same arithmetic in f32 torch on the CPU in two summation orders, and with the four MUTANTS that the
lattice bound must reject; student_step_emulated() is the whole student in that arithmetic (the yardstick of the distance to float64).
"""
import numpy as np
import torch

import student_ref as sr
from bf16_ref import rd, representable

MUTANTS = ("truncate", "blend_rounded_h", "no_rounding", "n_without_r")

# (M, K, H) of the GPU suite: M in {1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257}, K in {0, 1, 31, 32, 33, 124, 300}, H in {1, 15, 16, 17,
# 31, 32, 33, 44, 300} and the tile's own edges (128 rows: 127 / 129 are in the list; 64 columns: 63, 64, 65 added), every value of each
# axis at least once; (129, 124, 300) and (33, 300, 300) are required.
LATTICE_CASES = [(1, 0, 1), (15, 1, 15), (16, 31, 16), (17, 32, 17), (31, 33, 31), (32, 124, 32), (33, 300, 33), (127, 0, 44), (128, 1, 300),
                 (129, 124, 300), (257, 31, 63), (33, 300, 300), (1, 32, 64), (15, 33, 65), (16, 124, 1), (17, 300, 15), (31, 0, 16),
                 (32, 1, 17), (127, 31, 31), (128, 32, 32), (257, 33, 33), (129, 300, 44), (1, 124, 63), (257, 0, 65), (128, 33, 64)]
FAMILIES = ("a", "b")


def _sparse_rows(rows, cols, nnz, values, g):
    """[rows, cols] float64 with min(nnz, cols) non-zeros per row, drawn by values(count)."""
    w = torch.zeros(rows, cols, dtype=torch.float64)
    n = min(nnz, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:n]
        w[r, idx] = values(n)
    return w


def lattice_cell(m, k, hd, family, seed=0):
    """-> dict(x, h, w_ih, w_hh, b_ih, b_hh) of f32 CPU tensors, and ``counts`` = non-representable elements of (x, h, weights).
    Asserts the exactness conditions of the module docstring."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(7919 * seed + 131 * m + 17 * k + hd + (0 if family == "a" else 10 ** 6))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    sign = lambda *s: ri(0, 1, *s) * 2 - 1
    q10 = 2.0 ** -10
    xmax = 2048 if family == "a" else 1024
    x, h = ri(-xmax, xmax, m, k) * q10, ri(-1024, 1024, m, hd) * q10
    b_ih, b_hh = ri(-512, 512, 3 * hd) * q10, ri(-512, 512, 3 * hd) * q10
    if family == "a":
        qw, nnz, val = 0.25, 8, lambda n: sign(n) * 0.25
    else:
        qw, nnz, val = 2.0 ** -11, 4, lambda n: sign(n) * ri(256, 1024, n) * 2.0 ** -11
    w_ih, w_hh = _sparse_rows(3 * hd, k, nnz, val, g), _sparse_rows(3 * hd, hd, nnz, val, g)
    # exactness: rounded operands are multiples of their quanta (rounding a multiple of q to fewer bits gives a multiple of q), so every
    # product is a multiple of q = q10 * qw and so is every bias; sums of magnitudes below 2^24 q are exact in f32 in any order
    q = q10 * qw
    xr, hr, wir, whr = rd(x), rd(h), rd(w_ih), rd(w_hh)
    for t, qt in ((xr, q10), (hr, q10), (wir, qw), (whr, qw), (b_ih, q10), (b_hh, q10)):
        assert bool((torch.round(t / qt) * qt == t).all()), "an operand is not on its lattice"
        assert bool((t.float().double() == t).all())
    mag = xr.abs() @ wir.abs().T + hr.abs() @ whr.abs().T + b_ih.abs() + b_hh.abs()
    assert float(mag.max()) < 2.0 ** 24 * q, f"a partial sum may reach {float(mag.max()):.3g} >= 2^24 q"
    counts = (int((~representable(x)).sum()), int((~representable(h)).sum()), int((~representable(w_ih)).sum()) + int((~representable(w_hh)).sum()))
    if m * k >= 8:
        assert counts[0] > 0, "every x is bf16-representable"
    if m * hd >= 8:
        assert counts[1] > 0, "every h is bf16-representable"
    if family == "b" and hd * (k + hd) >= 8:
        assert counts[2] > 0, "every weight is bf16-representable"
    f32 = lambda t: t.float().contiguous()
    return dict(x=f32(x), h=f32(h), w_ih=f32(w_ih), w_hh=f32(w_hh), b_ih=f32(b_ih), b_hh=f32(b_hh)), counts


def cell_bound(d, mask=None, exact_sums=False, rounding=rd):
    """-> (h' float64, err): the bf16 cell on the f32 data ``d`` and the bound the kernel is held to.  student_ref.gru_cell_b's
    expressions with the products' operands rounded, zero input error and the blend on the unrounded h; ``exact_sums`` (lattice data)
    removes the summation terms: SIG_EVAL, TANH_EVAL and the epilogue's roundings remain."""
    x, h, w_ih, w_hh, b_ih, b_hh = (sr.f64(d[n]) for n in ("x", "h", "w_ih", "w_hh", "b_ih", "b_hh"))
    if mask is not None:
        h = torch.where(mask.bool()[:, None], torch.zeros_like(h), h)
    k, hd = x.shape[1], h.shape[1]
    xr, hr, wi, wh = rounding(x), rounding(h), rounding(w_ih), rounding(w_hh)
    ax, ah, awi, awh = xr.abs(), hr.abs(), wi.abs(), wh.abs()
    s = lambda a: slice(a * hd, (a + 1) * hd)
    gam = (lambda n: 0.0) if exact_sums else sr.gamma
    gi, gh = xr @ wi.T + b_ih, hr @ wh.T + b_hh
    out = {}
    for name, g in (("r", 0), ("z", 1)):
        e = gam(k + hd + 2) * (ax @ awi[s(g)].T + ah @ awh[s(g)].T + b_ih[s(g)].abs() + b_hh[s(g)].abs())
        out[name] = (torch.sigmoid(gi[:, s(g)] + gh[:, s(g)]), e / 4 + sr.SIG_EVAL)
    (r, er), (z, ez) = out["r"], out["z"]
    a, ea = gi[:, s(2)], gam(k + 1) * (ax @ awi[s(2)].T + b_ih[s(2)].abs())
    g, eg = gh[:, s(2)], gam(hd + 1) * (ah @ awh[s(2)].T + b_hh[s(2)].abs())
    n = torch.tanh(a + r * g)
    en = ea + er * g.abs() + r * eg + 3 * sr.U * (a.abs() + (r * g).abs()) + sr.TANH_EVAL
    hn = (1 - z) * n + z * h                                         # the UNROUNDED h
    e = ez * (n.abs() + h.abs()) + (1 - z) * en + 4 * sr.U * (((1 - z) * n).abs() + (z * h).abs())
    return hn, e * sr.SLACK


def _r32(t, truncate=False):
    return rd(t.double(), truncate).float()


def emulate_cell(d, mask=None, reverse=False, mutant=None):
    """The kernel's arithmetic in f32 torch on the CPU: rounded operands, f32 sums over k forward or in ``reverse`` order, the f32
    epilogue.  ``mutant``: one of MUTANTS — a deliberately WRONG cell."""
    assert mutant is None or mutant in MUTANTS, mutant
    x, h, w_ih, w_hh, b_ih, b_hh = (d[n].float() for n in ("x", "h", "w_ih", "w_hh", "b_ih", "b_hh"))
    if mask is not None:
        h = torch.where(mask.bool()[:, None], torch.zeros_like(h), h)
    rnd = (lambda t: t) if mutant == "no_rounding" else (lambda t: _r32(t, truncate=mutant == "truncate"))
    xr, hr, wi, wh = rnd(x), rnd(h), rnd(w_ih), rnd(w_hh)
    mm = (lambda a, w: a.flip(1) @ w.flip(1).T) if reverse else (lambda a, w: a @ w.T)
    hd = h.shape[1]
    s = lambda a: slice(a * hd, (a + 1) * hd)
    gi, gh = mm(xr, wi), mm(hr, wh)
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    r = sig(((gi[:, s(0)] + gh[:, s(0)]) + b_ih[s(0)]) + b_hh[s(0)])
    z = sig(((gi[:, s(1)] + gh[:, s(1)]) + b_ih[s(1)]) + b_hh[s(1)])
    q = gh[:, s(2)] + b_hh[s(2)]
    n = torch.tanh((gi[:, s(2)] + b_ih[s(2)]) + (q if mutant == "n_without_r" else r * q))
    hb = hr if mutant == "blend_rounded_h" else h
    return (1.0 - z) * n + z * hb


# ---- the whole student in the kernels' arithmetic (f32 torch, rd at every operand read) --------------------------------------------
def _linear_emulated(x, w, b, act):
    return sr.act_fn(_r32(x) @ _r32(w).T + b, act)


def student_step_emulated(sd, info, obs, h, reset=None):
    """student_ref.student_step_f32 with every matrix product on rounded operands: -> (actions, estimated, h')."""
    p, ns, nd = info["proprioceptive"], info["sparse"], info["dense"]
    f = obs.shape[1]

    def run(v, layers):
        for w, b, a in layers:
            v = _linear_emulated(v, w, b, a)
        return v

    prop, sparse, dense = obs[:, :p], obs[:, f - ns - nd:f - nd], obs[:, f - nd:]
    l_e = torch.cat((run(sparse, sr._chain_names(sd, "encoder1.encoder")), run(dense, sr._chain_names(sd, "encoder2.encoder"))), 1)
    x, hn = torch.cat((prop, l_e), 1), []
    for l in range(len(h)):
        names = [f"belief_encoder.gru.{nm}_l{l}" for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        x = emulate_cell(dict(x=x, h=h[l], w_ih=sd[names[0]], w_hh=sd[names[1]], b_ih=sd[names[2]], b_hh=sd[names[3]]), mask=reset)
        hn.append(x)
    belief = sr.gated_sum(run(x, sr._chain_names(sd, "belief_encoder.gb")), l_e, run(x, sr._chain_names(sd, "belief_encoder.ga")))
    act = run(torch.cat((prop, belief), 1), sr._chain_names(sd, "MLP.network"))
    last = x[-1:]
    est = sr.gated_sum(run(last, sr._chain_names(sd, "belief_decoder.decoder")), torch.cat((sparse, dense), 1),
                       run(last, sr._chain_names(sd, "belief_decoder.gate_encoder")))
    return act, est, hn


F64_MARGIN = 4.0          # max |GPU - float64| <= 4 x max |emulation - float64|: both carry the same bf16 rounding noise; the factor allows
#                           for hidden values near a rounding tie that fall to the other side under the device's summation order
