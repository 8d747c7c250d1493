"""The student's training path on the GPU: rover_gru_cell_train, rover_gru_cell_backward, rover_linear_dgrad, rover_gated_sum_backward,
StudentPolicy.forward_train / backward and StudentTrainer.update against float64 (tests/student_grad_ref.py states the rule)."""
import functools

import pytest
import torch

import student_grad_ref as gr
import student_ref as sr
from test_distill_host import BWD_SHAPES, RECON, default_case, fixture_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    yield e
    e.close()


def dev(d):
    return {k: (None if v is None else v.to(DEV)) for k, v in d.items()}


# ---- gru_cell_train ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,hd", sr.CELL_CASES)
def test_gru_cell_train_has_the_cells_bits_and_stores_the_gates(eng, m, k, hd):
    d = sr.cell_data(m, k, hd)
    g = dev(d)
    mask = (torch.arange(m) % 4 == 1) if m > 1 else None
    for msk in (None, mask):
        mk = None if msk is None else msk.to(DEV)
        plain, out = torch.full_like(g["h"], float("nan")), torch.full_like(g["h"], float("nan"))
        gates = torch.full((m, 4 * hd + 3), 3.25, device=DEV)
        eng.gru_cell(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], plain, reset_mask=mk)
        eng.gru_cell_train(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], out, gates[:, :4 * hd], reset_mask=mk)
        assert torch.equal(out, plain)
        assert bool((gates[:, 4 * hd:] == 3.25).all())
        # r, z, n inside the cell's own bound: n is h' with z = 0, r and z are bounded like the sigmoids inside gru_cell_b
        x, h = sr.f64(d["x"]), sr.f64(d["h"])
        if msk is not None:
            h = torch.where(msk[:, None], torch.zeros_like(h), h)
        w_ih, w_hh, b_ih, b_hh = (sr.f64(d[n]) for n in ("w_ih", "w_hh", "b_ih", "b_hh"))
        gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
        s = lambda a: slice(a * hd, (a + 1) * hd)
        mag = lambda a: x.abs() @ w_ih[s(a)].abs().T + h.abs() @ w_hh[s(a)].abs().T + b_ih[s(a)].abs() + b_hh[s(a)].abs()
        got = sr.f64(gates[:, :4 * hd])
        e_sig = {}
        for a, name in ((0, "r"), (1, "z")):
            want = torch.sigmoid(gi[:, s(a)] + gh[:, s(a)])
            e_sig[name] = (sr.gamma(k + hd + 2) * mag(a) / 4 + sr.SIG_EVAL) * sr.SLACK
            assert bool(((got[:, s(a)] - want).abs() <= e_sig[name]).all()), name
        r = torch.sigmoid(gi[:, s(0)] + gh[:, s(0)])
        q = gh[:, s(2)]
        e_q = sr.gamma(hd + 1) * (h.abs() @ w_hh[s(2)].abs().T + b_hh[s(2)].abs()) * sr.SLACK
        assert bool(((got[:, s(3)] - q).abs() <= e_q).all())
        e_a = sr.gamma(k + 1) * (x.abs() @ w_ih[s(2)].abs().T + b_ih[s(2)].abs())
        e_n = (e_a + e_sig["r"] * q.abs() + r * e_q + 3 * sr.U * (gi[:, s(2)].abs() + (r * q).abs()) + sr.TANH_EVAL) * sr.SLACK
        assert bool(((got[:, s(2)] - torch.tanh(gi[:, s(2)] + r * q)).abs() <= e_n).all())


def test_gru_cell_train_refuses_overlapping_gates(eng):
    from isaac_rover_amd._lib import RoverError
    m, k, hd = 33, 3, 44
    g = dev(sr.cell_data(m, k, hd, seed=3))
    buf = torch.zeros(m, 5 * hd, device=DEV)
    with pytest.raises(RoverError, match="gates overlaps h_out"):
        eng.gru_cell_train(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], buf[:, :hd], buf[:, :4 * hd])
    with pytest.raises(RoverError):
        eng.gru_cell_train(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], torch.empty(m, hd, device=DEV), buf[:, :4 * hd - 1])
    torch.cuda.synchronize()
    assert not buf.any()


# ---- gru_cell_backward -------------------------------------------------------------------------------------------------------------------
def bwd_data(m, hd, seed=0):
    g = torch.Generator().manual_seed(977 * seed + 13 * m + hd)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    u = lambda *s: torch.rand(*s, generator=g)
    gates = torch.cat((u(m, hd), u(m, hd), r(m, hd), r(m, hd)), 1)                 # r, z in (0, 1); n, q in (-1, 1)
    return dict(dh_above=r(m, hd), dh_next=r(m, hd), gates=gates, h_in=r(m, hd), w_hh=r(3 * hd, hd) * max(0.5 if hd < 4 else 0.0, 1.0 / hd ** 0.5))


def bwd_formulas(d, mask, with_next):
    """rover_gru_cell_backward's formulas in the dtype of ``d`` -> (dgi, dgh, dh_in)"""
    hd = d["h_in"].shape[1]
    gt = d["gates"]
    r, z, n, q = gt[:, :hd], gt[:, hd:2 * hd], gt[:, 2 * hd:3 * hd], gt[:, 3 * hd:]
    h = d["h_in"] if mask is None else torch.where(mask[:, None], torch.zeros_like(d["h_in"]), d["h_in"])
    g = d["dh_above"] + d["dh_next"] if with_next else d["dh_above"]
    a_n = (g * (1 - z)) * (1 - n * n)
    a_z = (g * (h - n)) * (z * (1 - z))
    a_r = (a_n * q) * (r * (1 - r))
    dgi, dgh = torch.cat((a_r, a_z, a_n), 1), torch.cat((a_r, a_z, a_n * r), 1)
    dh_in = dgh @ d["w_hh"] + g * z
    if mask is not None:
        dh_in = torch.where(mask[:, None], torch.zeros_like(dh_in), dh_in)
    return dgi, dgh, dh_in


def run_bwd(eng, g, mask, with_next, outs=None):
    m, hd = g["h_in"].shape
    dgi, dgh, dh_in = outs or (torch.full((m, 3 * hd), float("nan"), device=DEV), torch.full((m, 3 * hd), float("nan"), device=DEV),
                               torch.full((m, hd), float("nan"), device=DEV))
    eng.gru_cell_backward(g["dh_above"], g["dh_next"] if with_next else None, g["gates"], g["h_in"], g["w_hh"], dgi, dgh, dh_in,
                          reset_mask=None if mask is None else mask.to(DEV))
    return dgi, dgh, dh_in


@pytest.mark.parametrize("m,hd", BWD_SHAPES)
def test_gru_cell_backward_against_float64(eng, m, hd):
    d = bwd_data(m, hd)
    g, d64 = dev(d), {k: sr.f64(v) for k, v in d.items()}
    mask = torch.arange(m) % 3 == 0
    for msk in (None, mask):
        for with_next in (False, True):
            got = run_bwd(eng, g, msk, with_next)
            want, yard = bwd_formulas(d64, msk, with_next), bwd_formulas(d, msk, with_next)
            for name, a, b, c in zip(("dgi", "dgh", "dh_in"), got, want, yard):
                ok, dd, gap, allowed = gr.verdict(a, b, c)
                print(f"gru_cell_backward ({m},{hd}) {eng.gru_cell_backward_route(m, hd)} mask {msk is not None} next {with_next} {name}: "
                      f"max |d| {dd:.3e} gap {gap:.3e} allowed {allowed:.3e}")
                assert torch.isfinite(a).all() and ok, (name, msk is not None, with_next)
            if msk is not None:
                assert not got[2][msk.to(DEV)].any()                 # a reset row's dh_in is exactly 0


def test_gru_cell_backward_strides_permutation_determinism(eng):
    m, hd = 65, 44
    d = bwd_data(m, hd, seed=1)
    g = dev(d)
    mask = torch.arange(m) % 4 == 1
    dense = run_bwd(eng, g, mask, True)
    pad = lambda t, extra: torch.cat((torch.randn(t.shape[0], 3), t, torch.randn(t.shape[0], extra)), 1).to(DEV)[:, 3:3 + t.shape[1]]
    gs = dict(g, dh_above=pad(d["dh_above"], 2), dh_next=pad(d["dh_next"], 5), gates=pad(d["gates"], 1), h_in=pad(d["h_in"], 4))
    wide = [torch.full((m, 3 * hd + 6), 3.25, device=DEV), torch.full((m, 3 * hd + 2), 3.25, device=DEV), torch.full((m, hd + 7), 3.25, device=DEV)]
    run_bwd(eng, gs, mask, True, outs=(wide[0][:, :3 * hd], wide[1][:, 1:1 + 3 * hd], wide[2][:, 2:2 + hd]))
    assert torch.equal(wide[0][:, :3 * hd], dense[0]) and torch.equal(wide[1][:, 1:1 + 3 * hd], dense[1]) and torch.equal(wide[2][:, 2:2 + hd], dense[2])
    assert bool((wide[0][:, 3 * hd:] == 3.25).all()) and bool((wide[1][:, :1] == 3.25).all()) and bool((wide[1][:, 1 + 3 * hd:] == 3.25).all())
    assert bool((wide[2][:, :2] == 3.25).all()) and bool((wide[2][:, 2 + hd:] == 3.25).all())
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(5))
    gp = dict(g, **{k: g[k][perm.to(DEV)].contiguous() for k in ("dh_above", "dh_next", "gates", "h_in")})
    for a, b in zip(run_bwd(eng, gp, mask[perm], True), dense):
        assert torch.equal(a, b[perm.to(DEV)])                        # a row's result does not depend on where the row is
    for a, b in zip(run_bwd(eng, g, mask, True), dense):
        assert torch.equal(a, b)                                     # two runs, the same bits


def test_gru_cell_backward_refuses_overlap_and_bad_arguments(eng):
    from isaac_rover_amd._lib import RoverError
    m, hd = 33, 44
    g = dev(bwd_data(m, hd, seed=2))
    snap = {k: v.clone() for k, v in g.items()}
    dgi, dgh, dh_in = (torch.full((m, n), 3.25, device=DEV) for n in (3 * hd, 3 * hd, hd))
    with pytest.raises(RoverError, match="dh_in overlaps dh_next"):
        eng.gru_cell_backward(g["dh_above"], g["dh_next"], g["gates"], g["h_in"], g["w_hh"], dgi, dgh, g["dh_next"])
    with pytest.raises(RoverError, match="dgi overlaps gates"):
        eng.gru_cell_backward(g["dh_above"], g["dh_next"], g["gates"], g["h_in"], g["w_hh"], g["gates"][:, :3 * hd], dgh, dh_in)
    with pytest.raises(RoverError, match="dgh overlaps dgi"):
        eng.gru_cell_backward(g["dh_above"], g["dh_next"], g["gates"], g["h_in"], g["w_hh"], dgi, dgi, dh_in)
    with pytest.raises(RoverError, match="dh_in overlaps dgh"):
        eng.gru_cell_backward(g["dh_above"], g["dh_next"], g["gates"], g["h_in"], g["w_hh"], dgi, dgh, dgh[:, :hd])
    with pytest.raises(RoverError):
        eng.gru_cell_backward(g["dh_above"], g["dh_next"], g["gates"][:, :-1], g["h_in"], g["w_hh"], dgi, dgh, dh_in)
    with pytest.raises(RoverError):
        eng.gru_cell_backward(g["dh_above"], g["dh_next"], g["gates"], g["h_in"], g["w_hh"][:-1].contiguous(), dgi, dgh, dh_in)
    with pytest.raises(RoverError):
        eng.gru_cell_backward(g["dh_above"].double(), g["dh_next"], g["gates"], g["h_in"], g["w_hh"], dgi, dgh, dh_in)
    torch.cuda.synchronize()
    assert all(torch.equal(g[k], snap[k]) for k in g)                # nothing was written
    assert bool((dgi == 3.25).all()) and bool((dgh == 3.25).all()) and bool((dh_in == 3.25).all())
    e = lambda n: torch.empty(0, n, device=DEV)                       # M = 0: a no-op
    eng.gru_cell_backward(e(hd), None, e(4 * hd), e(hd), g["w_hh"], e(3 * hd), e(3 * hd), e(hd))


# ---- linear_dgrad ------------------------------------------------------------------------------------------------------------------------
NS, KS, MS = (1, 33, 257, 900), (1, 32, 33, 257, 300, 512), (1, 33, 65)
DGRAD_CASES = [(MS[(i + j) % 3], n, k, ("none", "leakyrelu")[(i + j) % 2]) for i, n in enumerate(NS) for j, k in enumerate(KS)]
DGRAD_CASES += [(MS[(i + j + 1) % 3], n, k, ("leakyrelu", "none")[(i + j) % 2]) for i, n in enumerate(NS) for j, k in enumerate(KS) if (n, k) in
                ((900, 300), (257, 257), (1, 1), (33, 512), (900, 512))]
# both sides of the route's switch points: rows 65 535 | 65 536, and at 65 536 rows K = 32 | 33
DGRAD_CASES += [(65535, 33, 33, "leakyrelu"), (65536, 33, 32, "none"), (65536, 33, 33, "leakyrelu"), (65536, 257, 300, "none")]


@pytest.mark.parametrize("m,n,k,act", DGRAD_CASES)
def test_linear_dgrad_against_float64(eng, m, n, k, act):
    g = torch.Generator().manual_seed(m * 7 + n * 131 + k)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    w, dyw, yw = r(n, k) / max(n, 1) ** 0.5, r(m, n + 3), r(m, n + 1)
    dy, y = dyw[:, :n], yw[:, 1:]                                    # column slices of wider rows, on the device too
    dx = torch.full((m, k + 5), 3.25, device=DEV)
    eng.linear_dgrad(yw.to(DEV)[:, 1:] if act != "none" else None, dyw.to(DEV)[:, :n], w.to(DEV), act, dx[:, 2:2 + k])
    dz = sr.f64(dy) * (torch.where(sr.f64(y) > 0, 1.0, 0.01) if act == "leakyrelu" else 1.0)
    want, bound = dz @ sr.f64(w), sr.gamma(n + 2) * (dz.abs() @ sr.f64(w).abs())
    got = sr.f64(dx[:, 2:2 + k])
    diff = (got - want).abs()
    print(f"linear_dgrad ({m},{k},{n}) {act} {eng.linear_dgrad_route(m, k, n)}: max |d| {float(diff.max()):.3e}, worst d / bound "
          f"{float((diff / bound.clamp_min(1e-300)).max()):.4f}")
    assert torch.isfinite(got).all() and bool((diff <= bound).all())
    assert bool((dx[:, :2] == 3.25).all()) and bool((dx[:, 2 + k:] == 3.25).all())


def test_linear_dgrad_refusals(eng):
    from isaac_rover_amd._lib import RoverError
    m, n, k = 33, 40, 300
    w, dy, dx = torch.zeros(n, k, device=DEV), torch.zeros(m, n, device=DEV), torch.full((m, k), 3.25, device=DEV)
    with pytest.raises(RoverError):
        eng.linear_dgrad(None, dy, w, "leakyrelu", dx)               # an activation needs y
    with pytest.raises(RoverError):
        eng.linear_dgrad(None, dy[:, :-1], w, None, dx)
    both = torch.full((m, n + k), 3.25, device=DEV)
    with pytest.raises(RoverError, match="dx overlaps"):
        eng.linear_dgrad(None, both[:, :n], w, None, both[:, n:])
    torch.cuda.synchronize()
    assert bool((dx == 3.25).all()) and bool((both == 3.25).all())
    eng.linear_dgrad(None, torch.empty(0, n, device=DEV), w, None, torch.empty(0, k, device=DEV))


# ---- gated_sum_backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", sr.GATED_CASES)
def test_gated_sum_backward_against_float64(eng, m, n):
    g = torch.Generator().manual_seed(m * 137 + n)
    pad = 0 if (m, n) != (5, 37) else 6
    d_out, mul, pre = (torch.rand(m, n + pad, generator=g) * 2 - 1 for _ in range(3))
    pre = pre * 8
    pre[0, 0], pre[-1, n - 1] = 100.0, -100.0
    a, b, c = (t.to(DEV)[:, :n] for t in (d_out, mul, pre))

    def check(mul_t, pre_t, bm, cm):
        d_mul, d_pre = torch.full((m, n + 2), 3.25, device=DEV), torch.full((m, n + 1), 3.25, device=DEV)
        eng.gated_sum_backward(a, bm, cm, d_mul=d_mul[:, :n], d_pre=d_pre[:, 1:])
        d, mu, s = sr.f64(d_out[:, :n]), sr.f64(mul_t), torch.sigmoid(sr.f64(pre_t))
        # s off by SIG_EVAL; s (1 - s): that once more through each factor, and two roundings; then one product each
        e_mul = (d.abs() * sr.SIG_EVAL + sr.U * (d * s).abs()) * sr.SLACK
        e_pre = ((d * mu).abs() * (sr.SIG_EVAL + 4 * sr.U * s * (1 - s))) * sr.SLACK
        gm, gp = sr.f64(d_mul[:, :n]), sr.f64(d_pre[:, 1:])
        assert torch.isfinite(gm).all() and torch.isfinite(gp).all()
        assert bool(((gm - d * s).abs() <= e_mul).all()) and bool(((gp - (d * mu) * (s * (1 - s))).abs() <= e_pre).all())
        assert bool((d_mul[:, n:] == 3.25).all()) and bool((d_pre[:, :1] == 3.25).all())
        return d_mul[:, :n].clone(), d_pre[:, 1:].clone()

    gm, gp = check(mul[:, :n], pre[:, :n], b, c)
    assert float(gp[-1, n - 1]) == 0.0 and float(gm[-1, n - 1]) == 0.0                     # pre = -100: sigmoid 0
    if (m, n) != (1, 1):
        assert float(gp[0, 0]) == 0.0 and float(gm[0, 0]) == float(d_out[0, 0])         # pre = +100: sigmoid 1
    # one row of mul / pre for every row (row stride 0); the outputs stay per row
    check(mul[:1, :n].expand(m, n), pre[:1, :n].expand(m, n), b[:1].expand(m, n), c[:1].expand(m, n))
    # each output alone has the bits of the pair
    only = torch.empty(m, n, device=DEV)
    eng.gated_sum_backward(a, None, c, d_mul=only)
    assert torch.equal(only, gm)
    eng.gated_sum_backward(a, b, c, d_pre=only)
    assert torch.equal(only, gp)


# ---- StudentPolicy.forward_train + backward ----------------------------------------------------------------------------------------------
def small_case(which):
    sd, info, cfg, d = fixture_case()
    if which == "B=1":
        d = {k: (None if v is None else (v[:, :1] if k == "h0" else v[:1]).contiguous()) for k, v in d.items()}
    else:
        d = {k: (None if v is None else (v if k == "h0" else v[:, :1]).contiguous()) for k, v in d.items()}
    return sd, info, cfg, d


CASES = {"fixture": fixture_case, "default": default_case, "B=1": functools.partial(small_case, "B=1"), "T=1": functools.partial(small_case, "T=1")}


@functools.lru_cache(maxsize=None)
def reference(name):
    sd, info, cfg, d = CASES[name]()
    return (sd, info, cfg, d) + gr.reference(sd, info, d, RECON)


def make_policy(eng, info, cfg, sd):
    from isaac_rover_amd.learning.student import StudentPolicy
    pol = StudentPolicy(eng, info, cfg, device=DEV)
    pol.load_state_dict(sd)
    return pol


@pytest.mark.parametrize("name", list(CASES))
def test_forward_train_and_backward_against_float64(eng, name):
    from isaac_rover_amd.learning.distill import StudentTrainer
    sd, info, cfg, d, g64, l64, g32, l32 = reference(name)
    pol, g = make_policy(eng, info, cfg, sd), dev(d)
    # the forward: against float64 with f32 torch on the CPU as the yardstick, and (without resets) against forward()
    actions, est, h = pol.forward_train(g["x"], g["h0"], g["reset"])
    sd64 = {k: sr.f64(v) for k, v in sd.items()}
    want = gr.unroll(sd64, info, sr.f64(d["x"]), sr.f64(d["h0"]), d["reset"])
    yard = gr.unroll(sd, info, d["x"], d["h0"], d["reset"])
    for nm, a, b, c in (("actions", actions, want[0], yard[0]), ("estimated", est, want[1], yard[1]), ("h", h, torch.stack(want[2]), torch.stack(yard[2]))):
        ok, dd, gap, allowed = gr.verdict(a, b, c)
        print(f"{name} forward_train {nm}: max |d| {dd:.3e} gap {gap:.3e} allowed {allowed:.3e}")
        assert tuple(a.shape) == tuple(b.shape) and ok, nm
    if d["reset"] is None:
        fa, fe, fh = pol.forward(g["x"], g["h0"])
        for nm, a, b, w, c in (("actions", actions, fa, want[0], yard[0]), ("estimated", est, fe, want[1], yard[1]),
                               ("h", h, fh, torch.stack(want[2]), torch.stack(yard[2]))):
            assert gr.verdict(b, w, c)[0], nm                        # forward() passes the same rule: the two agree to twice its margin
    # the backward through the trainer's loss: all 52 gradients and dh0
    tr = StudentTrainer(eng, pol, recon_scale=RECON)
    ls = tr.loss_and_grads(g["x"], g["teacher"], g["h0"], g["reset"], g["target"])
    for nm, a, b, c in zip(("loss", "action_loss", "recon_loss"), ls, l64, l32):
        ok, dd, gap, allowed = gr.verdict(a, b, c)
        print(f"{name} {nm}: {float(a):.8f} want {float(b):.8f} max |d| {dd:.3e} allowed {allowed:.3e}")
        assert ok, nm
    got = {k: v.grad for k, v in pol.state_dict().items() if k != gr.FREE}
    assert len(got) == 52 and pol.log_std_parameter.grad is None
    got["dh0"] = tr.dh0
    assert gr.check_all(got, g64, g32, label=f"{name} ") == []
    first = {k: v.clone() for k, v in got.items()}
    tr.loss_and_grads(g["x"], g["teacher"], g["h0"], g["reset"], g["target"])
    assert all(torch.equal(first[k], (tr.dh0 if k == "dh0" else pol.state_dict()[k].grad)) for k in first)      # two runs, the same bits


# ---- StudentTrainer.update ---------------------------------------------------------------------------------------------------------------
LR, CLIP, UPDATES = 1e-3, 0.1, 20


def torch_loop(sd, info, d, dtype):
    """UPDATES steps of clip_grad_norm_ + torch.optim.Adam on the CPU in ``dtype`` -> the loss before each step"""
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(k != gr.FREE) for k, v in sd.items()}
    params = [v for k, v in leaf.items() if k != gr.FREE]
    opt = torch.optim.Adam(params, lr=LR)
    x, h0, ta, tg = (d[k].to(dtype) for k in ("x", "h0", "teacher", "target"))
    out = []
    for _ in range(UPDATES):
        opt.zero_grad()
        a, s, _ = gr.unroll(leaf, info, x, h0, d["reset"])
        ls = gr.losses(a, s, ta, tg, RECON)
        ls[0].backward()
        torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()
        out.append(ls[0].detach())
    return torch.stack(out)


def test_trainer_update_follows_the_float64_loop(eng):
    from isaac_rover_amd.learning.distill import StudentTrainer
    from isaac_rover_amd.learning.optim import Adam
    sd, info, cfg, d = fixture_case()
    want, yard = torch_loop(sd, info, d, torch.float64), torch_loop(sd, info, d, torch.float32)
    g = dev(d)

    def run():
        pol = make_policy(eng, info, cfg, sd)
        tr = StudentTrainer(eng, pol, lr=LR, grad_norm_clip=CLIP, recon_scale=RECON)
        ls = [tr.update(g["x"], g["teacher"], g["h0"], g["reset"], g["target"]) for _ in range(UPDATES)]
        assert tuple(ls[0][3].shape) == tuple(g["h0"].shape)
        return torch.stack([l[0] for l in ls]).cpu(), pol

    got, pol = run()
    for i in range(UPDATES):
        ok, dd, gap, allowed = gr.verdict(got[i], want[i], yard[i])
        print(f"update {i}: loss {float(got[i]):.8f} float64 {float(want[i]):.8f} f32 torch {float(yard[i]):.8f} |d| {dd:.3e} allowed {allowed:.3e}")
    assert float(got[-1]) < float(got[0])
    assert all(gr.verdict(got[i], want[i], yard[i])[0] for i in range(UPDATES))
    got2, pol2 = run()
    assert torch.equal(got, got2)
    assert all(torch.equal(a, b) for a, b in zip(pol.state_dict().values(), pol2.state_dict().values()))      # two runs end in the same bits
    # one update = loss_and_grads + optim.Adam.step on the same gradients
    pa, pb = make_policy(eng, info, cfg, sd), make_policy(eng, info, cfg, sd)
    StudentTrainer(eng, pa, lr=LR, grad_norm_clip=CLIP, recon_scale=RECON).update(g["x"], g["teacher"], g["h0"], g["reset"], g["target"])
    tb = StudentTrainer(eng, pb, lr=LR, grad_norm_clip=CLIP, recon_scale=RECON, native_step=False)
    tb.loss_and_grads(g["x"], g["teacher"], g["h0"], g["reset"], g["target"])
    Adam(eng, pb.parameters(), lr=LR).step(CLIP)
    assert all(torch.equal(a, b) for a, b in zip(pa.state_dict().values(), pb.state_dict().values()))
    assert not any(torch.equal(a.cpu(), b) for (k, a), b in zip(pa.state_dict().items(), sd.values()) if k != gr.FREE)      # and every tensor moved
    # the torch step (native_step=False) follows the same losses
    pc = make_policy(eng, info, cfg, sd)
    tc = StudentTrainer(eng, pc, lr=LR, grad_norm_clip=CLIP, recon_scale=RECON, native_step=False)
    lc = torch.stack([tc.update(g["x"], g["teacher"], g["h0"], g["reset"], g["target"])[0] for _ in range(UPDATES)]).cpu()
    assert all(gr.verdict(lc[i], want[i], yard[i])[0] for i in range(UPDATES))
