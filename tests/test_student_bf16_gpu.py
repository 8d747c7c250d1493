"""rover_gru_cell_bf16, rover_linear_forward_bf16 and StudentPolicy(precision="bf16") on the GPU against tests/gru_bf16_ref.py (cells,
the student) and tests/bf16_ref.py (one Layer)."""
import copy

import pytest
import torch

import bf16_ref as B
import gru_bf16_ref as G
import mlp_ref as R
import student_ref as sr
from test_student_host import INFO_FULL, act_case_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = {"precision": "bf16"}


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    yield e
    e.close()


def dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def run_cell(eng, d, mask=None):
    g = dev(d)
    out = torch.full_like(g["h"], float("nan"))
    eng.gru_cell(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], out, reset_mask=None if mask is None else mask.to(DEV), **BF)
    return out


def run_cell_trapped(eng, d, mask=None):
    """The cell with x and h at odd offsets and strides inside NaN, weights and biases as heads of NaN-filled buffers, h_out inside a
    canary-filled buffer -> h_out (the canaries are checked)."""
    g = dev(d)
    m, hd = g["h"].shape
    x, h = R.trapped_input(g["x"], 3), R.trapped_input(g["h"], 1)
    out = R.Canary(m, hd, DEV)
    eng.gru_cell(x, h, R.nan_head(g["w_ih"]), R.nan_head(g["w_hh"]), R.nan_head(g["b_ih"]), R.nan_head(g["b_hh"]), out.y,
                 reset_mask=None if mask is None else mask.to(DEV), **BF)
    torch.cuda.synchronize()
    assert out.intact(), "a write outside h_out"
    return out.y.clone()


# ---- the cell -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("m,k,hd", G.LATTICE_CASES)
def test_cell_lattice_inside_the_epilogue_bound(eng, m, k, hd, family):
    d, counts = G.lattice_cell(m, k, hd, family)
    mask = (torch.arange(m) % 3 == 1) if (m + k) % 2 else None
    got = run_cell_trapped(eng, d, mask).cpu()
    want, err = G.cell_bound(d, mask, exact_sums=True)
    diff = (sr.f64(got) - want).abs()
    print(f"gru_cell_bf16 lattice {family} ({m},{k},{hd}): non-representable x / h / w {counts}, max |d| {float(diff.max()):.3e}, "
          f"worst d / bound {float((diff / err).max()):.4f}")
    assert torch.isfinite(got).all() and bool((diff <= err).all())


@pytest.mark.parametrize("m,k,hd", sr.CELL_CASES)
def test_cell_real_valued_inside_the_rounded_operand_bound(eng, m, k, hd):
    d = sr.cell_data(m, k, hd)
    got = run_cell(eng, d).cpu()
    want, err = G.cell_bound(d)
    diff = (sr.f64(got) - want).abs()
    print(f"gru_cell_bf16 ({m},{k},{hd}): max |d| {float(diff.max()):.3e}, worst d / bound {float((diff / err).max()):.4f}")
    assert torch.isfinite(got).all() and bool((diff <= err).all())


def test_cell_reset_mask_rows_permutation_determinism(eng):
    m, k, hd = 129, 124, 300
    d = sr.cell_data(m, k, hd, seed=2)
    mask = torch.arange(m) % 4 == 1
    plain, masked = run_cell(eng, d), run_cell(eng, d, mask)
    zeroed = dict(d, h=torch.where(mask[:, None], torch.zeros_like(d["h"]), d["h"]))
    md = mask.to(DEV)
    assert torch.equal(masked[md], run_cell(eng, zeroed)[md])        # marked rows: the run on a zeroed h, bit for bit
    assert torch.equal(masked[~md], plain[~md])                      # unmarked rows: the unmasked run
    assert not torch.equal(masked[md], plain[md])
    assert torch.equal(run_cell(eng, d, mask.to(torch.uint8) * 7), masked)       # any non-zero byte
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(5))
    pd = dict(d, x=d["x"][perm].contiguous(), h=d["h"][perm].contiguous())
    assert torch.equal(run_cell(eng, pd, mask[perm]), masked[perm.to(DEV)])      # a row's result does not depend on where the row is
    assert torch.equal(run_cell(eng, d, mask), masked)                           # two runs, the same bits


def test_cell_refuses_overlap_and_bad_arguments(eng):
    from isaac_rover_amd._lib import RoverError
    m, k, hd = 33, 3, 44
    g = dev(sr.cell_data(m, k, hd, seed=3))
    cell = lambda *a, **kw: eng.gru_cell(*a, **kw, **BF)
    before = g["h"].clone()
    with pytest.raises(RoverError, match="overlaps h_in"):
        cell(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], g["h"])
    both = torch.zeros(m + 1, hd, device=DEV)
    both[:m] = before
    snap = both.clone()
    with pytest.raises(RoverError, match="overlaps h_in"):
        cell(g["x"], both[:m], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], both[1:])      # shifted by one row
    torch.cuda.synchronize()
    assert torch.equal(g["h"], before) and torch.equal(both, snap)               # nothing was written
    out = torch.full((m, hd), 3.25, device=DEV)
    with pytest.raises(RoverError):
        cell(g["x"], g["h"], g["w_ih"][:, :2].contiguous(), g["w_hh"], g["b_ih"], g["b_hh"], out)
    with pytest.raises(RoverError):
        cell(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"][:-1].contiguous(), g["b_hh"], out)
    with pytest.raises(RoverError):
        cell(g["x"].double(), g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], out)
    with pytest.raises(RoverError):
        cell(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], out[:-1])
    with pytest.raises(RoverError):
        cell(g["x"], g["h"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], out, reset_mask=torch.zeros(m, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == 3.25).all())                                 # nothing was written by a refused call
    # M = 0: a no-op
    e0 = torch.empty(0, hd, device=DEV)
    cell(torch.empty(0, k, device=DEV), e0, g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], torch.empty(0, hd, device=DEV))


# ---- one Layer ------------------------------------------------------------------------------------------------------------------
# M in {1, 17, 129} x K in {0, 1, 33, 300} x N in {1, 33, 120, 128, 256}: every pair (K, N) at an M that walks through the list
LINEAR_CASES = [((1, 17, 129)[(i + j) % 3], k, n) for i, k in enumerate((0, 1, 33, 300)) for j, n in enumerate((1, 33, 120, 128, 256))]
LAST = ("none", "relu", "leakyrelu", "tanh")


def run_linear(eng, x, w, b, act, n):
    out = R.Canary(x.shape[0], n, DEV)
    eng.linear_forward(R.trapped_input(x.to(DEV), 3), R.nan_head(w.to(DEV)), R.nan_head(b.to(DEV)), act, out.y, **BF)
    torch.cuda.synchronize()
    assert out.intact(), "a write outside y"
    return out.y.clone()


@pytest.mark.parametrize("m,k,n", LINEAR_CASES)
def test_linear_lattice_exact(eng, m, k, n):
    act = LAST[(m + k + n) % 4]
    assert eng.linear_route(m, k, n, **BF) == "linear_bf16<128,128>"
    x, layers, want = B.lattice(m, k, (n,), (act,), seed=m + 3 * k + n)
    (w, b, _), = layers
    B.check_exact(run_linear(eng, x, w, b, act, n), want, act, f"linear_bf16 ({m},{k},{n}) {act}")


@pytest.mark.parametrize("m,k,n", LINEAR_CASES)
def test_linear_real_valued_inside_the_interval_bound(eng, m, k, n):
    act = ("leakyrelu", "tanh", "none", "elu")[(m + k + n) % 4]
    x, layers = R.make_data(m, k, (n,), (act,), m + 3 * k + n, "cpu")
    want, bound = B.reference(x, layers)
    (w, b, _), = layers
    ratio = B.check(run_linear(eng, x, w, b, act, n), want, bound, f"linear_bf16 ({m},{k},{n}) {act}")
    print(f"linear_bf16 ({m},{k},{n}) {act}: worst error / bound {ratio:.4f}")


def test_linear_refuses_257_columns(eng):
    from isaac_rover_amd._lib import RoverError
    x, w, b = torch.zeros(4, 8, device=DEV), torch.zeros(257, 8, device=DEV), torch.zeros(257, device=DEV)
    out = torch.full((4, 257), 3.25, device=DEV)
    assert eng.linear_route(4, 8, 257, **BF) is None
    with pytest.raises(RoverError):
        eng.linear_forward(x, w, b, "none", out, **BF)
    torch.cuda.synchronize()
    assert bool((out == 3.25).all())


# ---- StudentPolicy(precision="bf16") ----------------------------------------------------------------------------------------------
def make_policy(eng, sd, cfg=None, **kw):
    from isaac_rover_amd.learning.student import DEFAULT_CFG, StudentPolicy
    pol = StudentPolicy(eng, INFO_FULL, DEFAULT_CFG if cfg is None else cfg, device=DEV, **kw)
    pol.load_state_dict(sd)
    return pol


@pytest.fixture(scope="module")
def sd_full():
    from isaac_rover_amd.learning.student import param_shapes
    return sr.random_state_dict(param_shapes(INFO_FULL), seed=3)


def by_hand(eng, pol, obs, h, reset):
    """One bf16 step composed from the Engine calls alone -> (actions, estimated, [h' per layer])."""
    p, ns, nd = pol.info["proprioceptive"], pol.info["sparse"], pol.info["dense"]
    e, f = obs.shape
    ef, ex = pol.encoder1[-1].weight.shape[0], ns + nd
    new = lambda r, c: torch.full((r, c), float("nan"), device=DEV)
    cat, mlp_in = new(e, p + 2 * ef), new(e, p + 2 * ef)
    cat[:, :p] = obs[:, :p]
    mlp_in[:, :p] = obs[:, :p]
    eng.chain_forward(obs[:, f - ex:f - nd], pol.encoder1, cat[:, p:p + ef], **BF)
    eng.chain_forward(obs[:, f - nd:], pol.encoder2, cat[:, p + ef:], **BF)
    x, hn = cat, []
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(pol.gru):
        x = eng.gru_cell(x, h[l], w_ih, w_hh, b_ih, b_hh, new(e, pol.hidden_dim), reset_mask=reset, **BF)
        hn.append(x)

    def layers(v, ls):                                               # layer by layer, in column blocks of the 256 the library takes
        for layer in ls:
            n = layer.weight.shape[0]
            y = new(v.shape[0], n)
            for lo in range(0, n, 256):
                hi = min(n, lo + 256)
                assert eng.linear_route(v.shape[0], v.shape[1], hi - lo, **BF) is not None
                eng.linear_forward(v, layer.weight[lo:hi], layer.bias[lo:hi], layer.activation, y[:, lo:hi], **BF)
            v = y
        return v

    x_b, x_a = layers(x, pol.gb), layers(x, pol.ga)
    eng.gated_sum(x_b, cat[:, p:], x_a, mlp_in[:, p:])
    actions = eng.chain_forward(mlp_in, pol.network, new(e, pol.info["actions"]), **BF)
    last = x[e - 1:e]
    gate, dec = layers(last, pol.gate_encoder), layers(last, pol.decoder)
    est = new(e, ex)
    eng.gated_sum(dec.expand(e, ex), obs[:, f - ex:], gate.expand(e, ex), est)
    return actions, est, hn


def test_act_bf16_is_the_composition_of_the_engine_calls(eng, sd_full):
    pol = make_policy(eng, sd_full, precision="bf16")
    obs_seq, resets = act_case_inputs()
    pol.init_hidden(33)
    ptr = pol.h.data_ptr()
    h = [torch.zeros(33, 300, device=DEV) for _ in range(2)]
    for t in range(12):
        r = None if resets[t] is None else resets[t].to(DEV)
        obs = obs_seq[t].to(DEV)
        actions, est = pol.act(obs, reset=r, reconstruct=True)
        wa, we, h = by_hand(eng, pol, obs, h, r)
        assert torch.equal(actions, wa) and torch.equal(est, we), t
        assert torch.equal(pol.h[0], h[0]) and torch.equal(pol.h[1], h[1]), t
        assert pol.h.data_ptr() == ptr and pol.h.dtype == torch.float32
    assert torch.isfinite(actions).all() and torch.isfinite(est).all() and torch.isfinite(pol.h).all()
    assert tuple(actions.shape) == (33, 2) and tuple(est.shape) == (33, 50)


def test_f32_policy_keeps_its_bits_next_to_a_bf16_one(eng, sd_full):
    plain, both = make_policy(eng, sd_full), make_policy(eng, sd_full, precision="bf16")
    assert plain.precision == "f32" and both.precision == "bf16"
    obs_seq, resets = act_case_inputs()
    lower = make_policy(eng, sd_full, precision="bf16")
    for t in range(5):
        r = None if resets[t] is None else resets[t].to(DEV)
        obs = obs_seq[t].to(DEV)
        a0, e0 = plain.act(obs, reset=r, reconstruct=True)
        a1, e1 = both.act(obs, reset=r, reconstruct=True, precision="f32")
        assert torch.equal(a0, a1) and torch.equal(e0, e1) and torch.equal(plain.h, both.h), t
        a2 = lower.act(obs, reset=r)
        assert not torch.equal(a0, a2) and float((a0 - a2).abs().max()) < 0.05      # another arithmetic, the same policy
    x = torch.stack([o.to(DEV) for o in obs_seq[:3]], 1)
    h0 = torch.zeros(2, 33, 300, device=DEV)
    for got, want in zip(both.forward(x, h0, precision="f32"), plain.forward(x, h0)):
        assert torch.equal(got, want)


def test_captured_act_bf16_equals_eager(eng, sd_full):
    obs_seq, _ = act_case_inputs()
    obs_seq = [o.to(DEV) for o in obs_seq[:4]]
    eager = make_policy(eng, sd_full, precision="bf16")
    eager.init_hidden(33)
    want = [(eager.act(o).clone(), eager.h.clone()) for o in obs_seq]
    pol = make_policy(eng, sd_full, precision="bf16")
    pol.init_hidden(33)
    static_obs = obs_seq[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act(static_obs)                                          # warm-up: buffers and plans
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(pol.h, want[0][1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pol.act(static_obs)
    ptr = pol.h.data_ptr()
    for t in range(1, 4):
        static_obs.copy_(obs_seq[t])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[t][0]) and torch.equal(pol.h, want[t][1]) and pol.h.data_ptr() == ptr and pol.h.dtype == torch.float32


def test_a_branch_wider_than_one_layer_kernel_runs_in_column_blocks(eng):
    """gb / ga with a first width of 300 > the 256 columns linear_route(..., "bf16") takes: the defined behaviour is the chunking of
    the f32 path (column blocks the library accepts), not a ValueError — and no f32 layer in between."""
    from isaac_rover_amd.learning.student import DEFAULT_CFG, param_shapes
    cfg = copy.deepcopy(DEFAULT_CFG)
    cfg["belief_encoder"]["gb_features"] = [300, 128, 120]
    cfg["belief_encoder"]["ga_features"] = [300, 128, 120]
    assert eng.linear_route(33, 300, 300, **BF) is None
    sd = sr.random_state_dict(param_shapes(INFO_FULL, cfg), seed=4)
    pol = make_policy(eng, sd, cfg, precision="bf16")
    obs_seq, _ = act_case_inputs()
    h = [torch.zeros(33, 300, device=DEV) for _ in range(2)]
    for t in range(2):
        obs = obs_seq[t].to(DEV)
        actions, est = pol.act(obs, reconstruct=True)
        wa, we, h = by_hand(eng, pol, obs, h, None)
        assert torch.equal(actions, wa) and torch.equal(est, we) and torch.equal(pol.h[1], h[1])


def test_distance_to_float64_against_the_emulations(eng, sd_full):
    """max |GPU bf16 - float64| over 12 steps of act() on actions and on h, against the same distance of the CPU emulation of the
    kernels' arithmetic (f32 torch, rd at every operand read): within gru_bf16_ref.F64_MARGIN = 4 x (EXPERIMENTS.md §20)."""
    pol = make_policy(eng, sd_full, precision="bf16")
    sd64 = {k: sr.f64(v) for k, v in sd_full.items()}
    obs_seq, resets = act_case_inputs()
    pol.init_hidden(33)
    zeros = lambda dt: [torch.zeros(33, 300, dtype=dt) for _ in range(2)]
    h64, e64, hem = zeros(torch.float64), zeros(torch.float64), zeros(torch.float32)
    gpu, emu = {"actions": 0.0, "h": 0.0}, {"actions": 0.0, "h": 0.0}
    for t in range(12):
        r = resets[t]
        actions = pol.act(obs_seq[t].to(DEV), reset=None if r is None else r.to(DEV))
        a64, _, _, _, h64, e64 = sr.student_step_b(sd64, INFO_FULL, sr.f64(obs_seq[t]), h64, e64, r)
        aem, _, hem = G.student_step_emulated(sd_full, INFO_FULL, obs_seq[t], hem, r)
        dist = lambda got, want: float((sr.f64(got) - want).abs().max())
        gpu["actions"], emu["actions"] = max(gpu["actions"], dist(actions, a64)), max(emu["actions"], dist(aem, a64))
        for l in range(2):
            gpu["h"], emu["h"] = max(gpu["h"], dist(pol.h[l], h64[l])), max(emu["h"], dist(hem[l], h64[l]))
    for name in ("actions", "h"):
        print(f"bf16 act() over 12 steps, {name}: max |GPU - float64| {gpu[name]:.3e}, max |emulation - float64| {emu[name]:.3e}, "
              f"ratio {gpu[name] / emu[name]:.3f}")
    for name in ("actions", "h"):
        assert gpu[name] <= G.F64_MARGIN * emu[name], name
