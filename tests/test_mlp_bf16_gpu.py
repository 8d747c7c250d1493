"""GPU: the bf16 chain kernels (csrc/rover_mlp.hip chain_bf16<...>, rover_mlp_chain_forward_bf16 / rover_mlp_chain_act_bf16) and
HeightmapNet(precision="bf16").

The weight rests on LATTICE data (tests/bf16_ref.py): integer inputs, weights in {-1, 0, +1}, integer biases, every partial sum below
2^24 — the result is determined bit for bit whatever the summation order, and is compared with ==.  Every lattice run reads its input
as an odd-offset, odd-stride column slice of a NaN-filled tensor, its weights and biases as heads of NaN-filled buffers, and writes
into a column slice of a canary-filled tensor.  The same shapes then run LeakyReLU nets on mlp_ref.make_data against the interval bound
(the worst error / bound ratio is printed), twice, with equal bits."""
import itertools

import numpy as np
import pytest
import torch

import bf16_ref as B
import mlp_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MS = (1, 15, 16, 17, 127, 128, 129, 300)          # 300 rows span three workgroups
K0S = (1, 31, 32, 33, 124, 634)
W2 = ((80, 60), (96, 64), (17, 3))
W4 = ((256, 160, 128, 2), (256, 160, 128, 16), (100, 50, 20, 1))
LAST = ("none", "relu", "leakyrelu", "tanh")


def _cases(k_main, w_main, widths_all):
    """Every M at the main shape; every (K0, widths) of the grid at an M that walks through MS."""
    out = [(m, k_main, w_main) for m in MS]
    for i, (k0, w) in enumerate(itertools.product(K0S, widths_all)):
        if (k0, w) != (k_main, w_main):
            out.append((MS[(3 * i + 1) % len(MS)], k0, w))
    return out


CASES = _cases(634, (80, 60), W2) + _cases(124, (256, 160, 128, 2), W4)
ROUTE = {(80, 60): "chain_bf16<5,4,0,0>", (96, 64): "chain_bf16<6,4,0,0>", (17, 3): "chain_bf16<5,4,0,0>"}


def _id(case):
    return "-".join(str(v).replace(" ", "") for v in case)


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(8, device=0)
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _trapped(x, layers, seed):
    x, layers = x.to(DEV), [(w.to(DEV), b.to(DEV), a) for w, b, a in layers]
    return R.trapped_input(x, 1 + 2 * (seed % 2)), R.trapped_layers(layers)


def _run_twice(eng, x, layers, n, label):
    """-> y of the first run; the canaries are intact and a second run writes the same bits."""
    out = R.Canary(x.shape[0], n, DEV)
    eng.chain_forward(x, layers, out.y, precision="bf16")
    torch.cuda.synchronize()
    assert out.intact(), f"{label}: a write outside the output slice"
    first = out.y.clone()
    out.y.fill_(float("nan"))
    eng.chain_forward(x, layers, out.y, precision="bf16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.y), _bits(first)), f"{label}: the second run differs"
    return first


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_lattice_exact(eng, case):
    m, k0, widths = case
    seed = m + 3 * k0 + sum(widths)
    acts = tuple(("relu", "none")[(seed + i) % 2] for i in range(len(widths) - 1)) + (LAST[seed % 4],)
    assert eng.chain_route(m, k0, widths, acts, precision="bf16") == ROUTE.get(widths, "chain_bf16<16,10,8,1>")
    x, layers, want = B.lattice(m, k0, widths, acts, seed)
    xt, lt = _trapped(x, layers, seed)
    y = _run_twice(eng, xt, lt, widths[-1], _id(case))
    B.check_exact(y, want, acts[-1], f"{_id(case)} {acts}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_leakyrelu_inside_the_interval_bound(eng, case):
    m, k0, widths = case
    seed = m + 3 * k0 + sum(widths)
    acts = ("leakyrelu",) * (len(widths) - 1) + (("tanh", "none", "leakyrelu", "elu")[seed % 4],)
    x, layers = R.make_data(m, k0, widths, acts, seed, "cpu")
    want, bound = B.reference(x, layers)
    xt, lt = _trapped(x, layers, seed)
    y = _run_twice(eng, xt, lt, widths[-1], _id(case))
    ratio = B.check(y, want, bound, f"{_id(case)} {acts}")
    print(f"bf16 interval bound {_id(case)}: worst error / bound = {ratio:.3g}")


# ---- the Gaussian head on the bf16 mean -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,a_dim", [(300, 2), (129, 16), (17, 1), (128, 4)], ids=str)
def test_chain_act_is_forward_then_head(eng, m, a_dim):
    widths = (256, 160, 128, a_dim)
    acts = ("leakyrelu", "leakyrelu", "leakyrelu", "tanh")
    assert eng.chain_act_route(m, 124, widths, acts, precision="bf16") == "chain_bf16<16,10,8,1>" + ("+gauss" if a_dim <= 4 else ";gauss")
    x, layers = R.make_data(m, 124, widths, acts, seed=m + a_dim, device=DEV)
    lt = R.trapped_layers(layers)
    xt = R.trapped_input(x, 3)
    log_std = torch.linspace(-1.0, 0.5, a_dim, device=DEV)
    head = dict(seed=77, step=5, row_offset=1000)
    new = lambda *s: torch.full(s, float("nan"), device=DEV)

    mean_f = eng.chain_forward(xt, lt, new(m, a_dim), precision="bf16")
    act_h, lp_h = eng.gaussian_head(mean_f, log_std, new(m, a_dim), new(m, 1), **head)
    mean_a, act_a, lp_a = new(m, a_dim), new(m, a_dim), new(m, 1)
    eng.chain_act(xt, lt, mean_a, log_std, act_a, lp_a, precision="bf16", **head)
    torch.cuda.synchronize()
    assert torch.equal(_bits(mean_a), _bits(mean_f))
    assert torch.equal(_bits(act_a), _bits(act_h)) and torch.equal(_bits(lp_a), _bits(lp_h))
    assert bool(torch.isfinite(act_a).all()) and bool(torch.isfinite(lp_a).all()) and not torch.equal(act_a, mean_a)

    act_t, lp_t = new(m, a_dim), new(m, 1)                              # taken_actions = the returned actions: the same log_prob bits
    eng.chain_act(xt, lt, new(m, a_dim), log_std, act_t, lp_t, precision="bf16", taken_actions=act_a.clone(), **head)
    act_d, lp_d = new(m, a_dim), new(m, 1)
    eng.chain_act(xt, lt, new(m, a_dim), log_std, act_d, lp_d, precision="bf16", deterministic=True, **head)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lp_t), _bits(lp_a))
    assert torch.equal(_bits(act_d), _bits(mean_f))


# ---- HeightmapNet(precision="bf16") on the reference's weights ------------------------------------------------------------------------
def _p37(eng, outputs, head, tag, **kw):
    from isaac_rover_amd.learning.model import HeightmapNet
    fx = load_golden("policy_p37")
    nobs, ns, nd = int(fx["num_observations"]), int(fx["num_sparse"]), int(fx["num_dense"])
    net = HeightmapNet(eng, nobs, ns, nd, outputs, head, **kw)
    net.load_state_dict({k[len(tag) + 1:]: torch.from_numpy(v.astype(np.float32)) for k, v in fx.items() if k.startswith(tag + ".")})
    return net, torch.from_numpy(fx["states"].astype(np.float32)).to(DEV), fx


def _layers(ls):
    return [(l.weight, l.bias, l.activation) for l in ls]


@pytest.mark.parametrize("tag,outputs,head", [("actor", 2, "tanh"), ("critic", 1, None)], ids=["actor", "critic"])
def test_net_compute_bf16(eng, tag, outputs, head):
    net, x, fx = _p37(eng, outputs, head, tag, precision="bf16")
    p, ns, nd, ef = net.num_proprioception, net.num_sparse, net.num_dense, 60
    y = net.compute(x).clone()
    # the composition of the Engine calls, bit for bit (the dense slice of this net is EMPTY: a chain with K0 = 0)
    cat = torch.empty(x.shape[0], p + 2 * ef, device=DEV)
    cat[:, :p] = x[:, :p]
    eng.chain_forward(x[:, p:p + ns], net.encoder0, cat[:, p:p + ef], precision="bf16")
    eng.chain_forward(x[:, p + ns:p + ns + nd], net.encoder1, cat[:, p + ef:p + 2 * ef], precision="bf16")
    y2 = eng.chain_forward(cat, net.network, torch.empty(x.shape[0], outputs, device=DEV), precision="bf16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(y2))
    assert torch.equal(_bits(net.compute(x, precision="bf16")), _bits(y))
    acted = net.act(x, deterministic=True)[0] if head else net.act(x)[0]       # the actor's mean / the critic's value: the same forward
    assert torch.equal(_bits(acted), _bits(y))
    # inside the interval bound of the bf16 reference, chain after chain
    e0, b0 = B.reference(x[:, p:p + ns], _layers(net.encoder0))
    e1, b1 = B.reference(x[:, p + ns:p + ns + nd], _layers(net.encoder1))
    cat64 = torch.cat([x[:, :p].cpu().double(), e0, e1], dim=1)
    want, bound = B.reference(cat64, _layers(net.network), e0=torch.cat([torch.zeros(x.shape[0], p, dtype=torch.float64), b0, b1], dim=1))
    ratio = B.check(y, want, bound, tag)
    f32 = fx["out_" + tag]
    print(f"bf16 net {tag}: worst error / bound = {ratio:.3g}; max |bf16 - f32 fixture| = {float(np.abs(y.cpu().numpy() - f32).max()):.3g} "
          f"(max |f32| = {float(np.abs(f32).max()):.3g})")
    # the default stays f32, per call too
    np.testing.assert_allclose(net.compute(x, precision="f32").cpu().numpy(), f32, atol=2e-5, rtol=2e-4)
    # no stale copy of the weights: one changed in place changes the next output
    net.network[0].weight[0, 0] += 8.0
    net.encoder0[0].bias[3] -= 4.0
    y3 = net.compute(x).clone()
    torch.cuda.synchronize()
    assert not torch.equal(_bits(y3), _bits(y))


def test_net_precision_errors(eng):
    from isaac_rover_amd.learning.model import HeightmapNet
    net, x, _ = _p37(eng, 2, "tanh", "actor")
    assert net.precision == "f32"
    with pytest.raises(ValueError, match="fused=False"):
        net.compute(x, fused=False, precision="bf16")
    with pytest.raises(ValueError, match="fused=False"):
        net.act(x, fused=False, precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        net.compute(x, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        HeightmapNet(eng, 41, 37, 0, 2, "tanh", precision="fp16")
    net.compute(x, precision="bf16")
    with pytest.raises(RuntimeError, match="fused"):
        net.backward(torch.zeros(x.shape[0], 2, device=DEV))
    net.compute(x, fused=False)                                          # an f32 layer-by-layer forward: backward runs again
    net.backward(torch.zeros(x.shape[0], 2, device=DEV))
    wide = HeightmapNet(eng, 41, 37, 0, 2, "tanh", encoder_features=(100, 60), precision="bf16")      # 100 > 96: no chain kernel
    with pytest.raises(ValueError, match="encoder0"):
        wide.compute(x)
    tanh_hidden = HeightmapNet(eng, 41, 37, 0, 2, "tanh", activation_function="tanh", precision="bf16")
    with pytest.raises(ValueError, match="network"):
        tanh_hidden.act(x)
    wide.compute(x, precision="f32")                                     # f32 runs such nets layer by layer, as before
    torch.cuda.synchronize()
