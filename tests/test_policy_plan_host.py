"""CPU: the Python side of the policy nets holds no routing rule of its own any more — ``Engine.chain_fits`` and ``HeightmapNet``'s
forward plan are answers of the library's route queries.  Here the rule they used to restate (the widths table, the hidden activations,
the row switch of the encoder pair) is written out ONCE, as the expectation, and both must agree with it over a grid around every
switch point; compute() / act() must then make exactly the engine calls the old code made.  No device: the nets live on torch's
"meta" device and the engine is a recorder that forwards the route queries to the library."""
import itertools
from types import SimpleNamespace

import pytest
import torch

ACTS = ("none", None, "leakyrelu", "tanh", "relu", "elu")
ENC_WIDTHS = list(itertools.product((1, 80, 81, 96, 97), (64, 65)))
MLP_WIDTHS = list(itertools.product((256, 257), (160, 161), (128, 129), (16, 17)))
K0S = (0, 1, 127, 128, 256, 257)
ROWS = (1, 20479, 20480)


# ---- the rule as Python used to hold it (Engine.CHAIN_SHAPES / CHAIN_HIDDEN_ACTS / chain_fits, HeightmapNet._encode) ----
OLD_SHAPES = {2: (96, 64), 4: (256, 160, 128, 16)}
OLD_HIDDEN_ACTS = (None, "none", "leakyrelu", "relu")


def old_fits(layers):
    lim = OLD_SHAPES.get(len(layers))
    if lim is None or not all(l.weight.shape[0] <= m for l, m in zip(layers, lim)) or layers[0].weight.shape[1] <= 0:
        return False
    return len(layers) == 2 or all(l.activation in OLD_HIDDEN_ACTS for l in layers[:-1])


def old_forward(net, rows, fused):
    """-> (plan, engine calls of the encoders, whether the MLP + head is one chain) as the old _encode / compute / act decided them."""
    if fused is None:
        fused = True
    ns, nd = net.num_sparse, net.num_dense
    if (fused and ns > 0 and nd > 0 and rows < 20480 and len(net.encoder0) == 2 and len(net.encoder1) == 2
            and old_fits(net.encoder0) and old_fits(net.encoder1)):
        return (True, True, True, old_fits(net.network)), ["chain_pair_forward"], old_fits(net.network)
    calls, chains = [], []
    for enc, n in ((net.encoder0, ns), (net.encoder1, nd)):
        chains.append(bool(fused and n > 0 and old_fits(enc)))
        calls += ["chain_forward"] if chains[-1] else ["linear_forward"] * len(enc)
    mlp = bool(fused and old_fits(net.network))
    return (False, chains[0], chains[1], mlp), calls, mlp


def _layers(k0, widths, acts):
    out, k = [], k0
    for n, a in zip(widths, acts):
        out.append(SimpleNamespace(weight=torch.empty(n, k, device="meta"), activation=a))
        k = n
    return out


def _act_patterns(n_layers):
    """Every activation name on every layer at once, and on each single layer among LeakyReLU layers."""
    pats = {(a,) * n_layers for a in ACTS}
    for i in range(n_layers):
        pats |= {tuple(a if j == i else "leakyrelu" for j in range(n_layers)) for a in ACTS}
    return sorted(pats, key=str)


@pytest.mark.parametrize("widths", ENC_WIDTHS + MLP_WIDTHS + [(80,), (256, 160, 128), (96, 64, 64, 16, 2)], ids=str)
def test_chain_fits_is_the_librarys_answer(widths):
    from isaac_rover_amd import _lib
    E = _lib.Engine
    for acts in _act_patterns(len(widths)):
        for k0 in K0S:
            layers = _layers(k0, widths, acts)
            want = old_fits(layers)
            assert E.chain_fits(layers) == want, (widths, acts, k0)
            for m in ROWS:                                           # ... at every batch size: fitting does not depend on the rows
                assert (E.chain_route(m, k0, widths, acts) is not None) == want, (m, widths, acts, k0)
    assert not E.chain_fits([])


class Recorder:
    """Stands in for an Engine: answers the route queries from the library, records the forward calls."""

    def __init__(self, lib_engine):
        self.calls = []
        self.chain_route, self.chain_pair_route, self.chain_shape, self.chain_fits = (
            lib_engine.chain_route, lib_engine.chain_pair_route, lib_engine.chain_shape, lib_engine.chain_fits)

    def linear_forward(self, x, weight, bias, activation, out):
        self.calls.append("linear_forward")
        return out

    def chain_forward(self, x, layers, out):
        self.calls.append("chain_forward")
        return out

    def chain_pair_forward(self, xa, la, oa, xb, lb, ob, copy_src=None, copy_dst=None, copy_cols=0):
        assert copy_src is not None and copy_dst is not None
        self.calls.append("chain_pair_forward")

    def chain_act(self, x, layers, mean, log_std, actions, log_prob, **head):
        self.calls.append("chain_act")

    def gaussian_head(self, mean, log_std, actions, log_prob, **head):
        self.calls.append("gaussian_head")


@pytest.mark.parametrize("enc", ENC_WIDTHS, ids=str)
def test_forward_plan_and_calls_match_the_old_rule(enc, monkeypatch):
    """Nets over the whole grid — encoder widths x MLP widths (the head's width is the net's output count) x every activation name x
    slice sizes ns, nd in {0, 37} x MLP input lengths 4 + 2 ef and, where a proprioception width gives them, 256 and 257: the plan per
    (rows, fused) equals the old rule's, and compute() / act() make the old code's engine calls in the old order."""
    from isaac_rover_amd import _lib
    from isaac_rover_amd.learning import model
    HeightmapNet = model.HeightmapNet
    # thousands of nets whose weights are never read: their layers hold shapes only, nothing is drawn
    monkeypatch.setattr(model, "Layer", lambda i, o, act="elu", device=None, generator=None: SimpleNamespace(
        weight=torch.empty(o, i, device="meta"), bias=torch.empty(o, device="meta"), activation=act))
    checked = 0
    for mlp, act, ns, nd in itertools.product(MLP_WIDTHS, ACTS, (0, 37), (0, 37)):
        for p in {4} | {k0 - 2 * enc[1] for k0 in K0S if k0 - 2 * enc[1] >= 0}:
            for head in ("tanh", None):
                rec = Recorder(_lib.Engine)
                net = HeightmapNet(rec, p + ns + nd, ns, nd, mlp[3], head, mlp_features=mlp[:3], encoder_features=enc, activation_function=act,
                                   device="meta")
                assert net.network[0].weight.shape[1] == p + 2 * enc[1]
                for rows, fused in itertools.product(ROWS, (None, False)):
                    what = (enc, mlp, act, ns, nd, p, head, rows, fused)
                    plan, enc_calls, mlp_chain = old_forward(net, rows, fused)
                    assert tuple(net._plan(rows, fused is None)) == plan, what
                    states = torch.empty(rows, p + ns + nd, device="meta")
                    forward = enc_calls + (["chain_forward"] if mlp_chain else ["linear_forward"] * 4)
                    if head is None:                                 # the critic: act() is compute()
                        want = forward
                    else:
                        net.compute(states, fused)
                        assert rec.calls == forward, what
                        rec.calls.clear()
                        want = enc_calls + (["chain_act"] if mlp_chain else ["linear_forward"] * 4 + ["gaussian_head"])
                    net.act(states, fused=fused)
                    assert rec.calls == want, what
                    rec.calls.clear()
                    checked += 1
    assert checked == 16 * 6 * 4 * 2 * 6 * len({4} | {k0 - 2 * enc[1] for k0 in K0S if k0 - 2 * enc[1] >= 0})


def test_deeper_encoders_never_pair():
    """The pair call is for 2-layer encoders: a 4-layer encoder that fits a chain kernel runs as a chain of its own."""
    from isaac_rover_amd import _lib
    from isaac_rover_amd.learning.model import HeightmapNet
    net = HeightmapNet(Recorder(_lib.Engine), 4 + 300 + 300, 300, 300, 2, "tanh", encoder_features=(256, 160, 128, 16), device="meta")
    for rows in ROWS:
        assert tuple(net._plan(rows, True)) == old_forward(net, rows, True)[0] == (False, True, True, True)
