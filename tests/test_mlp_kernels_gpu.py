"""GPU: every policy-net kernel instantiation (csrc/rover_mlp.hip) at the edges of its dispatch rules, against the float64 reference
and its rigorous per-element bound (tests/mlp_ref.py).

Each case asserts the route it expects before launching, reads its input as an odd-offset column slice of a NaN-filled tensor and its
weights and biases as heads of NaN-filled buffers (any read past K, N or the rows poisons an output), writes into a column slice of a
canary-filled tensor (every canary must survive), uses data on which a dropped last column, a neighbouring row or a neighbouring bias
would break the bound, and runs twice with bitwise-equal results (split-k's partial sums are added in a fixed order)."""
import itertools

import pytest
import torch

import mlp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A = R.ACTS
HIDDEN = ("none", "leakyrelu", "relu")          # what the 4-layer kernels accept on hidden layers


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(8, device=0)
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- case tables: (M, K, N, activation, route) / (M, K0, widths, activations, route) -----------------------------------------
def _spread(shapes):
    """(M, K0, widths, route) -> cases with activations dealt per route: the c-th case of a route gives layer l activation
    c + 2 l of its pool (all five on a 2-layer chain's layers and on every last layer, none / LeakyReLU / ReLU on the hidden layers of
    a 4-layer net), so a route with >= 5 cases sees every activation it accepts on every layer."""
    seen, out = {}, []
    for m, k0, widths, route in shapes:
        c = seen[route] = seen.get(route, -1) + 1
        pools = [A if len(widths) == 2 or li == len(widths) - 1 else HIDDEN for li in range(len(widths))]
        out.append((m, k0, widths, tuple(p[(c + 2 * li) % len(p)] for li, p in enumerate(pools)), route))
    return out


LINEAR_SMALL = [(m, k, n, A[i % 5], "linear_act<1,1>")
                for i, (m, n, k) in enumerate(itertools.product((1, 31, 33), (1, 31, 33, 256), (0, 1, 31, 32, 33, 1112)))]
LINEAR_SMALL += [(65535, 1112, 1, "elu", "linear_act<1,1>"), (65535, 0, 33, "tanh", "linear_act<1,1>"),
                 (65535, 33, 256, "leakyrelu", "linear_act<1,1>"), (65535, 32, 31, "relu", "linear_act<1,1>")]

WIDE_ROUTE = {1: "linear_act<1,4>", 33: "linear_act<2,4>", 96: "linear_act<3,4>", 97: "linear_act<4,4>", 160: "linear_act<5,4>",
              161: "linear_act<3,4>x2", 192: "linear_act<3,4>x2", 193: "linear_act<4,4>x2", 256: "linear_act<4,4>x2"}
LINEAR_WIDE = [((65536, 65536 + 77)[j % 2], (5, 33, 634)[(i + j) % 3], n, A[(i + j) % 5], WIDE_ROUTE[n])
               for i, n in enumerate(WIDE_ROUTE) for j in range(5)]

_N0, _N1 = (1, 17, 80, 81, 96), (1, 17, 64)
_MK = [(m, k) for m in (1, 127, 128, 129) for k in (1, 3, 33, 127)] + [(m, k) for m in (20480, 65537) for k in (1, 3, 33, 127, 128, 634, 1112)]
CHAIN2 = _spread([(m, k, (_N0[i % 5], _N1[i % 3]), "chain16<5,4,0,0>" if _N0[i % 5] <= 80 else "chain16<6,4,0,0>")
                  for i, (m, k) in enumerate(_MK)])

SPLITK = _spread([(m, k, ((80, 81, 80, 96)[i % 4], (1, 17, 60, 64)[i % 3]), f"splitk<{6 if i % 2 else 5},{2 if m >= 2048 else 1}>")
                  for i, (m, k) in enumerate(itertools.product((1, 16, 17, 2047, 2048, 20479), (128, 129, 634, 1105, 1112, 4099)))])

WIDTHS4 = [(256, 160, 128, 16), (1, 1, 1, 1), (17, 33, 15, 2), (129, 16, 5, 2), (128, 160, 128, 1)]
MLP_SMALL = _spread([((1, 16, 17, 20479)[i % 4], (1, 17, 124, 256)[(i + i // 4) % 4], WIDTHS4[(i + i // 5) % 5], "mlp_small")
                     for i in range(20)])
CHAIN16_LONG = _spread([(m, (124, 17, 256, 1, 33)[(i + j) % 5], w, "chain16<16,10,8,1>") for i, w in enumerate(WIDTHS4)
                        for j, m in enumerate((20480, 65537))] +
                       [(300, 257, (256, 160, 128, 16), "chain16<16,10,8,1>"), (300, 1112, (129, 16, 5, 2), "chain16<16,10,8,1>")])
CHAINS = CHAIN2 + SPLITK + MLP_SMALL + CHAIN16_LONG

# (M, chain a (K0, widths, acts), chain b, copy_cols, route)
_E80 = lambda k0, acts=("leakyrelu", "leakyrelu"): (k0, (80, 60), acts)
_E96 = lambda k0, acts=("elu", "tanh"): (k0, (96, 64), acts)
PAIRS = [(1, _E80(634), _E80(1112, ("relu", "tanh")), 0, "pair(splitk<5,1>)"),
         (17, _E80(634, ("elu", "none")), _E80(1112), 4, "pair(splitk<5,1>)"),
         (2048, _E80(634), _E80(1112, ("tanh", "elu")), 7, "pair(splitk<5,2>)"),
         (20479, _E80(634, ("none", "relu")), _E80(1112), 4, "pair(splitk<5,2>)"),
         (17, _E96(634), _E96(1112, ("leakyrelu", "relu")), 7, "pair(splitk<6,1>)"),
         (17, _E80(634), _E96(1112), 4, "seq(splitk<5,1>;splitk<6,1>)"),
         (2048, _E96(1112), _E80(634), 7, "seq(splitk<6,2>;splitk<5,2>)"),
         (20480, _E80(634), _E80(1112), 7, "seq(chain16<5,4,0,0>;chain16<5,4,0,0>)")]

BUILT = ["linear_act<1,1>"] + [f"linear_act<{nt},4>" for nt in range(1, 6)] + ["linear_act<3,4>x2", "linear_act<4,4>x2"] + \
        [f"splitk<{tn},{rt}>" for tn in (5, 6) for rt in (1, 2)] + \
        ["mlp_small", "chain16<5,4,0,0>", "chain16<6,4,0,0>", "chain16<16,10,8,1>", "pair(splitk<5,1>)", "pair(splitk<5,2>)", "pair(splitk<6,1>)"]


def _id(case):
    return "-".join(str(v).replace(" ", "") for v in case[:-1])


# ---- runners -----------------------------------------------------------------------------------------------------------------
def _chain_data(m, k0, widths, acts, seed):
    x, layers, want, bound = R.sensitive_data(m, k0, widths, acts, seed, DEV)
    return R.trapped_input(x, 1 + 2 * (seed % 2)), R.trapped_layers(layers), want, bound


def _twice(call, out, label):
    """call() writes out.y: within the bound is checked by the caller; here the canaries and a bitwise-equal second run."""
    torch.cuda.synchronize()
    assert out.intact(), f"{label}: a write outside the output slice"
    first = out.y.clone()
    out.y.fill_(float("nan"))
    call()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.y), _bits(first)), f"{label}: the second run differs"


@pytest.mark.parametrize("case", LINEAR_SMALL + LINEAR_WIDE, ids=_id)
def test_linear_forward(eng, case):
    m, k, n, act, route = case
    assert eng.linear_route(m, k, n) == route
    x, (l,), want, bound = _chain_data(m, k, (n,), (act,), seed=m + 7 * k + n)
    out = R.Canary(m, n, DEV)
    call = lambda: eng.linear_forward(x, l.weight, l.bias, act, out.y)
    call()
    torch.cuda.synchronize()
    R.check(out.y, want, bound, route)
    _twice(call, out, route)


@pytest.mark.parametrize("case", CHAINS, ids=_id)
def test_chain_forward(eng, case):
    m, k0, widths, acts, route = case
    assert eng.chain_route(m, k0, widths, acts) == route
    x, layers, want, bound = _chain_data(m, k0, widths, acts, seed=m + 3 * k0 + sum(widths))
    out = R.Canary(m, widths[-1], DEV)
    call = lambda: eng.chain_forward(x, layers, out.y)
    call()
    torch.cuda.synchronize()
    R.check(out.y, want, bound, route)
    _twice(call, out, route)
    h = x                                        # the same net one rover_linear_forward per layer: the same bound
    for l in layers:
        h = eng.linear_forward(h, l.weight, l.bias, l.activation, torch.empty(m, l.weight.shape[0], device=DEV))
    torch.cuda.synchronize()
    R.check(h, want, bound, "layer by layer")


@pytest.mark.parametrize("case", PAIRS, ids=_id)
def test_chain_pair_forward(eng, case):
    m, ca, cb, copy_cols, route = case
    assert eng.chain_pair_route(m, ca, cb) == route
    xa, la, want_a, bound_a = _chain_data(m, *ca, seed=m + 1)
    xb, lb, want_b, bound_b = _chain_data(m, *cb, seed=m + 2)
    out_a, out_b = R.Canary(m, ca[1][-1], DEV), R.Canary(m, cb[1][-1], DEV, offset=3)
    src = R.trapped_input(torch.rand(m, 8, device=DEV) * 4 - 2, 3)
    dst = R.Canary(m, max(copy_cols, 1), DEV)
    kw = dict(copy_src=src, copy_dst=dst.y, copy_cols=copy_cols) if copy_cols else {}
    call = lambda: eng.chain_pair_forward(xa, la, out_a.y, xb, lb, out_b.y, **kw)
    call()
    torch.cuda.synchronize()
    R.check(out_a.y, want_a, bound_a, route + " a")
    R.check(out_b.y, want_b, bound_b, route + " b")
    if copy_cols:
        assert torch.equal(dst.y, src[:, :copy_cols])
    assert dst.intact() and out_b.intact()
    b_first = out_b.y.clone()
    out_b.y.fill_(float("nan"))
    _twice(call, out_a, route)
    assert torch.equal(_bits(out_b.y), _bits(b_first)), f"{route}: chain b's second run differs"


def test_every_built_instantiation_is_a_case_route():
    """Computed from the route query alone (no launch): a routing change that moves a kernel out of this module's cases fails here."""
    from isaac_rover_amd._lib import Engine
    seen = {Engine.linear_route(m, k, n) for m, k, n, _, _ in LINEAR_SMALL + LINEAR_WIDE}
    seen |= {Engine.chain_route(m, k0, w, a) for m, k0, w, a, _ in CHAINS}
    for m, ca, cb, _, _ in PAIRS:
        seen |= {Engine.chain_pair_route(m, ca, cb), Engine.chain_route(m, *ca), Engine.chain_route(m, *cb)}
    assert not set(BUILT) - seen, sorted(set(BUILT) - seen)
    assert all(r in seen for r in ("seq(splitk<5,1>;splitk<6,1>)", "seq(chain16<5,4,0,0>;chain16<5,4,0,0>)"))
    acts = {}                                              # every route sees every activation it accepts, on the hidden and the last layer
    for m, k0, w, a, route in CHAINS:
        for li, act in enumerate(a):
            acts.setdefault((route, li == len(a) - 1), set()).add(act)
    for (route, last), got in acts.items():
        allowed = set(A) if last or route.startswith(("splitk", "chain16<5", "chain16<6")) else set(HIDDEN)
        assert got == allowed, (route, last, sorted(allowed - got))
    lin = {}
    for m, k, n, act, route in LINEAR_SMALL + LINEAR_WIDE:
        lin.setdefault(route, set()).add(act)
    assert all(v == set(A) for v in lin.values()), lin


def test_splitk_scratch_regrowth():
    """A small batch, a larger one (the ctx's split-k scratch is reallocated), the small one again: every result within the bound."""
    from isaac_rover_amd import _lib
    e = _lib.Engine(8, device=0)
    try:
        for m in (17, 2047, 20479, 17, 2047):
            assert e.chain_route(m, 1112, (96, 60), ("elu", "tanh")).startswith("splitk<6,")
            x, layers, want, bound = _chain_data(m, 1112, (96, 60), ("elu", "tanh"), seed=m)
            out = R.Canary(m, 60, DEV)
            e.chain_forward(x, layers, out.y)
            torch.cuda.synchronize()
            R.check(out.y, want, bound, f"M={m}")
            assert out.intact()
    finally:
        e.close()
