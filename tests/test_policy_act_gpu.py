"""GPU: the actor's act() — device noise against its numpy restatement, every route of the Gaussian head against float64
``torch.distributions.Normal`` within the bounds of tests/gauss_ref.py (NaN traps on every input, canaries round every output),
the taken-actions identity, invariance under batch size / sharding / kernel route, graph replay, the reference's weights, the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gauss_ref as G
import mlp_ref as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID = ("leakyrelu", "relu", "none")
NATIVE = dict(num_observations=1750, num_sparse=634, num_dense=1112)


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(8, device=0)
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got, want, bound, label):
    d = (got.double() - want).abs()
    bad = ~(d <= bound)
    print(f"{label}: max |d| {float(d[~torch.isnan(d)].max()) if d.numel() else 0.0:.3e}, max |d| / bound "
          f"{float((d / bound.clamp_min(G.TINY)).max()) if d.numel() else 0.0:.3f}")
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {got.numel()} outside the bound; first at {idx}: got {float(got[idx])!r}, "
                             f"want {float(want[idx])!r} +- {float(bound[idx]):.3e}")


# ---- 4. device noise vs the numpy restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 512, 20479, 20480, 65536])
def test_device_noise_matches_definition(eng, m):
    for i, (row_offset, t, a, seed) in enumerate([(0, 0, 2, 1234), (32768, 1, 2, 1234), (0, 2 ** 32, 5, 99), (32768, 2 ** 32 + 1, 16, 2 ** 63 + 5),
                                                  (2 ** 32 - m, 7, 1, 3)]):
        out = R.Canary(m, a, DEV)
        t_dev = torch.tensor([t - 1 if i % 2 else 0], dtype=torch.int64, device=DEV)      # the counter split over step and *step_dev
        eng.policy_noise(m, a, seed=seed, step=(1 if i % 2 else t), step_dev=t_dev, row_offset=row_offset, out=out.y)
        torch.cuda.synchronize()
        assert out.intact()
        want, rad = G.noise(seed, t, row_offset + np.arange(m), a)
        got = out.y.cpu().double().numpy()
        d = np.abs(got - want)
        print(f"M={m} offset={row_offset} t={t} A={a}: max |d| / (u (1 + rad)) = {float((d / (G.U * (1 + rad))).max()):.2f}")
        assert np.isfinite(got).all() and (d <= G.noise_bound(rad)).all()
        assert float(np.abs(got).max()) <= G.EPS_MAX * (1 + 4 * G.U)


# ---- 5. every route of the head -----------------------------------------------------------------------------------------------------
def _ls(kind, a):
    base = {"zero": [0.0], "min": [-20.0], "max": [2.0], "beyond": [-25.0, 3.0], "mixed": [0.0, -1.5, 0.7, -20.0, 2.0, -3.0]}[kind]
    return torch.tensor([base[j % len(base)] for j in range(a)], device=DEV)


# (log_std kind, clip_log_std, clip_actions, deterministic, reduction, taken_actions)
CONFIGS = [("zero", True, False, False, "sum", False), ("min", True, False, False, "sum", False), ("max", True, False, False, "sum", False),
           ("beyond", True, False, False, "sum", False), ("beyond", False, False, False, "sum", False), ("mixed", True, True, False, "sum", False),
           ("max", True, True, False, "mean", False), ("mixed", True, False, True, "sum", False), ("mixed", False, False, False, "mean", False),
           ("mixed", True, False, False, "prod", False), ("zero", True, False, False, "max", False), ("mixed", True, False, False, "min", False),
           ("mixed", True, False, False, None, False), ("mixed", True, False, False, "sum", True), ("beyond", False, True, False, None, True)]


def _head_case(eng, run, mean_of, m, a, label, want_mean=None, bound_mean=None):
    """run(mean_out, log_std, actions, log_prob, **head) on every CONFIG; mean_of(): the forward alone on the same route (bits)."""
    for ci, (kind, clip_ls, clip_a, det, red, taken) in enumerate(CONFIGS):
        seed, step, row_offset = 1000 + ci, (2 ** 32 + ci if ci % 3 == 0 else ci), (32768 if ci % 2 else 0)
        ls = R.nan_head(_ls(kind, a))
        mean, act, lp = R.Canary(m, a, DEV), R.Canary(m, a, DEV, offset=3), R.Canary(m, a if red is None else 1, DEV, offset=2)
        tk = R.trapped_input(torch.rand(m, a, device=DEV) * 2 - 1, 3) if taken else None
        head = dict(clip_log_std=clip_ls, clip_actions=clip_a, deterministic=det, reduction=red, taken_actions=tk, seed=seed, step=step,
                    row_offset=row_offset, low=-1.0, high=1.0)
        run(mean.y, ls, act.y, lp.y, **head)
        torch.cuda.synchronize()
        tag = f"{label} cfg{ci} {kind} clip_ls={clip_ls} clip_a={clip_a} det={det} red={red} taken={taken}"
        assert mean.intact() and act.intact() and lp.intact(), f"{tag}: a write outside an output slice"
        if want_mean is not None:
            R.check(mean.y, want_mean, bound_mean, tag + " mean")
        assert torch.equal(_bits(mean.y), _bits(mean_of())), f"{tag}: mean differs from the forward's"
        ls_c = G.clipped_log_std(ls, clip_ls)
        eps = eng.policy_noise(m, a, seed=seed, step=step, row_offset=row_offset)
        want_a, bound_a = G.actions_reference(mean.y, ls_c, eps, clip_a, -1.0, 1.0, det)
        _check(act.y, want_a, bound_a, tag + " actions")
        if det:
            assert torch.equal(_bits(act.y), _bits(mean.y)) or clip_a
        if clip_a:
            assert float(act.y.min()) >= -1.0 and float(act.y.max()) <= 1.0
        x = tk if taken else act.y
        want_lp, bound_lp = G.log_prob_reference(mean.y, ls_c, x, red)
        _check(lp.y, want_lp, bound_lp, tag + " log_prob")


FUSED = [(m, a, route) for a in (1, 2, 3, 4) for m, route in ((63, "mlp_small+gauss"), (20479, "mlp_small+gauss"),
                                                              (20480, "chain16<16,10,8,1>+gauss"), (20480 + 77, "chain16<16,10,8,1>+gauss"))]
FUSED = [c for i, c in enumerate(FUSED) if c[0] in (63, 20480 + 77) or c[1] == 2]          # both batch edges for the rover's A = 2
SEPARATE = [(63, 124, (256, 160, 128, 5), "mlp_small;gauss"), (20480, 124, (256, 160, 128, 16), "chain16<16,10,8,1>;gauss"),
            (513, 634, (80, 5), "splitk<5,1>;gauss"), (20480, 33, (96, 16), "chain16<6,4,0,0>;gauss")]


@pytest.mark.parametrize("case", FUSED, ids=lambda c: f"{c[0]}-A{c[1]}")
def test_fused_head_routes(eng, case):
    m, a, route = case
    widths, acts = (256, 160, 128, a), HID + ("tanh",)
    assert eng.chain_act_route(m, 124, widths, acts) == route
    x, layers, want, bound = R.sensitive_data(m, 124, widths, acts, m + a, DEV)
    x, layers = R.trapped_input(x, 1), R.trapped_layers(layers)
    fwd = torch.empty(m, a, device=DEV)
    _head_case(eng, lambda mean, ls, act, lp, **h: eng.chain_act(x, layers, mean, ls, act, lp, **h),
               lambda: eng.chain_forward(x, layers, fwd), m, a, route, want, bound)


@pytest.mark.parametrize("case", SEPARATE, ids=lambda c: c[3])
def test_head_as_its_own_launch_after_a_chain(eng, case):
    m, k0, widths, route = case
    acts = (HID + ("tanh",)) if len(widths) == 4 else ("leakyrelu", "tanh")
    assert eng.chain_act_route(m, k0, widths, acts) == route
    x, layers, want, bound = R.sensitive_data(m, k0, widths, acts, m, DEV)
    x, layers = R.trapped_input(x, 1), R.trapped_layers(layers)
    fwd = torch.empty(m, widths[-1], device=DEV)
    _head_case(eng, lambda mean, ls, act, lp, **h: eng.chain_act(x, layers, mean, ls, act, lp, **h),
               lambda: eng.chain_forward(x, layers, fwd), m, widths[-1], route, want, bound)


@pytest.mark.parametrize("a", [1, 2, 5, 16])
def test_per_layer_forward_then_standalone_head(eng, a):
    """A chain outside the built tile shapes: rover_mlp_chain_act refuses it, the layers run one by one, then rover_gaussian_head."""
    m, widths, acts = 777, (256, 200, 128, a), HID + ("tanh",)
    assert eng.chain_act_route(m, 124, widths, acts) is None
    x, layers, want, bound = R.sensitive_data(m, 124, widths, acts, a, DEV)
    x, layers = R.trapped_input(x, 1), R.trapped_layers(layers)

    def forward():
        h = x
        for l in layers:
            h = eng.linear_forward(h, l.weight, l.bias, l.activation, torch.empty(m, l.weight.shape[0], device=DEV))
        return h

    def run(mean, ls, act, lp, **head):
        mean.copy_(forward())
        src = R.trapped_input(mean.clone(), 3)
        eng.gaussian_head(src, ls, act, lp, **head)

    _head_case(eng, run, forward, m, a, f"per-layer;gauss A={a}", want, bound)
    from isaac_rover_amd import _lib
    with pytest.raises(_lib.RoverError):
        eng.chain_act(x, layers, torch.empty(m, a, device=DEV), _ls("zero", a), torch.empty(m, a, device=DEV), torch.empty(m, 1, device=DEV))


# ---- the model's act() ----------------------------------------------------------------------------------------------------------------
def _actor(eng, **kw):
    from isaac_rover_amd.learning.model import HeightmapNet
    net = HeightmapNet(eng, NATIVE["num_observations"], NATIVE["num_sparse"], NATIVE["num_dense"], 2, "tanh", seed=11, **kw)
    net.log_std_parameter.copy_(torch.tensor([-0.5, 0.25]))
    return net


def _obs(rows, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(rows, NATIVE["num_observations"], generator=g, device=DEV) * 2 - 1


def test_taken_actions_reproduce_log_prob_and_do_not_advance(eng):
    for reduction in ("sum", None):
        net = _actor(eng, reduction=reduction)
        s = _obs(700)
        c0 = int(net._act_counter)
        a, lp, out = net.act(s)
        assert int(net._act_counter) == c0 + 1 and out["mean_actions"].shape == (700, 2) and lp.shape == (700, 2 if reduction is None else 1)
        a2, lp2, _ = net.act({"states": s, "taken_actions": a}, role="policy")
        torch.cuda.synchronize()
        assert int(net._act_counter) == c0 + 1, "the taken-actions path advanced the counter"
        assert torch.equal(_bits(lp), _bits(lp2))
        assert a2.data_ptr() != a.data_ptr() and lp2.data_ptr() != lp.data_ptr()
        a3, lp3, _ = net.act(s, step=c0)
        assert int(net._act_counter) == c0 + 1 and torch.equal(_bits(a3), _bits(a)) and torch.equal(_bits(lp3), _bits(lp))
        am, lpm, outm = net.act(s, deterministic=True)
        assert torch.equal(_bits(am), _bits(outm["mean_actions"])) and torch.equal(_bits(outm["mean_actions"]), _bits(net.compute(s)))
        ls_c = G.clipped_log_std(net.log_std_parameter)
        np.testing.assert_allclose(net.get_entropy().cpu().double().numpy(), (0.5 + G.HALF_LOG_2PI + ls_c).expand(700, 2).cpu().numpy(), rtol=1e-6)
        assert net.get_log_std().shape == (700, 2) and torch.equal(net.get_log_std()[5].double(), ls_c)


def test_invariance_under_batch_size_sharding_and_route(eng):
    net = _actor(eng)
    s = _obs(65536)
    t = 2 ** 32 + 3
    ls_c = G.clipped_log_std(net.log_std_parameter)
    full_a, full_lp, out = net.act(s, step=t)
    full_mean = out["mean_actions"].clone()
    again_a, again_lp, _ = net.act(s, step=t)
    assert torch.equal(_bits(again_a), _bits(full_a)) and torch.equal(_bits(again_lp), _bits(full_lp))
    next_a, _, _ = net.act(s, step=t + 1)
    assert float((next_a != full_a).any(dim=1).float().mean()) > 0.999
    eps = eng.policy_noise(65536, 2, seed=net.seed, step=t)
    for lo in (0, 32768):                                              # two shards: the same kernel route, their own row_offset
        net.row_offset = lo
        a, lp, o = net.act(s[lo:lo + 32768], step=t)
        assert torch.equal(_bits(eng.policy_noise(32768, 2, seed=net.seed, step=t, row_offset=lo)), _bits(eps[lo:lo + 32768]))
        same = (o["mean_actions"] == full_mean[lo:lo + 32768]).all(dim=1)
        print(f"shard at {lo}: mean bit-identical on {float(same.float().mean()):.4%} of rows")
        assert torch.equal(_bits(a[same]), _bits(full_a[lo:lo + 32768][same])) and torch.equal(_bits(lp[same]), _bits(full_lp[lo:lo + 32768][same]))
        want, bound = G.actions_reference(o["mean_actions"], ls_c, eps[lo:lo + 32768])
        _check(a, want, bound, f"shard at {lo}: actions")
    for lo in (0, 40000):                                              # 512 rows: mlp_small instead of chain16
        net.row_offset = lo
        a, lp, o = net.act(s[lo:lo + 512], step=t)
        torch.cuda.synchronize()
        assert torch.equal(_bits(eng.policy_noise(512, 2, seed=net.seed, step=t, row_offset=lo)), _bits(eps[lo:lo + 512]))
        same = (o["mean_actions"] == full_mean[lo:lo + 512]).all(dim=1)
        assert torch.equal(_bits(a[same]), _bits(full_a[lo:lo + 512][same]))
        want, bound = G.actions_reference(o["mean_actions"], ls_c, eps[lo:lo + 512])
        _check(a, want, bound, f"512 rows at {lo}: actions")
        want, bound = G.log_prob_reference(o["mean_actions"], ls_c, a)
        _check(lp, want, bound, f"512 rows at {lo}: log_prob")


def test_graph_replay_draws_fresh_noise_and_equals_eager(eng):
    net = _actor(eng)
    s = _obs(512)
    net.act(s)                                                         # warm-up: sizes the split-k scratch outside the capture
    torch.cuda.synchronize()
    c0 = int(net._act_counter)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a, lp, out = net.act(s)
    assert int(net._act_counter) == c0, "capturing must not run the increment"
    got = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got.append((a.clone(), lp.clone(), out["mean_actions"].clone()))
    assert int(net._act_counter) == c0 + 3
    for i, (ga, glp, gm) in enumerate(got):
        ea, elp, eo = net.act(s, step=c0 + i)
        assert torch.equal(_bits(ea), _bits(ga)) and torch.equal(_bits(elp), _bits(glp)) and torch.equal(_bits(eo["mean_actions"]), _bits(gm))
    assert not torch.equal(got[0][0], got[1][0]) and not torch.equal(got[1][0], got[2][0]) and not torch.equal(got[0][0], got[2][0])
    ea, _, _ = net.act(s)                                              # an eager call goes on where the replays stopped
    e3, _, _ = net.act(s, step=c0 + 3)
    assert int(net._act_counter) == c0 + 4 and torch.equal(_bits(ea), _bits(e3))


TOL_NET_ABS, TOL_NET_REL = 2e-5, 2e-4      # tests/test_next_rows_gpu.py: f32 MFMA accumulation order vs the reference's nn.Linear on CPU


@pytest.mark.parametrize("name", ["policy_native", "policy_p37"])
def test_act_with_reference_weights(name):
    from isaac_rover_amd import _lib
    from isaac_rover_amd.learning.model import HeightmapNet
    fx = load_golden(name)
    nobs, ns, nd = int(fx["num_observations"]), int(fx["num_sparse"]), int(fx["num_dense"])
    eng = _lib.Engine(8, device=0)
    x = torch.from_numpy(fx["states"].astype(np.float32)).cuda()

    def load(net, tag):
        net.load_state_dict({k[len(tag) + 1:]: torch.from_numpy(v.astype(np.float32)) for k, v in fx.items() if k.startswith(tag + ".")})

    actor = HeightmapNet(eng, nobs, ns, nd, 2, "tanh")
    load(actor, "actor")
    for fused in (True, False):
        a, lp, out = actor.act(x, fused=fused)
        torch.cuda.synchronize()
        np.testing.assert_allclose(out["mean_actions"].cpu().numpy(), fx["out_actor"], atol=TOL_NET_ABS, rtol=TOL_NET_REL)
        ls_c = G.clipped_log_std(actor.log_std_parameter)
        want, bound = G.log_prob_reference(out["mean_actions"], ls_c, a)
        _check(lp, want, bound, f"{name} fused={fused} log_prob")
        assert a.shape == (x.shape[0], 2) and lp.shape == (x.shape[0], 1) and bool(torch.isfinite(a).all())
    if "out_critic" in fx:
        critic = HeightmapNet(eng, nobs, ns, nd, 1, None)
        load(critic, "critic")
        v, none, extra = critic.act({"states": x}, role="value")
        torch.cuda.synchronize()
        assert none is None and extra == {}
        np.testing.assert_allclose(v.cpu().numpy(), fx["out_critic"], atol=TOL_NET_ABS, rtol=TOL_NET_REL)
        clipped = HeightmapNet(eng, nobs, ns, nd, 1, None, clip_actions=True)
        load(clipped, "critic")
        vc, _, _ = clipped.act(x)
        np.testing.assert_array_equal(vc.cpu().numpy(), np.clip(v.cpu().numpy(), -1.0, 1.0))
    eng.close()


def test_rollout_example_with_the_actor():
    """examples/rollout.py --policy actor runs; --policy random (the default) prints what it printed before."""
    base = [sys.executable, os.path.join(ROOT, "examples", "rollout.py"), "--envs", "512", "--steps", "20"]
    out = subprocess.run(base + ["--policy", "actor"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "policy: StochasticActorHeightmap" in out.stdout and "(incl. actor policy + toy pose feeder)" in out.stdout
    assert "20 steps x 512 envs" in out.stdout and "obs (512, " in out.stdout
    out = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("obs (512, ") and "  actions 2  device " in lines[0]
    assert lines[1].startswith("20 steps x 512 envs in ") and "(incl. random policy + toy pose feeder); episodes finished: " in lines[1]
