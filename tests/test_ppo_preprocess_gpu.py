"""GPU: PPO with the running standard scalers and the KL-adaptive learning rate (learning/ppo.py, learning/preprocess.py).  One update at
test_ppo_update_matches_float64_autograd's small shape with both scalers on against a float64 autograd restatement that writes the
scalers out from their definition (tests/scaler_ref.py), under that test's tolerance; the scalers' states under their bound; the stored
values and returns; host against device KL stop, bit for bit, with the stop inside epoch 0; the scheduler over three epochs of hand-set
KLs; and the unchanged default path."""
import copy

import numpy as np
import pytest
import torch

import scaler_ref as R
import test_ppo_gpu as TP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = TP.P
T, E = 4, 64


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    yield e
    e.close()


def _setup(eng, kl_threshold, scalers=True, mini_batches=2, epochs=2, seed=3, old_way=False, **kw):
    """test_ppo_gpu._setup_update's memory and nets, with the rollout as the module docstring of learning/ppo.py prescribes it: both nets
    read preprocess_states(obs), the memory stores denormalize_values(v), last_values is denormalised."""
    from isaac_rover_amd.learning.ppo import PPO
    from isaac_rover_amd.learning.preprocess import RunningStandardScaler
    from isaac_rover_amd.learning.rollout import RolloutMemory
    nets, states64 = TP._nets(eng, "policy_p37")
    (actor, _), (critic, _) = nets
    g = torch.Generator().manual_seed(seed)
    mem = RolloutMemory(T, E, device=DEV)
    obs = states64.shape[1]
    for nm, size, dt in (("states", obs, torch.float32), ("actions", 2, torch.float32), ("log_prob", 1, torch.float32), ("values", 1, torch.float32),
                         ("rewards", 1, torch.float32), ("terminated", 1, torch.bool), ("returns", 1, torch.float32), ("advantages", 1, torch.float32)):
        mem.create_tensor(nm, size, dt)
    cfg = {"learning_epochs": epochs, "mini_batches": mini_batches, "kl_threshold": kl_threshold}
    if old_way:
        ppo = PPO(eng, actor, critic, mem, cfg, torch.Generator().manual_seed(11))
    else:
        if scalers:
            kw = dict(state_preprocessor=RunningStandardScaler(eng, obs), value_preprocessor=RunningStandardScaler(eng, 1), **kw)
        ppo = PPO(eng, actor, critic, mem, cfg, generator=torch.Generator().manual_seed(11), **kw)
    for t in range(T):
        s = (states64[torch.randperm(64, generator=g)] + 0.01 * torch.randn(64, obs, generator=g)).to(DEV)
        a = (torch.rand(E, 2, generator=g) * 2 - 1).to(DEV)
        sp = ppo.preprocess_states(s)
        _, lp, _ = actor.act(sp, taken_actions=a, fused=False)
        v = ppo.denormalize_values(critic.act(sp, fused=False)[0])
        mem.add_samples(states=s, actions=a, log_prob=lp.clone(), values=v.clone(), rewards=torch.rand(E, generator=g).to(DEV),
                        terminated=(torch.rand(E, generator=g) < 0.1).to(DEV))
    last = ppo.denormalize_values((torch.rand(E, generator=g) - 0.5).to(DEV).view(E, 1)).view(E)
    return ppo, mem, last


def _state_of(s):
    return s.running_mean.cpu().numpy(), s.running_variance.cpu().numpy(), float(s.current_count.cpu()[0])


def _within(got, want, bounds, label):
    """The scaler's state against the restatement's after a SEQUENCE of train calls: the capped bounds of the calls add (a fold moves
    the state by a convex combination, so an earlier call's error is never amplified)."""
    b_mean, b_var = sum(b[0] for b in bounds), sum(b[1] for b in bounds)
    e_mean, e_var = np.abs(got[0] - want[0]), np.abs(got[1] - want[1])
    print(f"{label}: worst mean error / bound {float((e_mean / b_mean).max()):.3f}, var {float((e_var / b_var).max()):.3f}")
    assert got[2] == want[2] and np.all(e_mean <= b_mean) and np.all(e_var <= b_var), label


def _step_ref(state, x):
    """One train call of the restatement -> (new state, its capped bound)."""
    from isaac_rover_amd import _lib
    new = R.update(state, x)
    return new, R.capped(*R.update_bound(state, x, _lib.scaler_plan(x.shape[0], x.shape[1])["n_chunks"]), new[0], new[1])


def test_update_with_both_scalers_matches_float64_autograd(eng):
    from isaac_rover_amd.learning import ppo as ppo_mod
    from isaac_rover_amd.learning.rollout import compute_gae
    ppo, mem, last = _setup(eng, 0.0)
    sds = [{k: v.detach().cpu().clone() for k, v in n.state_dict().items()} for n in (ppo.policy, ppo.value)]
    raw = copy.deepcopy(mem)                                                       # the raw returns: the same GAE on a copy of the memory
    compute_gae(eng, raw, last, discount_factor=ppo.cfg["discount_factor"], lambda_coefficient=ppo.cfg["lambda"])
    values_raw, returns_raw = (raw.get_tensor_by_name(k, keepdim=False).cpu().numpy() for k in ("values", "returns"))
    out = ppo.update(last)
    torch.cuda.synchronize()
    assert ppo.minibatches_done == [2, 2] and all(bool(torch.isfinite(v)) for v in out.values())
    # the value scaler: values, then returns — two train calls, each normalised with the statistics that include it
    v1, b1 = _step_ref(R.fresh(1), values_raw)
    v2, b2 = _step_ref(v1, returns_raw)
    _within(_state_of(ppo.value_preprocessor), v2, (b1, b2), "value scaler")
    cpu = {k: mem.get_tensor_by_name(k, keepdim=False).cpu() for k in ppo_mod.NAMES}
    for name, x, st in (("values", values_raw, v1), ("returns", returns_raw, v2)):
        want = R.forward(x, st[0], st[1])
        err = np.abs(cpu[name].numpy() - want)
        assert np.all(err <= 4 * np.spacing(np.maximum(np.abs(want), np.float32(1.0)))), (name, float(err.max()))     # f32 of statistics 1e-13 apart
        assert float(np.abs(cpu[name].numpy() - x).max()) > 1e-3                   # and they ARE the normalised ones
    assert torch.equal(cpu["advantages"], raw.get_tensor_by_name("advantages", keepdim=False).cpu())                  # as GAE left them
    # the same update in float64 autograd + Adam, the state scaler written out: train on every minibatch of epoch 0, then normalise
    ref = [P.TorchNet(sd, torch.float64) for sd in sds]
    params = [p for n in ref for p in n.p.values()]
    opt = torch.optim.Adam(params, lr=ppo.cfg["learning_rate"])
    gen = torch.Generator().manual_seed(11)
    n = cpu["states"].shape[0]
    sstate, sbounds = R.fresh(cpu["states"].shape[1]), []
    for epoch in range(2):
        perm = torch.randperm(n, generator=gen)
        for i in range(2):
            idx = perm[i * (n // 2):(i + 1) * (n // 2)]
            b = {k: v[idx].double() for k, v in cpu.items()}
            xs = cpu["states"][idx].numpy()
            if epoch == 0:
                sstate, bound = _step_ref(sstate, xs)
                sbounds.append(bound)
            states = torch.from_numpy(R.forward(xs, sstate[0], sstate[1])).double()
            D = {"actions": b["actions"], "old_log_prob": b["log_prob"][:, 0], "advantages": b["advantages"][:, 0], "old_values": b["values"][:, 0],
                 "returns": b["returns"][:, 0]}
            opt.zero_grad()
            mean, _ = ref[0].forward(states)
            value, _ = ref[1].forward(states)
            pol, val, ent, _ = P.ppo_loss_expr(mean, ref[0].p["log_std_parameter"], value[:, 0], D, dict(P.PPO_CFG))
            (pol + val + ent).backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
    _within(_state_of(ppo.state_preprocessor), sstate, sbounds, "state scaler")
    assert sstate[2] == 1 + n
    worst = 0.0
    for net, r in zip((ppo.policy, ppo.value), ref):
        for k, v in net.state_dict().items():
            if v.numel():
                worst = max(worst, float((v.cpu().double() - r.p[k].detach()).abs().max()))
    print(f"PPO.update with both scalers vs float64 autograd + Adam: max parameter difference {worst:.3e}")
    assert worst <= 1e-5                                                           # test_ppo_update_matches_float64_autograd's limit
    assert torch.equal(mem.get_tensor_by_name("states"), raw.get_tensor_by_name("states"))       # the memory's states stay raw


def test_host_and_device_kl_stop_agree_bit_for_bit(eng):
    """The stop fires inside epoch 0 with minibatches left after it: those train the state scaler in neither form."""
    probe, _, last = _setup(eng, 0.0, mini_batches=4, epochs=1, native_step=True)
    kls, inner = [], probe.minibatch

    def recording(*batch):
        stats = inner(*batch)
        kls.append(float(stats[3]))
        return stats
    probe.minibatch = recording
    probe.update(last)
    # a minibatch whose KL exceeds every earlier one can be made the first to pass a threshold; one with steps before it where there is one
    fire = next((j for j in (1, 2) if kls[j] > max(kls[:j])), 0)
    print("epoch 0 KLs without a stop:", kls, "-> the stop is put at minibatch", fire)
    threshold = 0.5 * (kls[fire] + max(kls[:fire], default=0.0))
    assert kls[fire] > threshold > 0.0, kls
    runs = {}
    for form in ("host", "device"):
        ppo, _, last = _setup(eng, threshold, mini_batches=4, epochs=2, native_step=True, kl_stop=form)
        ppo.update(last)
        torch.cuda.synchronize()
        runs[form] = ppo
    host, dev = runs["host"], runs["device"]
    assert host.minibatches_done == dev.minibatches_done and host.minibatches_done[0] == fire, (host.minibatches_done, dev.minibatches_done)
    for a, b in zip(host.params, dev.params):
        assert torch.equal(TP._bits(a), TP._bits(b))
    for name in ("state_preprocessor", "value_preprocessor"):
        sa, sb = getattr(host, name), getattr(dev, name)
        for k in ("running_mean", "running_variance", "current_count"):
            assert torch.equal(getattr(sa, k).view(torch.int64), getattr(sb, k).view(torch.int64)), (name, k)
    n = T * E
    assert float(host.state_preprocessor.current_count) == 1 + (fire + 1) * (n // 4)      # the stopping minibatch trained it, the later ones did not


@pytest.mark.parametrize("native", [False, True])
def test_scheduler_follows_the_rule_over_three_epochs(eng, native):
    from isaac_rover_amd.learning.ppo import KLAdaptiveRL
    hand = [[0.02, 0.03], [0.001, 0.002], [0.008, 0.012]]                          # epoch means 0.025 (down), 0.0015 (up), 0.01 (stay)
    ppo, _, last = _setup(eng, 0.0, epochs=3, native_step=native, lr_scheduler=KLAdaptiveRL())
    inner, calls = ppo.minibatch, []

    def hand_set(*batch):
        stats = inner(*batch)
        stats[3] = hand[len(calls) // 2][len(calls) % 2]
        calls.append(1)
        return stats
    ppo.minibatch = hand_set
    lr0 = ppo.cfg["learning_rate"]
    ppo.update(last)
    want, lr = [], lr0
    for e in hand:
        lr = R.kl_adaptive(lr, (e[0] + e[1]) / 2)
        want.append(lr)
    assert want == [lr0 / 1.5, lr0 / 1.5 * 1.5, lr0 / 1.5 * 1.5] and ppo.learning_rates == want and ppo.minibatches_done == [2, 2, 2]
    assert (ppo.optimizer.lr if native else ppo.optimizer.param_groups[0]["lr"]) == want[-1]
    # the minibatch whose KL stops the epoch counts in the epoch's mean: (0.001 + 0.1) / 2 is above the scheduler's 0.016, 0.001 alone is below 0.004
    ppo2, _, last2 = _setup(eng, 0.05, epochs=1, native_step=native, lr_scheduler=KLAdaptiveRL())
    inner2, calls2 = ppo2.minibatch, []

    def stopping(*batch):
        stats = inner2(*batch)
        stats[3] = (0.001, 0.1)[len(calls2)]
        calls2.append(1)
        return stats
    ppo2.minibatch = stopping
    ppo2.update(last2)
    assert ppo2.minibatches_done == [1] and ppo2.learning_rates == [lr0 / 1.5]


def test_default_path_is_unchanged(eng):
    """Without the new arguments: the same parameter bits as a PPO built the way the callers of the previous version build it (positional
    arguments only), and no scaler anywhere."""
    new, _, last = _setup(eng, 0.0, scalers=False)
    old, _, last_old = _setup(eng, 0.0, old_way=True)
    assert new.state_preprocessor is None and new.value_preprocessor is None and new.lr_scheduler is None
    assert torch.equal(last, last_old)
    new.update(last)
    old.update(last_old)
    torch.cuda.synchronize()
    assert new.minibatches_done == old.minibatches_done == [2, 2] and new.learning_rates == []
    for a, b in zip(new.params, old.params):
        assert torch.equal(TP._bits(a), TP._bits(b))
    ref, _, last_ref = TP._setup_update(eng, 0.0)                                  # and as the existing update test sets it up
    ref.update(last_ref)
    torch.cuda.synchronize()
    for a, b in zip(new.params, ref.params):
        assert torch.equal(TP._bits(a), TP._bits(b))


def test_train_example_with_scalers_saves_and_resumes(tmp_path):
    """examples/train.py with both scalers, the scheduler and the native step runs to the end, saves, and a second process resumes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = str(tmp_path / "agent.pt")
    base = [sys.executable, os.path.join(root, "examples", "train.py"), "--envs", "64", "--steps", "20", "--rollouts", "10", "--mini-batches", "4",
            "--kl-threshold", "0", "--state-preprocessor", "--value-preprocessor", "--lr-scheduler", "kl", "--native-step"]      # no early stop: every row trains
    out = subprocess.run(base + ["--save", ck], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "preprocessors: state_preprocessor, value_preprocessor  lr scheduler: KLAdaptiveRL" in out.stdout
    assert "update 2:" in out.stdout and "  lr " in out.stdout and f"saved policy, value and preprocessors to {ck}" in out.stdout
    saved = torch.load(ck, map_location="cpu")
    assert set(saved) == {"policy", "value", "state_preprocessor", "value_preprocessor"}
    for name, rows in (("state_preprocessor", 2 * 10 * 64 // 4 * 4), ("value_preprocessor", 2 * 2 * 10 * 64)):
        sd = saved[name]
        assert set(sd) == {"running_mean", "running_variance", "current_count"} and all(v.dtype == torch.float64 for v in sd.values())
        assert float(sd["current_count"]) == 1 + rows, (name, float(sd["current_count"]))     # every row of both updates trained it once
    out2 = subprocess.run(base + ["--load", ck], capture_output=True, text=True, timeout=120)
    assert out2.returncode == 0, out2.stderr[-2000:]
    assert f"resumed from {ck}: policy, value, state_preprocessor, value_preprocessor" in out2.stdout and "update 2:" in out2.stdout
