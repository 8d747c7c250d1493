"""GPU: the native optimiser step (csrc/rover_optim.hip) against the float64 reference and the derived bound of tests/optim_ref.py on a
tensor list that holds every path of the kernels, its determinism, its gate and its refusals; PPO.update with native_step against
float64 autograd + Adam, the device-side KL stop against the host-side one, and a whole minibatch with its gated step in a graph.

Parameters, gradients and the state sit in CANARY-guarded buffers; every step is checked from the GPU's own state before it (so the
bound is the one-step bound), and the observed error / bound ratios are printed."""
import ctypes as C

import pytest
import torch

import optim_ref as O
import ppo_ref as P
from test_ppo_gpu import DEV, Guarded, _bits, _setup_update

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(8, device=0)
    yield e
    e.close()


def _chunk():
    from isaac_rover_amd import _lib
    return _lib.Engine.optim_plan([1 << 20])[0][2]


class Tensors:
    """The test's tensor list with its state, bound to a handle.  In order: one chunk exactly (its state 16-byte aligned), numel 0, 1, 3
    and 5, chunk + 1, 3 chunks + 7, a view that starts 4 bytes into an allocation (chunk + 6 elements: the scalar path, more than one
    chunk), a 2-D weight.  The flat state offsets are 0, c, c, c + 1, c + 4, c + 9, ...: both state paths occur with both tensor paths."""

    def __init__(self, eng, seed):
        c = _chunk()
        self.eng = eng
        self.shapes = [(c,), (0,), (1,), (3,), (5,), (c + 1,), (3 * c + 7,), (c + 6,), (37, 21)]
        gen = torch.Generator().manual_seed(seed)
        self.gen = gen
        self.pb = [Guarded(s if i != 7 else (s[0] + 1,)) for i, s in enumerate(self.shapes)]
        self.gb = [Guarded(s if i != 7 else (s[0] + 1,)) for i, s in enumerate(self.shapes)]
        view = lambda b, i: b.y[1:] if i == 7 else b.y
        self.p = [view(b, i) for i, b in enumerate(self.pb)]
        self.g = [view(b, i) for i, b in enumerate(self.gb)]
        assert self.p[7].data_ptr() % 16 == 4 and self.p[0].data_ptr() % 16 == 0
        for b in self.pb:
            b.y.copy_(torch.randn(b.y.shape, generator=gen) * 0.3)
        total = sum(t.numel() for t in self.p)
        self.mb, self.vb = Guarded((total,)), Guarded((total,))
        self.mb.y.zero_()
        self.vb.y.zero_()
        self.step = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.stopped = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.norm = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
        self.set_grads(1.0)
        self.handle = eng.optim_create(self.p, self.g, self.mb.y, self.vb.y, self.step, self.stopped)

    def set_grads(self, scale):
        """Fresh random gradients of total norm ~ scale."""
        n = sum(t.numel() for t in self.p)
        for b in self.gb:
            b.y.copy_(torch.randn(b.y.shape, generator=self.gen) * (scale / n ** 0.5))

    def split(self, flat):
        out, lo = [], 0
        for t in self.p:
            out.append(flat[lo:lo + t.numel()].view(t.shape))
            lo += t.numel()
        return out

    def snapshot(self):
        torch.cuda.synchronize()
        cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
        return {"p": cpu(self.p), "m": cpu(self.split(self.mb.y)), "v": cpu(self.split(self.vb.y)), "g": cpu(self.g),
                "step": int(self.step), "stopped": int(self.stopped)}

    def intact(self):
        return all(b.intact() for b in self.pb + self.gb + [self.mb, self.vb])

    def do_step(self, clip, **kw):
        self.eng.optim_step(self.handle, grad_norm_clip=clip, norm_out=self.norm, **HYPER, **kw)

    def close(self):
        self.eng.optim_destroy(self.handle)


def _same(a, b, keys=("p", "m", "v")):
    return all(torch.equal(_bits(x), _bits(y)) for k in keys for x, y in zip(a[k], b[k]))


def _checked_step(ts, clip, worst):
    """One step, checked against the float64 reference from the state before it -> the state after it."""
    before = ts.snapshot()
    ts.do_step(clip)
    after = ts.snapshot()
    t = before["step"] + 1
    assert after["step"] == t and after["stopped"] == 0 and ts.intact()
    assert _same(before, after, keys=("g",))                                   # gradients are read only
    Pw, Mw, Vw, norm, coef = O.step64(before["p"], before["m"], before["v"], before["g"], t, clip=clip, **HYPER)
    assert abs(float(ts.norm) - norm) <= 1e-12 * norm
    B = O.bounds(before["p"], before["m"], before["v"], before["g"], t, clip=clip, **HYPER)
    for name, want, bound in zip("pmv", (Pw, Mw, Vw), B):
        for i, (w, b, x) in enumerate(zip(want, bound, after[name])):
            if x.numel():
                ratio = float(((x.double() - w).abs() / b).max())
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert ratio <= 1.0, (name, i, t, ratio)
        if name == "p":                                                        # the step did something: no parameter tensor is unchanged
            assert all(not torch.equal(x, y) for x, y in zip(after["p"], before["p"]) if x.numel())
    return coef


@pytest.mark.parametrize("case", ["clip_active", "clip_inactive", "clip_zero", "clip_negative"])
def test_one_step_against_float64(eng, case):
    ts = Tensors(eng, seed=3)
    ts.set_grads({"clip_active": 4.0, "clip_inactive": 0.25}.get(case, 4.0))
    worst = {}
    coef = _checked_step(ts, {"clip_active": 1.0, "clip_inactive": 1.0, "clip_zero": 0.0, "clip_negative": -1.0}[case], worst)
    assert (coef < 0.5) if case == "clip_active" else coef == 1.0
    print(f"{case}: error / bound {worst}")
    ts.close()


def test_five_steps_follow_the_device_counter(eng):
    ts, worst, active = Tensors(eng, seed=4), {}, []
    for scale in (3.0, 1e-3, 2.0, 0.3, 1.5):
        ts.set_grads(scale)
        active.append(_checked_step(ts, 1.0, worst) < 1.0)
    assert active == [True, False, True, False, True] and int(ts.step) == 5
    print(f"five steps: error / bound {worst}")
    ts.close()


def _five(eng, seed):
    ts = Tensors(eng, seed)
    for scale in (3.0, 1e-3, 2.0, 0.3, 1.5):
        ts.set_grads(scale)
        ts.do_step(1.0)
    out = ts.snapshot()
    ts.close()
    return out


def test_two_fresh_runs_are_bit_equal(eng):
    a, b = _five(eng, 5), _five(eng, 5)
    assert a["step"] == b["step"] == 5 and _same(a, b)


def test_gate(eng):
    ts = Tensors(eng, seed=6)
    gate = torch.tensor([0.02], dtype=torch.float64, device=DEV)
    ts.do_step(1.0)                                                            # some state to preserve
    s0 = ts.snapshot()
    ts.norm.fill_(-1.0)
    ts.do_step(1.0, gate=gate, gate_threshold=0.01)                            # above the threshold: stops
    s1 = ts.snapshot()
    assert _same(s0, s1) and s1["step"] == s0["step"] == 1 and s1["stopped"] == 1 and float(ts.norm) == -1.0
    gate.fill_(0.0)
    ts.do_step(1.0, gate=gate, gate_threshold=0.01)                            # a passing gate, but the latch is set
    s2 = ts.snapshot()
    assert _same(s0, s2) and s2["step"] == 1 and s2["stopped"] == 1
    ts.do_step(1.0)                                                            # ... and no gate at all
    assert _same(s0, ts.snapshot()) and int(ts.step) == 1
    ts.stopped.zero_()
    worst = {}
    _checked_step(ts, 1.0, worst)                                              # steps again, the counter advanced by exactly one
    assert int(ts.step) == 2
    gate.fill_(0.01)
    ts.do_step(1.0, gate=gate, gate_threshold=0.01)                            # equal to the threshold: a plain >, steps
    assert int(ts.step) == 3 and int(ts.stopped) == 0
    gate.fill_(float("nan"))
    s3 = ts.snapshot()
    ts.do_step(1.0, gate=gate, gate_threshold=0.01)                            # a NaN gate steps
    s4 = ts.snapshot()
    assert s4["step"] == 4 and s4["stopped"] == 0 and not _same(s3, s4, keys=("p",)) and ts.intact()
    ts.close()


def test_refusals_before_any_launch(eng):
    from isaac_rover_amd import _lib as L
    ts = Tensors(eng, seed=7)
    ts.do_step(1.0)
    s0 = ts.snapshot()
    lib, h = eng.lib, eng._h
    f32 = lambda n: torch.zeros(n, device=DEV)
    a, b, ga, gb, m, v = f32(8), f32(8), f32(8), f32(8), f32(16), f32(16)
    step, stopped = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    wide = torch.zeros(4, dtype=torch.int64, device=DEV)                       # 32 bytes that can stand in for step / stopped

    def create(params=(a, b), grads=(ga, gb), numel=(8, 8), exp_avg=m, exp_avg_sq=v, step_=step, stopped_=stopped, n=None, desc=True, out=True):
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        k = len(numel)
        pa = (C.c_void_p * max(k, 1))(*[ptr(t) for t in params])
        ga_ = (C.c_void_p * max(k, 1))(*[ptr(t) for t in grads])
        na = (C.c_int64 * max(k, 1))(*numel)
        d = L.OptimDesc(k if n is None else n, C.cast(pa, C.c_void_p), C.cast(ga_, C.c_void_p), C.cast(na, C.c_void_p), ptr(exp_avg), ptr(exp_avg_sq),
                        ptr(step_), ptr(stopped_))
        hd = C.c_int32(-5)
        rc = lib.rover_optim_create(h, C.byref(d) if desc else None, C.byref(hd) if out else None)
        assert rc != 0 or hd.value >= 0
        return rc, hd.value

    rc, ok = create()
    assert rc == 0
    assert lib.rover_optim_destroy(h, ok) == 0 and lib.rover_optim_destroy(h, ok) == -1        # destroyed twice
    assert lib.rover_optim_destroy(h, -1) == -1 and lib.rover_optim_destroy(h, 4096) == -1
    bad = {
        "null descriptor": dict(desc=False), "null handle": dict(out=False), "no tensors": dict(n=0), "257 tensors": dict(n=257),
        "negative numel": dict(numel=(8, -1)), "2^31 elements": dict(numel=(2 ** 30, 2 ** 30)),
        "null param": dict(params=(a, None)), "null grad": dict(grads=(None, gb)), "misaligned param": dict(params=(a.data_ptr() + 2, b)),
        "misaligned grad": dict(grads=(ga, gb.data_ptr() + 1)), "null exp_avg": dict(exp_avg=None), "null exp_avg_sq": dict(exp_avg_sq=None),
        "null step": dict(step_=None), "null stopped": dict(stopped_=None),
        "param is its grad": dict(grads=(a, gb)), "param overlaps the other grad": dict(grads=(ga, a[4:].data_ptr()), numel=(8, 4)),
        "two params overlap": dict(params=(a, a[4:].data_ptr()), numel=(8, 4)), "param in exp_avg": dict(params=(m[8:], b)),
        "param in exp_avg_sq": dict(params=(a, v)), "param on step": dict(params=(a, wide), step_=wide, numel=(8, 2)),
        "param on stopped": dict(params=(a, wide), stopped_=wide, numel=(8, 1)), "grad in exp_avg": dict(grads=(ga, m)),
        "grad on step": dict(grads=(ga, wide), step_=wide, numel=(8, 2)), "exp_avg is exp_avg_sq": dict(exp_avg_sq=m),
        "step on stopped": dict(step_=wide, stopped_=wide), "exp_avg on step": dict(exp_avg=wide.data_ptr(), step_=wide[1:], numel=(2, 2)),
    }
    for name, kw in bad.items():
        rc, _ = create(**kw)
        assert rc == -1, name
        assert eng.lib.rover_last_error(h).decode().startswith("optim_create"), name
    rc, again = create(params=(a, None), grads=(ga, None), numel=(8, 0), exp_avg=m, exp_avg_sq=v)     # a NULL pointer where numel is 0
    assert rc == 0 and again == ok                                             # (the destroyed handle's number is given out again)
    assert lib.rover_optim_destroy(h, again) == 0

    gate, out = torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)

    def step_rc(handle=ts.handle, desc=True, **kw):
        f = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_norm_clip=1.0, gate=None, gate_threshold=0.0, norm_out=None)
        f.update(kw)
        d = L.OptimStepDesc(f["lr"], f["beta1"], f["beta2"], f["eps"], f["grad_norm_clip"], f["gate"], f["gate_threshold"], f["norm_out"])
        return lib.rover_optim_step(h, handle, C.byref(d) if desc else None, None)

    nan, inf = float("nan"), float("inf")
    bad_steps = {
        "null descriptor": dict(desc=False), "dead handle": dict(handle=again), "handle -1": dict(handle=-1), "lr < 0": dict(lr=-1e-3),
        "lr inf": dict(lr=inf), "lr nan": dict(lr=nan), "beta1 = 1": dict(beta1=1.0), "beta1 < 0": dict(beta1=-0.1), "beta2 = 1": dict(beta2=1.0),
        "beta2 nan": dict(beta2=nan), "eps < 0": dict(eps=-1e-8), "eps inf": dict(eps=inf), "clip nan": dict(grad_norm_clip=nan),
        "threshold nan": dict(gate=gate.data_ptr(), gate_threshold=nan), "gate misaligned": dict(gate=gate.data_ptr() + 4),
        "norm_out misaligned": dict(norm_out=out.data_ptr() + 4), "norm_out is gate": dict(gate=gate.data_ptr(), norm_out=gate.data_ptr()),
        "norm_out in a param": dict(norm_out=ts.p[0].data_ptr()), "norm_out in a grad": dict(norm_out=ts.g[6].data_ptr() + 8),
        "norm_out in exp_avg": dict(norm_out=ts.mb.y.data_ptr() + 16), "norm_out in exp_avg_sq": dict(norm_out=ts.vb.y.data_ptr()),
        "norm_out on step": dict(norm_out=ts.step.data_ptr()),
    }
    for name, kw in bad_steps.items():
        assert step_rc(**kw) == -1, name
        assert eng.lib.rover_last_error(h).decode().startswith("optim_step"), name
    with pytest.raises(L.RoverError):
        eng.optim_step(ts.handle, 1e-3, gate=torch.zeros(1, device=DEV))       # the binding's own check: a float32 gate
    with pytest.raises(L.RoverError):
        eng.optim_create(ts.p, ts.g[:-1], ts.mb.y, ts.vb.y, ts.step, ts.stopped)
    s1 = ts.snapshot()                                                         # nothing ran: state, counter and latch as they were
    assert _same(s0, s1) and s1["step"] == s0["step"] and s1["stopped"] == 0 and ts.intact()
    _checked_step(ts, 1.0, {})                                                 # and the live handle still works
    ts.close()


# ---- PPO.update ----------------------------------------------------------------------------------------------------------------------
def _ppo(eng, kl_threshold, **kw):
    from isaac_rover_amd.learning.ppo import PPO
    base, mem, last = _setup_update(eng, kl_threshold)
    return PPO(eng, base.policy, base.value, mem, base.cfg, generator=torch.Generator().manual_seed(11), **kw), mem, last


def test_ppo_update_native_step_matches_float64_autograd(eng):
    """test_ppo_update_matches_float64_autograd's recipe and limit, with the native optimiser step."""
    from isaac_rover_amd.learning import ppo as ppo_mod
    ppo, mem, last = _ppo(eng, 0.0, native_step=True)
    sds = [{k: v.detach().cpu().clone() for k, v in n.state_dict().items()} for n in (ppo.policy, ppo.value)]
    out = ppo.update(last)
    torch.cuda.synchronize()
    assert ppo.minibatches_done == [2, 2] and all(bool(torch.isfinite(v)) for v in out.values()) and int(ppo.optimizer.steps) == 4
    ref = [P.TorchNet(sd, torch.float64) for sd in sds]
    params = [p for n in ref for p in n.p.values()]
    opt = torch.optim.Adam(params, lr=ppo.cfg["learning_rate"])
    gen = torch.Generator().manual_seed(11)
    cpu = {k: mem.get_tensor_by_name(k, keepdim=False).cpu() for k in ppo_mod.NAMES}
    n = cpu["states"].shape[0]
    for _ in range(2):
        perm = torch.randperm(n, generator=gen)
        for i in range(2):
            idx = perm[i * (n // 2):(i + 1) * (n // 2)]
            b = {k: v[idx].double() for k, v in cpu.items()}
            D = {"actions": b["actions"], "old_log_prob": b["log_prob"][:, 0], "advantages": b["advantages"][:, 0], "old_values": b["values"][:, 0],
                 "returns": b["returns"][:, 0]}
            opt.zero_grad()
            mean, _ = ref[0].forward(b["states"])
            value, _ = ref[1].forward(b["states"])
            pol, val, ent, _ = P.ppo_loss_expr(mean, ref[0].p["log_std_parameter"], value[:, 0], D, dict(P.PPO_CFG))
            (pol + val + ent).backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
    worst = 0.0
    for net, r in zip((ppo.policy, ppo.value), ref):
        for k, v in net.state_dict().items():
            if v.numel():
                worst = max(worst, float((v.cpu().double() - r.p[k].detach()).abs().max()))
    print(f"PPO.update (native step) vs float64 autograd + Adam: max parameter difference {worst:.3e}")
    assert worst <= 1e-5
    ppo2, _, last2 = _ppo(eng, 0.0, native_step=True)
    ppo2.update(last2)
    torch.cuda.synchronize()
    for a, b in zip(ppo.params, ppo2.params):
        assert torch.equal(_bits(a), _bits(b))
    # the optimiser's state in torch's layout: a torch Adam over the same parameters takes it
    sd = ppo.optimizer.state_dict()
    torch.optim.Adam(ppo.params, lr=1.0).load_state_dict(sd)
    assert float(sd["state"][0]["step"]) == 4.0


def test_device_kl_stop_matches_host_kl_stop(eng):
    host, _, last_h = _ppo(eng, 1e-9, native_step=True, kl_stop="host")
    host.update(last_h)
    dev, _, last_d = _ppo(eng, 1e-9, native_step=True, kl_stop="device")
    out = dev.update(last_d)
    torch.cuda.synchronize()
    # minibatch 1 of epoch 1 sees the rollout's own policy (KL exactly 0) and steps; every later one sees a changed policy
    assert host.minibatches_done == [1, 0] and dev.minibatches_done == [1, 0], (host.minibatches_done, dev.minibatches_done)
    assert int(dev.optimizer.steps) == 1 and int(dev.optimizer.stopped) == 1
    for a, b in zip(host.params, dev.params):
        assert torch.equal(_bits(a), _bits(b))
    assert all(float(v) == 0.0 for v in out.values())                          # the last epoch stepped nothing: sums of nothing


def test_minibatch_with_gated_step_captured_in_a_graph(eng):
    from isaac_rover_amd.learning import ppo as ppo_mod
    from isaac_rover_amd.learning.rollout import compute_gae

    def prepare():
        ppo, mem, last = _ppo(eng, 0.0, native_step=True)
        compute_gae(eng, mem, last)
        batch = [t.clone() for t in mem.sample_all(ppo_mod.NAMES, 2)[0]]

        def run():
            stats = ppo.minibatch(*batch)
            ppo.backward(batch[0].shape[0], 2)
            ppo.step(gate=stats[3:], gate_threshold=1e9)
        run()                                                                  # warm-up: buffers, .grad tensors and the scratch exist
        torch.cuda.synchronize()
        return ppo, run

    eager, run_eager = prepare()
    run_eager()
    run_eager()
    torch.cuda.synchronize()
    ppo, run = prepare()
    assert int(ppo.optimizer.steps) == 1
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert int(ppo.optimizer.steps) == 1                                       # capturing ran nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(ppo.optimizer.steps) == 3 and int(eager.optimizer.steps) == 3 and int(ppo.optimizer.stopped) == 0
    for a, b in zip(ppo.params, eager.params):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(ppo.optimizer.exp_avg), _bits(eager.optimizer.exp_avg))
