"""CPU: the optimiser step's chunk plan (rover_optim_plan, host only) and its refusals, the float64 reference of tests/optim_ref.py
against clip_grad_norm_ + torch.optim.Adam in float64, the same sequence in float32 torch inside the derived bound, and the Python-side
checks (PPO's kl_stop argument, the Adam state_dict round trip)."""
import ctypes as C
import types

import pytest
import torch

import optim_ref as O


def _lib():
    from isaac_rover_amd import _lib
    return _lib


def _chunk():
    """The library's chunk length, read off the plan of one long tensor."""
    plan = _lib().Engine.optim_plan([1 << 20])
    assert plan[0][:2] == (0, 0) and all(c[2] == plan[0][2] for c in plan)
    return plan[0][2]


def _check_plan(numel):
    chunk = _chunk()
    plan = _lib().Engine.optim_plan(numel)
    want = []                                          # every element of every tensor exactly once, in tensor order then element order
    for t, n in enumerate(numel):
        want += [(t, lo, min(chunk, n - lo)) for lo in range(0, n, chunk)]
    assert plan == want
    pos = {t: 0 for t in range(len(numel))}
    for t, first, length in plan:
        assert first == pos[t] and 1 <= length <= chunk and first % chunk == 0
        pos[t] += length
    assert [pos[t] for t in range(len(numel))] == list(numel)
    return plan


def test_optim_plan_covers_every_element_once_in_order():
    chunk = _chunk()
    assert chunk >= 4 and chunk % 4 == 0
    for numel in ([0], [1], [chunk - 1], [chunk], [chunk + 1], [0, 1, chunk - 1, chunk, chunk + 1, 0, 3 * chunk + 7, 5], [0] * 256,
                  O.native_numel(), [(7 * i) % (2 * chunk + 3) for i in range(256)]):
        _check_plan(numel)
    native = O.native_numel()
    assert len(native) == 33 and sum(native) == 486965
    assert _lib().Engine.optim_plan([0, 0]) == []
    assert len(_check_plan([2 ** 31 - 1 - chunk, chunk])) == -(-(2 ** 31 - 1 - chunk) // chunk) + 1       # one element short of the limit


def test_optim_plan_refusals():
    L = _lib()
    lib = L.load()
    assert "rover_optim_plan" in L.SYMBOLS and all(f"rover_optim_{n}" in L.SYMBOLS for n in ("create", "destroy", "step"))
    for numel in ([], [1] * 257, [5, -1], [2 ** 31], [2 ** 30, 2 ** 30], [2 ** 31 - 1, 1]):
        with pytest.raises(L.RoverError, match=r"rover_optim_plan failed \(-1\)"):
            L.Engine.optim_plan(numel)
    arr, n = (C.c_int64 * 2)(5, 3 * _chunk()), C.c_int64(-7)
    assert lib.rover_optim_plan(2, None, None, 0, C.byref(n)) == -1             # numel NULL
    assert lib.rover_optim_plan(2, arr, None, 0, None) == -1                    # n_chunks NULL
    few = (L.OptimChunk * 3)()
    assert lib.rover_optim_plan(2, arr, few, 3, C.byref(n)) == -1               # 4 chunks do not fit 3 records
    assert lib.rover_optim_plan(2, arr, None, -1, C.byref(n)) == -1
    assert n.value == -7                                                        # a refused call writes nothing
    assert lib.rover_optim_plan(2, arr, None, 0, C.byref(n)) == 0 and n.value == 4


# ---- the reference and the bound ---------------------------------------------------------------------------------------------------
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
CLIP = 1.0
SCALES = (3.0, 1e-3, 2.0, 2e-4, 1.0)                   # of the five steps' gradients (norm ~ 1.46 scale): the clip is active on steps 1, 3, 5 only
SHAPES = ((0,), (1,), (3,), (5,), (64, 33), (1025,), (257,))


def _sequence(dtype):
    """Five steps of clip_grad_norm_ + torch.optim.Adam in ``dtype`` on the CPU -> per step (p, m, v before; the unclipped g; p, m, v
    after), all as float32-exact tensors."""
    gen = torch.Generator().manual_seed(7)
    params = [(torch.randn(*s, generator=gen) * 0.3).to(dtype) for s in SHAPES]
    opt = torch.optim.Adam(params, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"])
    zeros = lambda: [torch.zeros_like(p) for p in params]
    out = []
    for scale in SCALES:
        grads = [(torch.randn(*s, generator=gen) * scale / 40).to(dtype) for s in SHAPES]     # 40 ~ sqrt of the element count
        snap = lambda: ([p.detach().clone() for p in params],
                        [opt.state[p]["exp_avg"].clone() for p in params] if opt.state else zeros(),
                        [opt.state[p]["exp_avg_sq"].clone() for p in params] if opt.state else zeros())
        before = snap()
        for p, g in zip(params, grads):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()
        out.append((before, grads, snap()))
    return out


def test_reference_matches_torch_float64():
    active = []
    for t, (before, g, after) in enumerate(_sequence(torch.float64), start=1):
        P, M, V, norm, coef = O.step64(*before, g, t, clip=CLIP, **HYPER)
        active.append(coef < 1.0)
        for name, mine, ref in (("p", P, after[0]), ("m", M, after[1]), ("v", V, after[2])):
            for a, b in zip(mine, ref):
                scale = float(b.abs().max()) if b.numel() else 0.0
                assert torch.allclose(a, b, rtol=1e-12, atol=1e-12 * scale), (t, name, float((a - b).abs().max()))
    assert active == [True, False, True, False, True]


def test_float32_torch_lies_inside_the_bound():
    n, worst = sum(int(torch.Size(s).numel()) for s in SHAPES), {}
    for t, (before, g, after) in enumerate(_sequence(torch.float32), start=1):
        P, M, V, _, _ = O.step64(*before, g, t, clip=CLIP, **HYPER)
        B = O.bounds(*before, g, t, clip=CLIP, e_norm=O.e_norm_f32(n, len(SHAPES)), **HYPER)
        for name, want, bound, got in zip("pmv", (P, M, V), B, after):
            for w, b, x in zip(want, bound, got):
                if x.numel():
                    ratio = float(((x.double() - w).abs() / b).max())
                    worst[name] = max(worst.get(name, 0.0), ratio)
                    assert ratio <= 1.0, (t, name, ratio)
    print("f32 torch, error / bound:", {k: round(v, 4) for k, v in worst.items()})
    # not vacuous: the bound is a few roundings wide where the clip is off (step 2: e_c = 0), far below the values it bounds
    before, g, _ = _sequence(torch.float32)[1]
    P, M, V, _, _ = O.step64(*before, g, 2, clip=CLIP, **HYPER)
    for want, bound in zip((P, M, V), O.bounds(*before, g, 2, clip=CLIP, **HYPER)):
        for w, b in zip(want, bound):
            if w.numel():
                assert float((b / (w.abs() + 1e-30)).median()) < 64 * O.U


# ---- Python-side validation --------------------------------------------------------------------------------------------------------
def test_ppo_kl_stop_needs_native_step():
    from isaac_rover_amd.learning.ppo import PPO
    mem = types.SimpleNamespace(memory_size=4, num_envs=8)
    with pytest.raises(ValueError, match="native_step"):
        PPO(None, None, None, mem, kl_stop="device")
    with pytest.raises(ValueError, match="kl_stop"):
        PPO(None, None, None, mem, native_step=True, kl_stop="gpu")


def _cpu_params(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen) for s in ((2,), (5, 3), (5,), (4, 0), (7,))]


def test_adam_state_dict_round_trip_is_exact():
    from isaac_rover_amd.learning.optim import Adam
    gen = torch.Generator().manual_seed(1)
    a = Adam(None, _cpu_params(0), lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
    a.exp_avg.copy_(torch.randn(a.exp_avg.shape, generator=gen))
    a.exp_avg_sq.copy_(torch.rand(a.exp_avg_sq.shape, generator=gen))
    a.steps.fill_(17)
    sd = a.state_dict()
    assert [tuple(sd["state"][i]["exp_avg"].shape) for i in range(5)] == [(2,), (5, 3), (5,), (4, 0), (7,)]
    b = Adam(None, _cpu_params(1), lr=1.0)
    b.load_state_dict(sd)
    assert torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq) and int(b.steps) == 17
    assert (b.lr, b.betas, b.eps) == (3e-4, (0.8, 0.99), 1e-7)
    # torch's Adam -> ours -> torch's Adam: the state survives, and torch accepts what state_dict() writes
    params = _cpu_params(2)
    opt = torch.optim.Adam(params, lr=1e-3)
    for k in range(3):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    ours = Adam(None, params, lr=0.5)
    ours.load_state_dict(opt.state_dict())
    assert int(ours.steps) == 3 and ours.lr == 1e-3
    back = torch.optim.Adam(params, lr=0.5)
    back.load_state_dict(ours.state_dict())
    for p in params:
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(back.state[p][key], opt.state[p][key]), key
    assert back.param_groups[0]["lr"] == 1e-3
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen)
    back.step()                                        # the loaded optimiser runs
    with pytest.raises(ValueError):
        Adam(None, params[:2], lr=1.0).load_state_dict(ours.state_dict())
    with pytest.raises(RuntimeError, match="without an engine"):
        ours.step(1.0)
