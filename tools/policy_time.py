"""Time the actor forward (f-4) on the GPU box, one launch per layer vs the fused chain kernels; HIP-event time per forward.

``--act``: compute() and act() side by side on the native 1 750-float obs at 512, 4 096 and 65 536 rows, and the same head written
with torch ops on top of compute() (exp, randn, mul, add, clamp, sub, div, pow, sum, ...) for the record.  Run it under
``rocprofv3 --kernel-trace --stats -- python tools/policy_time.py --act`` for per-kernel medians; ``--no-act`` in
that run times compute() alone (the yardstick, also what the parent commit can run)."""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from isaac_rover_amd import _lib
from isaac_rover_amd.learning.model import HeightmapNet


def timed(fn, reps=50, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter(); a.record()
    for _ in range(reps): fn()
    b.record(); th = (time.perf_counter() - t) / reps
    torch.cuda.synchronize(); dt = (time.perf_counter() - t) / reps
    return a.elapsed_time(b) / reps, dt * 1e3, th * 1e3


def torch_head(net, states):
    """act() as torch ops on compute()'s mean: what the fused epilogue replaces."""
    mean = net.compute(states)
    ls = torch.clamp(net.log_std_parameter, net.min_log_std, net.max_log_std)
    sigma = torch.exp(ls)
    actions = mean + sigma * torch.randn_like(mean)
    lp = (-((actions - mean) / sigma).pow(2) / 2 - ls - 0.5 * math.log(2 * math.pi)).sum(-1, keepdim=True)
    return actions, lp


if "--act" in sys.argv or "--no-act" in sys.argv:
    for e in (512, 4096, 65536):
        eng = _lib.Engine(e, device=0)
        ns, nd = 634, 1112
        w = 4 + ns + nd
        obs = torch.rand(e, w, device="cuda")
        net = HeightmapNet(eng, w, ns, nd, 2, "tanh")
        cases = [("compute", lambda: net.compute(obs))]
        if "--act" in sys.argv:
            cases += [("act", lambda: net.act(obs)), ("act(step=)", lambda: net.act(obs, step=5)), ("compute+torch head", lambda: torch_head(net, obs))]
        for name, fn in cases:
            gpu, wall, host = timed(fn)
            print(f"E={e} obs={w} {name}: gpu {gpu:.4f} ms, wall {wall:.4f} ms, host enqueue {host:.4f} ms")
        eng.close()
    sys.exit(0)

for e, ns, nd in ((4096, 634, 1112), (65536, 634, 1112), (65536, 37, 1)):
    eng = _lib.Engine(e, device=0)
    w = 4 + ns + nd
    obs = torch.rand(e, w, device="cuda")
    net = HeightmapNet(eng, w, ns, nd, 2, "tanh")
    for fused in (False, True):
        for _ in range(3): net.compute(obs, fused=fused)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter(); a.record()
        for _ in range(20): net.compute(obs, fused=fused)
        b.record(); th = (time.perf_counter() - t) / 20
        torch.cuda.synchronize(); dt = (time.perf_counter() - t) / 20
        gpu = a.elapsed_time(b) / 20
        flops = 2 * e * sum(l.weight.numel() for l in net.encoder0 + net.encoder1 + net.network)
        print(f"E={e} obs={w} fused={fused}: gpu {gpu:.3f} ms ({flops / gpu / 1e9:.1f} TFLOP/s f32), wall {dt*1e3:.3f} ms, host enqueue {th*1e3:.3f} ms")
    eng.close()
