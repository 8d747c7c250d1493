#!/usr/bin/env python3
"""Times the running standard scaler (rover_scaler_update / rover_scaler_apply through learning/preprocess.py) on the GPU against a torch
restatement of skrl's RunningStandardScaler on the same tensors and against a plain copy of the same bytes (EXPERIMENTS.md §25).

    python tools/scaler_timing.py [--rows 512 4096 65536] [--cols 1750] [--value-rows 30720 245760 3932160] [--reps 20] [--json out.json]

Per shape ([rows, cols] states and [rows, 1] values): train + forward, forward alone and inverse, each in HIP (in place and out of place)
and in torch (out of place, as skrl writes it: float64 statistics, float32 normalisation), and out.copy_(x), the traffic floor of a
forward.  Every figure is device-event time per call: median (min .. max) over --reps windows, the HIP and the torch form alternating
inside one process, each window long enough to dwarf the events' own cost.  A train call reads the batch once more than a forward, so
its floor is 1.5 copies.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from isaac_rover_amd import _lib  # noqa: E402
from isaac_rover_amd.learning.preprocess import RunningStandardScaler  # noqa: E402


class TorchScaler:
    """skrl's RunningStandardScaler, restated in torch ops (skrl is not installed): what a user would run without the kernels."""

    def __init__(self, size, device, epsilon=1e-8, clip_threshold=5.0):
        self.epsilon, self.clip = epsilon, clip_threshold
        self.running_mean = torch.zeros(size, dtype=torch.float64, device=device)
        self.running_variance = torch.ones(size, dtype=torch.float64, device=device)
        self.current_count = torch.ones((), dtype=torch.float64, device=device)

    def train(self, x):
        x = x.reshape(-1, x.shape[-1])
        mean, var, n = torch.mean(x, dim=0), torch.var(x, dim=0), x.shape[0]
        delta = mean - self.running_mean
        total = self.current_count + n
        m2 = self.running_variance * self.current_count + var * n + delta ** 2 * self.current_count * n / total
        self.running_mean = self.running_mean + delta * n / total
        self.running_variance = m2 / total
        self.current_count = total

    def __call__(self, x, train=False, inverse=False):
        if train:
            self.train(x)
        if inverse:
            return torch.sqrt(self.running_variance.float()) * torch.clamp(x, -self.clip, self.clip) + self.running_mean.float()
        return torch.clamp((x - self.running_mean.float()) / (torch.sqrt(self.running_variance.float()) + self.epsilon), -self.clip, self.clip)


def timed_pair(fns, reps, inner):
    """{name: (median, min, max)} microseconds per call: ``reps`` rounds, every round one event-bracketed window of ``inner`` calls per
    function, the functions alternating."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--cols", type=int, default=1750)
    ap.add_argument("--value-rows", type=int, nargs="+", default=[60 * 512, 60 * 4096, 60 * 65536], help="T x E rows of the [T E, 1] value shapes")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scaler_timing: needs a GPU")
    dev = torch.device("cuda", 0)
    eng = _lib.Engine(64, device=0)
    result = {"version": _lib.version(), "shapes": {}}
    for m, n in [(m, args.cols) for m in args.rows] + [(m, 1) for m in args.value_rows]:
        inner = max(4, min(200, (1 << 25) // (m * n)))                 # calls per event pair: a window of a millisecond or more
        x = torch.randn(m, n, device=dev) * 3.0 + 1.0
        out, work = torch.empty_like(x), x.clone()
        hip, ref = RunningStandardScaler(eng, n), TorchScaler(n, dev)
        hip(x, train=True, out=out)                                    # the scratch has its size; both hold real statistics
        ref(x, train=True)
        plan = _lib.scaler_plan(m, n)
        fns = {
            "copy": lambda: out.copy_(x),
            "hip_train_forward": lambda: hip(x, train=True, out=out), "torch_train_forward": lambda: ref(x, train=True),
            "hip_train_forward_in_place": lambda: hip(work, train=True, out=work),
            "hip_forward": lambda: hip(x, out=out), "torch_forward": lambda: ref(x),
            "hip_forward_in_place": lambda: hip(work, out=work),
            "hip_inverse": lambda: hip(x, inverse=True, out=out), "torch_inverse": lambda: ref(x, inverse=True),
        }
        rec = timed_pair(fns, args.reps, inner)
        moved = 2 * 4 * m * n
        result["shapes"][f"{m}x{n}"] = dict(rec, inner=inner, bytes_moved_by_a_forward=moved, plan=plan)
        print(f"--- {m} x {n}  plan {plan}  (us per call: median (min .. max); {inner} calls per window, {args.reps} windows)")
        for k, (med, lo, hi) in rec.items():
            extra = ""
            if k.startswith("hip_"):
                floor = rec["copy"][0] * (1.5 if "train" in k else 1.0)
                peer = rec.get(k.replace("hip_", "torch_").replace("_in_place", ""))
                extra = f"   {floor / med:6.1%} of its copy floor" + (f", torch / hip {peer[0] / med:5.2f}x" if peer else "")
            print(f"{k:30s} {med:10.2f} ({lo:.2f} .. {hi:.2f}){extra}")
        del x, out, work
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
