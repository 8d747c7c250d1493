#!/usr/bin/env python3
"""Times rover_obs_noise on the GPU against the torch formulation of the same sensor model and against a plain copy (EXPERIMENTS.md §21).

    python tools/obs_noise_timing.py [--rows 65536 512] [--cols 1750] [--reps 30] [--json out.json]

Per size: the kernel out of place and in place with (a) all three components, (b) sigma_point only, (c) dropout only; the same three in
torch (randn_like, rand_like < p, where, the per-env offset by indexing) writing into a given output; out.copy_(in), the traffic floor.
Every figure is device-event time per call: median (min .. max) over --reps windows, each window long enough to dwarf the events' own
cost; the kernel's share of the copy's bandwidth is copy time / kernel time (both move M F floats in and out).  Then the peak device
memory of a distillation window fill [E, T, F] (examples/distill.py) with torch.randn and with HeightmapNoise.  Needs a GPU; there is no
fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from isaac_rover_amd import _lib  # noqa: E402
from isaac_rover_amd.learning.noise import HeightmapNoise  # noqa: E402

FIRST = 4
CONFIGS = {"a_all": dict(sigma_point=0.05, sigma_offset=0.02, dropout=0.1), "b_point": dict(sigma_point=0.05), "c_dropout": dict(dropout=0.1)}


def timed(fn, reps, inner):
    """-> (median, min, max) microseconds per call of fn over ``reps`` event-bracketed windows of ``inner`` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(out), min(out), max(out)


def torch_model(x, out, sigma_point=0.0, sigma_offset=0.0, dropout=0.0, offsets=None, episode=None):
    """The same model in torch ops on the same tensors: per-element noise, the per-env offset by indexing, dropout by where."""
    h = x[:, FIRST:]
    v = h
    if sigma_offset:
        v = v + sigma_offset * offsets[episode].unsqueeze(1)
    if sigma_point:
        v = v + sigma_point * torch.randn_like(h)
    if dropout:
        v = torch.where(torch.rand_like(h) < dropout, 0.0, v)
    out[:, FIRST:] = v
    if out.data_ptr() != x.data_ptr():
        out[:, :FIRST] = x[:, :FIRST]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 512])
    ap.add_argument("--cols", type=int, default=1750)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window-envs", type=int, default=16384, help="E of the window-fill memory comparison (0 = skip)")
    ap.add_argument("--window-steps", type=int, default=32)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("obs_noise_timing: needs a GPU")
    dev = torch.device("cuda", 0)
    eng = _lib.Engine(64, device=0)
    result = {"version": _lib.version(), "cols": args.cols, "first": FIRST, "sizes": {}}
    for m in args.rows:
        f = args.cols
        inner = max(8, min(200, (1 << 24) // (m * f)))                 # calls per event pair: a window of a millisecond or more
        x, out = torch.randn(m, f, device=dev), torch.empty(m, f, device=dev)
        episode = torch.zeros(m, dtype=torch.int64, device=dev)
        offsets = torch.randn(8, device=dev)
        rec = {"inner": inner, "bytes_moved": 2 * 4 * m * f}
        rec["copy"] = timed(lambda: out.copy_(x), args.reps, inner)
        for name, cfg in CONFIGS.items():
            rec[f"hip_{name}_out_of_place"] = timed(lambda: eng.obs_noise(x, out, first=FIRST, episode=episode, seed=1, **cfg), args.reps, inner)
            rec[f"hip_{name}_in_place"] = timed(lambda: eng.obs_noise(out, out, first=FIRST, episode=episode, seed=1, **cfg), args.reps, inner)
            rec[f"torch_{name}_out_of_place"] = timed(lambda: torch_model(x, out, offsets=offsets, episode=episode, **cfg), args.reps, inner)
            rec[f"torch_{name}_in_place"] = timed(lambda: torch_model(out, out, offsets=offsets, episode=episode, **cfg), args.reps, inner)
        result["sizes"][str(m)] = rec
        print(f"--- {m} x {f} (us per call: median (min .. max); {inner} calls per window, {args.reps} windows)")
        for k, (med, lo, hi) in ((k, v) for k, v in rec.items() if isinstance(v, tuple)):
            extra = "" if not k.startswith("hip_") else f"   {rec['copy'][0] / med:6.1%} of the copy's bandwidth, {rec['bytes_moved'] / med / 1e6:7.3f} TB/s"
            print(f"{k:32s} {med:10.2f} ({lo:.2f} .. {hi:.2f}){extra}")
        del x, out
    if args.window_envs:
        e, t_len, f, ex = args.window_envs, args.window_steps, args.cols, args.cols - FIRST
        obs = torch.randn(e, f, device=dev)
        info = {"proprioceptive": FIRST, "sparse": ex, "dense": 0, "actions": 2}
        peaks = {}
        for mode in ("torch_randn", "device_noise"):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            win = torch.empty(e, t_len, f, device=dev)
            if mode == "torch_randn":
                for t in range(t_len):
                    win[:, t] = obs
                win[:, :, f - ex:] += 0.05 * torch.randn(e, t_len, ex, device=dev)
            else:
                noise = HeightmapNoise(eng, info, sigma_point=0.05, seed=2)
                for t in range(t_len):
                    noise.apply(obs, out=win[:, t])
            torch.cuda.synchronize()
            peaks[mode] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
            del win
        result["window_fill_peak_gib"] = dict(peaks, envs=e, steps=t_len, cols=f)
        print(f"--- window fill [{e}, {t_len}, {f}]: peak device memory above the observation: torch.randn {peaks['torch_randn']:.2f} GiB, "
              f"HeightmapNoise {peaks['device_noise']:.2f} GiB")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
