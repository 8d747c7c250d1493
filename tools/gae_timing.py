#!/usr/bin/env python3
"""Times Engine.gae (rover_gae: the scan + the finishing kernel) against the torch loop a user writes without it — the literal
transcription of the definition in tests/test_rollout_host.py, seven elementwise launches per time step, about 430 at T = 60 — on the same device, with
device events: warm-up, then `--reps` repetitions each, alternating the two; median and spread (min, 10th / 90th percentile).

    python tools/gae_timing.py [--reps 200] [--shapes 60x512,60x4096,60x65536] [--json out.json]

Also prints the traffic model (bytes the two passes must move: 9 read + 8 written per element in the scan, 4 + 4 in the normalisation)
over the measured time, as GB/s — an achieved rate to hold against the part's HBM bandwidth, not a share of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in ev])          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--shapes", default="60x512,60x4096,60x65536")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gae_timing needs a GPU (a CPU run says nothing about it)"
    from isaac_rover_amd import _lib
    from test_rollout_host import torch_loop
    import gae_ref as G
    eng = _lib.Engine(64, device=0)
    rows = []
    for shape in args.shapes.split(","):
        T, E = (int(x) for x in shape.split("x"))
        r, v, d, lv = (torch.from_numpy(a).cuda() for a in G.make_case(T, E, "random", seed=1))
        ret, adv = torch.empty_like(r), torch.empty_like(r)
        kernel = lambda: eng.gae(r, v, d, lv, ret, adv, 0.99, 0.95, True)
        raw = lambda: eng.gae(r, v, d, lv, ret, adv, 0.99, 0.95, False)
        loop = lambda: torch_loop(r, v, d, lv, 0.99, 0.95, True)
        for fn in (kernel, raw, loop):                                   # warm-up: code objects, allocator
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ret_l, adv_l = loop()
        kernel()
        torch.cuda.synchronize()
        err = float((adv - adv_l).abs().max()), float((ret - ret_l).abs().max())
        t = {"kernel": [], "raw": [], "loop": []}
        chunk = max(args.reps // 4, 1)
        for _ in range(4):                                               # alternate, so that drift hits all alike
            t["kernel"].append(timed(kernel, chunk))
            t["raw"].append(timed(raw, chunk))
            t["loop"].append(timed(loop, max(chunk // 4, 3)))
        row = {"T": T, "E": E, "max_abs_diff_advantages": err[0], "max_abs_diff_returns": err[1]}
        for k, v_ in t.items():
            a = np.concatenate(v_)
            row[k] = {"median_us": float(np.median(a)), "min_us": float(a.min()), "p10_us": float(np.percentile(a, 10)),
                      "p90_us": float(np.percentile(a, 90)), "n": int(a.size)}
        model_bytes = T * E * 25 + 4 * E
        row["model_bytes"] = model_bytes
        row["kernel_GBps"] = model_bytes / row["kernel"]["median_us"] * 1e-3
        row["speedup_vs_loop"] = row["loop"]["median_us"] / row["kernel"]["median_us"]
        rows.append(row)
        print(f"T={T} E={E}: gae normalised {row['kernel']['median_us']:.1f} us (p10 {row['kernel']['p10_us']:.1f}, p90 {row['kernel']['p90_us']:.1f}; "
              f"2 launches), raw {row['raw']['median_us']:.1f} us (1 launch), torch loop {row['loop']['median_us']:.1f} us "
              f"(p10 {row['loop']['p10_us']:.1f}, p90 {row['loop']['p90_us']:.1f}); x{row['speedup_vs_loop']:.0f}; model {model_bytes / 1e6:.2f} MB "
              f"-> {row['kernel_GBps']:.0f} GB/s; max |d| vs loop: advantages {err[0]:.2e}, returns {err[1]:.2e}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
