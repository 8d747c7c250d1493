#!/usr/bin/env python3
"""Times what a rollout step asks of the policy nets — the actor's act() and the critic's act() on the native 1 750-float obs
(4 + 634 + 1 112) — with precision="bf16" against precision="f32" (the f32 path is the code as it was: split-k / mlp_small below
20 480 rows, chain16 from there on).  One process, one pair of nets per precision holding the same weights; both sides are warmed up,
then `--reps` repetitions of `--inner` calls each, alternating the two, device events around each; median, min, max per side.

    python tools/actor_precision_timing.py [--rows 512 4096 65536] [--reps 10] [--inner 20] [--out out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/actor_precision_timing.py --rows 65536 --reps 2 --inner 5

On a shared machine run every GPU step under its own `timeout` and chain the steps with `&&`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaac_rover_amd import _lib  # noqa: E402
from isaac_rover_amd.learning.model import HeightmapNet  # noqa: E402

NOBS, NS, ND = 1750, 634, 1112
DEV = "cuda:0"


def timed(fn, n):
    """ms per call of ``fn`` over n calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = _lib.Engine(64, device=0)
    nets = {p: (HeightmapNet(eng, NOBS, NS, ND, 2, "tanh", seed=3, precision=p), HeightmapNet(eng, NOBS, NS, ND, 1, None, seed=4, precision=p))
            for p in ("f32", "bf16")}
    med = lambda v: sorted(v)[len(v) // 2]
    res = []
    for rows in a.rows:
        obs = (torch.rand(rows, NOBS, generator=torch.Generator().manual_seed(rows)) * 2 - 1).to(DEV)
        rec = {"rows": rows}
        for who, idx in (("actor", 0), ("critic", 1)):
            calls = {p: (lambda net=nets[p][idx]: net.act(obs)) for p in nets}
            out = {p: calls[p]()[0].clone() for p in nets}                      # warm-up; how far the two precisions are apart
            for p in nets:
                timed(calls[p], 3)
            rec[f"{who}_max_abs_diff"] = float((out["bf16"] - out["f32"]).abs().max()) if who == "critic" else \
                float((nets["bf16"][0].act(obs, deterministic=True)[0] - nets["f32"][0].act(obs, deterministic=True)[0]).abs().max())
            t = {p: [] for p in nets}
            for _ in range(a.reps):
                for p in nets:                                                   # alternating
                    t[p].append(timed(calls[p], a.inner))
            for p in nets:
                rec[f"{who}_{p}_ms"] = {"median": med(t[p]), "min": min(t[p]), "max": max(t[p])}
            rec[f"{who}_bf16_wins"] = max(t["bf16"]) < min(t["f32"])          # the slowest bf16 repetition beats the fastest f32 one
        print(json.dumps(rec), flush=True)
        res.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    eng.close()


if __name__ == "__main__":
    main()
