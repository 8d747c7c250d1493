#!/usr/bin/env python3
"""Times StudentPolicy.act with precision="bf16" against precision="f32" on the native 1 750-float obs (4 + 634 + 1 112, H = 300): one
process, two policies holding the same weights, each captured in a graph after a warm-up; `--reps` repetitions of `--inner` replays
each, alternating the two, device events around each; median, min, max per side in microseconds per act().  The f32 side is the code
as it was (rover_gru_cell on the f32 MFMA, rover_linear_forward for the gb / ga branches).

    python tools/student_precision_timing.py [--envs 512 4096 16384 65536] [--reps 10] [--inner 20] [--out out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/student_precision_timing.py --envs 65536 --reps 2 --inner 5

`--eager` replays nothing: the calls are made one by one (what a kernel trace should see if graph nodes are not traced).
On a shared machine run every GPU step under its own `timeout` and chain the steps with `&&`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaac_rover_amd import _lib  # noqa: E402
from isaac_rover_amd.learning.student import StudentPolicy  # noqa: E402

INFO = {"proprioceptive": 4, "sparse": 634, "dense": 1112, "actions": 2}      # the reference's native obs row
DEV = "cuda:0"


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def timed(fn, n):
    """microseconds per call of ``fn`` over n calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 4096, 16384, 65536])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "student_precision_timing needs a GPU"
    med = lambda v: sorted(v)[len(v) // 2]
    k0, res = INFO["proprioceptive"] + 120, []
    for e in a.envs:
        eng = _lib.Engine(e, device=0)
        pols = {p: StudentPolicy(eng, INFO, device=DEV, seed=1, precision=p) for p in ("f32", "bf16")}      # the same seed: the same weights
        obs = (torch.rand(e, 1750, generator=torch.Generator().manual_seed(e)) * 2 - 1).to(DEV)
        first = {}
        for p, pol in pols.items():
            pol.init_hidden(e)
            first[p] = pol.act(obs).clone()
        calls = {p: (lambda pol=pol: pol.act(obs)) if a.eager else capture(lambda pol=pol: pol.act(obs)) for p, pol in pols.items()}
        rec = {"envs": e, "routes": {p: eng.gru_cell_route(e, k0, 300, precision=p) for p in pols}, "graph": not a.eager,
               "max_abs_diff_first_step": float((first["bf16"] - first["f32"]).abs().max())}
        t = {p: [] for p in pols}
        for p in pols:
            timed(calls[p], 3)
        for _ in range(a.reps):
            for p in pols:                                                       # alternating
                t[p].append(timed(calls[p], a.inner))
        for p in pols:
            rec[f"{p}_us"] = {"median": med(t[p]), "min": min(t[p]), "max": max(t[p])}
        rec["bf16_wins"] = max(t["bf16"]) < min(t["f32"])                       # the slowest bf16 repetition beats the fastest f32 one
        print(json.dumps(rec), flush=True)
        res.append(rec)
        del calls, pols
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
