"""Cost of the evaluation latch (rover_set_evaluation) on the fused step, BASELINE configs[2] shape by default: 65 536 envs, 37 heightmap
+ 26 rock rays, the stone_info mask on.  Times rover_step with hipEvents on two ctxs over the same scene and states, one with
evaluation on and one without, interleaved (A B A B ...), and prints one JSON line with the medians.

    python tools/eval_overhead.py [--envs 65536] [--steps 200] [--mode both|on|off]

For the metrics pass on its own (obs_metrics_kernel) run a single mode under the kernel trace, once per mode:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/eval_overhead.py --mode on
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isaac_rover_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cells", type=int, default=600)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--stones", type=int, default=1024)
    ap.add_argument("--mode", choices=("both", "on", "off"), default="both")
    args = ap.parse_args()
    e = args.envs
    dev = torch.device("cuda", 0)
    scene = synth.make_scene(n_cells=args.cells, k=args.k, n_stones=args.stones, device=dev)
    distn = synth.ray_distribution("37")
    st = synth.make_states(e, args.cells * 0.1, seed=3)
    d = {k: v.to(dev).contiguous() for k, v in st.items()}
    modes = {"both": ("off", "on"), "on": ("on",), "off": ("off",)}[args.mode]
    runs = {}
    for m in modes:
        eng = _lib.Engine(e, device=0)
        eng.set_scene(scene, distn)
        if m == "on":
            eng.set_evaluation(True)
        progress = d["progress"].clone()
        sin = eng.make_in(d["pos"], d["quat"], d["joints"], d["target"], d["lin_hist"], d["ang_hist"], d["euler_pre"], progress)
        i64 = torch.int64
        bufs = dict(rew=torch.zeros(e, device=dev), reset=torch.zeros(e, dtype=i64, device=dev),
                    rock_collision=torch.zeros(e, dtype=i64, device=dev), reset_ids=torch.zeros(e, dtype=i64, device=dev),
                    n_reset=torch.zeros(1, dtype=torch.int32, device=dev), done_u8=torch.zeros(e, dtype=torch.uint8, device=dev),
                    stone_collision=torch.zeros(e, dtype=i64, device=dev))
        obs = torch.zeros(e, eng.num_observations, device=dev)
        sout = eng.make_out(obs, stone_margin=0.0, **bufs)
        runs[m] = (eng, sin, sout, progress, [])
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for i in range(args.warmup + args.steps):
        for m in modes:
            eng, sin, sout, progress, times = runs[m]
            if i % 100 == 0:
                progress.zero_()                  # keep the batch away from a mass timeout
            if i >= args.warmup:
                a, b = ev[i - args.warmup]
                a.record()
                eng.step(sin, sout, increment_progress=True, compact=True)
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            else:
                eng.step(sin, sout, increment_progress=True, compact=True)
    torch.cuda.synchronize()
    res = {"envs": e, "rays_per_env": 26 + 37, "steps": args.steps}
    for m in modes:
        t = runs[m][4]
        res[f"step_ms_median_{m}"] = round(statistics.median(t), 4)
        res[f"step_ms_min_{m}"] = round(min(t), 4)
    if len(modes) == 2:
        res["delta_us_median"] = round(1000 * (res["step_ms_median_on"] - res["step_ms_median_off"]), 2)
    if "on" in runs:
        summ = torch.zeros(8, dtype=torch.int64, device=dev)
        runs["on"][0].eval_read(summary8=summ)
        res["summary8"] = summ.tolist()
    print(json.dumps(res))
    for m in modes:
        runs[m][0].close()


if __name__ == "__main__":
    main()
