#!/usr/bin/env python3
"""Times one step of episode bookkeeping on the GPU: EpisodeTracker.step (one rover_episode_track call: two launches, nothing read back)
against a torch restatement of what skrl's agent does in record_transition (EXPERIMENTS.md §23).

    python tools/track_timing.py [--envs 512 4096 65536] [--reps 30] [--inner 200] [--done 0.001] [--json out.json]

Per size a pool of 16 steps is drawn once — rewards in [-1, 1], done with probability --done, eight component columns (seven float32
and one int64, as RoverTask's extras) — and every variant walks through the pool in windows of --inner calls between two device events;
the windows of the variants alternate, so that a drift of the machine meets all of them.  A figure is the time of one call inside such
a window — enqueue cost and host reads included, as in a rollout —: median (min .. max) over --reps windows.
  tracker         EpisodeTracker.step, eight components
  tracker_graph   the same window captured once in a graph and replayed: the device's share of a call
  skrl            cumulative adds, nonzero() and its numel() on the host, tolist() of the finished envs' figures into two deques of 100,
                  index writes, max / min / mean of the rewards as three .item() reads, numpy max / min / mean of the deques; no components
  skrl_no_reads   the same torch ops with every read this script can remove removed: adds, nonzero, two index reads, two index writes,
                  three reductions left on the device (nonzero still waits for its own size inside torch); no ring, no components
Needs a GPU; there is no fallback."""
import argparse
import collections
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from isaac_rover_amd import _lib  # noqa: E402
from isaac_rover_amd.learning.tracking import EpisodeTracker  # noqa: E402

POOL = 16


def window(fn, inner):
    """-> microseconds per call over one event-bracketed window of ``inner`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


class Skrl:
    """skrl 1.x Agent.record_transition's bookkeeping and the part of write_tracking_data's input it prepares every step."""

    def __init__(self, e, dev, reads):
        self.cum_r = torch.zeros(e, 1, device=dev)
        self.cum_t = torch.zeros(e, 1, device=dev)
        self.track_r, self.track_t = collections.deque(maxlen=100), collections.deque(maxlen=100)
        self.data = collections.defaultdict(list)
        self.reads = reads
        self.keep = None

    def step(self, rewards, done):
        rewards, done = rewards.view(-1, 1), done.view(-1, 1)
        self.cum_r.add_(rewards)
        self.cum_t.add_(1)
        finished = done.nonzero(as_tuple=False)
        if self.reads:
            if finished.numel():
                self.track_r.extend(self.cum_r[finished][:, 0].reshape(-1).tolist())
                self.track_t.extend(self.cum_t[finished][:, 0].reshape(-1).tolist())
                self.cum_r[finished] = 0
                self.cum_t[finished] = 0
            self.data["Reward / Instantaneous reward (max)"].append(torch.max(rewards).item())
            self.data["Reward / Instantaneous reward (min)"].append(torch.min(rewards).item())
            self.data["Reward / Instantaneous reward (mean)"].append(torch.mean(rewards).item())
            if len(self.track_r):
                r, t = np.array(self.track_r), np.array(self.track_t)
                for name, a in (("Reward / Total reward", r), ("Episode / Total timesteps", t)):
                    self.data[name + " (max)"].append(np.max(a))
                    self.data[name + " (min)"].append(np.min(a))
                    self.data[name + " (mean)"].append(np.mean(a))
            if len(self.data["Reward / Instantaneous reward (max)"]) >= 1000:
                self.data.clear()
        else:
            self.keep = (self.cum_r[finished][:, 0], self.cum_t[finished][:, 0], torch.max(rewards), torch.min(rewards), torch.mean(rewards))
            self.cum_r[finished] = 0
            self.cum_t[finished] = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200, help="calls per window")
    ap.add_argument("--done", type=float, default=0.001, help="probability that an env's episode ends with a step")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_timing: needs a GPU")
    dev = torch.device("cuda", 0)
    eng = _lib.Engine(64, device=0)
    result = {"version": _lib.version(), "inner": args.inner, "reps": args.reps, "done": args.done, "sizes": {}}
    for e in args.envs:
        g = torch.Generator().manual_seed(e)
        pool = []
        for _ in range(POOL):
            extras = {k: (torch.randint(0, 3, (e,), generator=g) if k == "collision_penalty" else torch.rand(e, generator=g)).to(dev) for k in _lib.EXTRAS}
            pool.append(((2 * torch.rand(e, generator=g) - 1).to(dev), (torch.rand(e, generator=g) < args.done).long().to(dev), extras))
        tracker, graphed = (EpisodeTracker(eng, e, window=100, components=_lib.EXTRAS) for _ in range(2))
        static = (pool[0][0].clone(), pool[0][1].clone(), {k: v.clone() for k, v in pool[0][2].items()})
        graphed.step(*static)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.inner):
                graphed.step(*static)
        skrl, bare = Skrl(e, dev, True), Skrl(e, dev, False)
        calls = {"tracker": lambda i: tracker.step(*pool[i % POOL]),
                 "skrl": lambda i: skrl.step(*pool[i % POOL][:2]),
                 "skrl_no_reads": lambda i: bare.step(*pool[i % POOL][:2])}
        for fn in calls.values():                                    # warm-up: every op's code object loaded, the descriptor built
            for i in range(POOL):
                fn(i)
        torch.cuda.synchronize()
        samples = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, fn in calls.items():
                samples[name].append(window(fn, args.inner))
            samples.setdefault("tracker_graph", []).append(window(lambda i: graph.replay(), 1) / args.inner)
        rec = {name: (statistics.median(v), min(v), max(v)) for name, v in samples.items()}
        result["sizes"][str(e)] = rec
        print(f"--- {e} envs (us per call: median (min .. max); {args.inner} calls per window, {args.reps} windows, alternating; "
              f"episodes finished per step {e * args.done:.2f})")
        for name, (med, lo, hi) in rec.items():
            print(f"{name:14s} {med:10.2f} ({lo:.2f} .. {hi:.2f})")
    eng.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
