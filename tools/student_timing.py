#!/usr/bin/env python3
"""Times StudentPolicy.act (learning/student.py: rover_gru_cell per GRU layer, rover_gated_sum, the chain kernels) against the same step
built from torch modules with the same weights — nn.Linear + LeakyReLU encoders, nn.GRU, the gb / ga branches, the MLP with its
Tanh head — the only yardstick that exists.  Both are captured in a graph after a warm-up and timed with device events around a
replay: `--reps` repetitions each, alternating the two; median and spread (min, 10th / 90th percentile).

    python tools/student_timing.py [--envs 512,65536] [--reps 100] [--json out.json]

Also prints the GRU's arithmetic counted from shapes (2 * 3 * H * (K + H) flop per row and layer) over the measured time of the
whole step, as TFLOP/s: an end-to-end rate, not a kernel's share of peak."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

INFO = {"proprioceptive": 4, "sparse": 634, "dense": 1112, "actions": 2}      # the reference's native obs row (1 750 floats)


class TorchStudent(torch.nn.Module):
    """student_loader.act's arithmetic (no decoder: act() drops its output) from torch modules, weights copied from a StudentPolicy."""

    def __init__(self, pol):
        super().__init__()
        sd = pol.state_dict()

        def chain(prefix, head=False):
            mods, i = [], 0
            while f"{prefix}.{i}.layer.0.weight" in sd or f"{prefix}.{i}.weight" in sd:
                plain = f"{prefix}.{i}.layer.0.weight" not in sd      # the head's bare nn.Linear, followed by nn.Tanh
                stem = f"{prefix}.{i}" if plain else f"{prefix}.{i}.layer.0"
                w = sd[stem + ".weight"]
                lin = torch.nn.Linear(w.shape[1], w.shape[0], device=w.device)
                lin.weight.data.copy_(w)
                lin.bias.data.copy_(sd[stem + ".bias"])
                mods += [lin, torch.nn.Tanh() if plain else torch.nn.LeakyReLU()]
                i += 1
            return torch.nn.Sequential(*mods)

        self.e1, self.e2 = chain("encoder1.encoder"), chain("encoder2.encoder")
        self.gb, self.ga, self.mlp = chain("belief_encoder.gb"), chain("belief_encoder.ga"), chain("MLP.network")
        k = sd["belief_encoder.gru.weight_ih_l0"].shape[1]
        self.gru = torch.nn.GRU(k, pol.hidden_dim, pol.n_layers, batch_first=True, device=pol.device)
        for name, p in self.gru.named_parameters():
            p.data.copy_(sd["belief_encoder.gru." + name])
        self.p, self.ns, self.nd = pol.info["proprioceptive"], pol.info["sparse"], pol.info["dense"]

    @torch.no_grad()
    def forward(self, obs, h):
        f = obs.shape[1]
        prop = obs[:, :self.p]
        l_e = torch.cat((self.e1(obs[:, f - self.ns - self.nd:f - self.nd]), self.e2(obs[:, f - self.nd:])), 1)
        out, hn = self.gru(torch.cat((prop, l_e), 1).unsqueeze(1), h)
        out = out[:, 0]
        belief = self.gb(out) + l_e * torch.sigmoid(self.ga(out))
        h.copy_(hn)
        return self.mlp(torch.cat((prop, belief), 1))


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
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="512,65536")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "student_timing needs a GPU (a CPU run says nothing about it)"
    from isaac_rover_amd import _lib
    from isaac_rover_amd.learning.student import StudentPolicy
    results = []
    for e in [int(v) for v in args.envs.split(",")]:
        eng = _lib.Engine(e, device=0)
        pol = StudentPolicy(eng, INFO, device="cuda:0", seed=1)
        pol.init_hidden(e)
        ref = TorchStudent(pol)
        obs = torch.rand(e, sum(INFO[k] for k in ("proprioceptive", "sparse", "dense")), device="cuda:0") * 2 - 1
        h_ref = torch.zeros_like(pol.h)
        d = float((pol.act(obs) - ref(obs, h_ref)).abs().max())
        graphs = {"hip": capture(lambda: pol.act(obs)), "torch": capture(lambda: ref(obs, h_ref))}
        times = {k: [] for k in graphs}
        for _ in range(args.reps):
            for k, g in graphs.items():                              # alternating
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g.replay()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3)
        hd, k0 = pol.hidden_dim, INFO["proprioceptive"] + 120
        flop = sum(2 * 3 * hd * (k + hd) for k in [k0] + [hd] * (pol.n_layers - 1)) * e
        row = {"envs": e, "route": eng.gru_cell_route(e, k0, hd), "max_abs_diff_first_step": d, "gru_gflop": flop / 1e9}
        for k, v in times.items():
            v = np.array(v)
            row[k + "_us"] = {"median": float(np.median(v)), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}
        row["gru_tflops_over_hip_step"] = flop / (row["hip_us"]["median"] * 1e-6) / 1e12
        results.append(row)
        print(json.dumps(row))
        eng.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
