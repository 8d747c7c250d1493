#!/usr/bin/env python3
"""Times one StudentTrainer.update() (learning/distill.py: forward_train, back-propagation through time on the HIP kernels, clip + Adam as
rover_optim_step) against the same step as torch autograd with the same weights — nn.GRU (two layers, batch first), F.linear + LeakyReLU
chains, the same loss, clip_grad_norm_ + torch.optim.Adam — the only yardstick that exists.  Native width (obs 1 750, H = 300), no
resets (nn.GRU cannot reset inside a sequence).  One process: both sides are warmed up with three updates (their losses are printed: they
must agree), then `--reps` repetitions of `--inner` updates each, alternating the two, device events around each; median, min, max.

    python tools/distill_timing.py [--b 512 4096] [--t 32] [--reps 8] [--inner 3] [--out out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/distill_timing.py --b 512 --ours-only --reps 2 --inner 2

A batch size that does not fit is reported as such (torch.cuda.OutOfMemoryError), not as a failure."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from isaac_rover_amd import _lib  # noqa: E402
from isaac_rover_amd.learning.distill import StudentTrainer  # noqa: E402
from isaac_rover_amd.learning.student import DEFAULT_CFG, StudentPolicy  # noqa: E402

INFO = {"proprioceptive": 4, "sparse": 634, "dense": 1112, "actions": 2}      # the reference's native obs row (1 750 floats)
DEV = "cuda:0"


class TorchStudent:
    """Student.forward + the distillation loss from torch ops on leaf tensors (weights copied from a StudentPolicy), stepped by torch."""

    def __init__(self, sd, lr, clip):
        self.p = {k: v.detach().clone().requires_grad_(k != "MLP.log_std_parameter") for k, v in sd.items()}
        hd = sd["belief_encoder.gru.weight_hh_l0"].shape[1]
        self.gru = torch.nn.GRU(sd["belief_encoder.gru.weight_ih_l0"].shape[1], hd, num_layers=2, batch_first=True).to(DEV)
        with torch.no_grad():
            for n, t in self.gru.named_parameters():
                t.copy_(sd["belief_encoder.gru." + n])
        self.params = [v for k, v in self.p.items() if k != "MLP.log_std_parameter" and ".gru." not in k] + list(self.gru.parameters())
        self.opt = torch.optim.Adam(self.params, lr=lr)
        self.clip = clip

    def chain(self, prefix, v):
        i = 0
        while True:
            if f"{prefix}.{i}.layer.0.weight" in self.p:
                v = F.leaky_relu(F.linear(v, self.p[f"{prefix}.{i}.layer.0.weight"], self.p[f"{prefix}.{i}.layer.0.bias"]), 0.01)
            elif f"{prefix}.{i}.weight" in self.p:
                v = torch.tanh(F.linear(v, self.p[f"{prefix}.{i}.weight"], self.p[f"{prefix}.{i}.bias"]))
            else:
                return v
            i += 1

    def update(self, x, ta, h0, target):
        p, ns, nd = INFO["proprioceptive"], INFO["sparse"], INFO["dense"]
        f = x.shape[2]
        self.opt.zero_grad(set_to_none=False)
        prop, ext = x[:, :, :p], x[:, :, f - ns - nd:]
        l_e = torch.cat((self.chain("encoder1.encoder", x[:, :, f - ns - nd:f - nd]), self.chain("encoder2.encoder", x[:, :, f - nd:])), 2)
        out, h = self.gru(torch.cat((prop, l_e), 2), h0)
        belief = self.chain("belief_encoder.gb", out) + l_e * torch.sigmoid(self.chain("belief_encoder.ga", out))
        act = self.chain("MLP.network", torch.cat((prop, belief), 2))
        last = out[-1]
        est = self.chain("belief_decoder.decoder", last) + ext * torch.sigmoid(self.chain("belief_decoder.gate_encoder", last))
        la, lr_ = ((act - ta) ** 2).mean(), ((est - target) ** 2).mean()
        loss = la + 0.5 * lr_
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.params, self.clip)
        self.opt.step()
        return loss.detach()


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
    ap.add_argument("--b", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--t", type=int, default=32)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--ours-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = _lib.Engine(64, device=0)
    res = []
    for b in a.b:
        try:
            g = torch.Generator().manual_seed(b)
            f = sum(INFO[k] for k in ("proprioceptive", "sparse", "dense"))
            x = (torch.rand(b, a.t, f, generator=g) * 2 - 1).to(DEV)
            ta = (torch.rand(b, a.t, 2, generator=g) * 2 - 1).to(DEV)
            target = (x[:, :, 4:] + 0.05 * torch.randn(b, a.t, f - 4, device=DEV)).contiguous()
            h0 = torch.zeros(2, b, 300, device=DEV)
            pol = StudentPolicy(eng, INFO, DEFAULT_CFG, device=DEV, seed=1)
            sd = {k: v.clone() for k, v in pol.state_dict().items()}
            tr = StudentTrainer(eng, pol, lr=1e-4, grad_norm_clip=1.0, recon_scale=0.5)
            ours = lambda: tr.update(x, ta, h0, None, target)
            l_ours = [float(ours()[0]) for _ in range(3)]
            rec = {"B": b, "T": a.t, "rows": b * a.t, "loss_ours_first3": l_ours}
            if not a.ours_only:
                ts = TorchStudent(sd, 1e-4, 1.0)
                theirs = lambda: ts.update(x, ta, h0, target)
                rec["loss_torch_first3"] = [float(theirs()) for _ in range(3)]
            to, tt = [], []
            for _ in range(a.reps):
                to.append(timed(ours, a.inner))
                if not a.ours_only:
                    tt.append(timed(theirs, a.inner))
            med = lambda v: sorted(v)[len(v) // 2]
            rec.update(ours_ms=med(to), ours_min=min(to), ours_max=max(to))
            if tt:
                rec.update(torch_ms=med(tt), torch_min=min(tt), torch_max=max(tt))
            rec["peak_mem_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
            del pol, tr, x, ta, target
            if not a.ours_only:
                del ts
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
        except torch.cuda.OutOfMemoryError as e:
            rec = {"B": b, "T": a.t, "oom": str(e)[:200]}
            torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
        res.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
